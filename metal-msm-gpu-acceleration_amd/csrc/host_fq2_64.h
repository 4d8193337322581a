// Host-only BN254 Fq2 / G2 arithmetic on the 4 x 64-bit limbs of host_fq64.h: the CPU tail of a G2 MSM (the Horner
// pass over the window partial sums and the final normalisation, host_combine_g2 in msm_host.hip), the CPU G2 MSM
// (msm_amd_host_msm_g2, host_msm.hip) and the host progression generator of the tests.  A second implementation next
// to the 29-bit-limb device code (bn254_fq2_29.hip.h, bn254_ec2_29.hip.h), sharing none of its arithmetic.
// External form throughout: Montgomery R = 2^256, canonical, c0 then c1.
#pragma once
#include "host_fq64.h"

namespace msm_amd {
namespace h64 {

struct Fe2 {
  Fe c0, c1;
};
struct Jac2 {   // same 192-byte layout as Jacobian2
  Fe2 x, y, z;
};
struct Aff2 {   // same 128-byte layout as Affine2 (halo2curves G2Affine); (0, 0) = identity
  Fe2 x, y;
};

inline bool is_zero2(const Fe2& a) { return is_zero(a.c0) && is_zero(a.c1); }
inline Fe2 add2(const Fe2& a, const Fe2& b) { return Fe2{add(a.c0, b.c0), add(a.c1, b.c1)}; }
inline Fe2 sub2(const Fe2& a, const Fe2& b) { return Fe2{sub(a.c0, b.c0), sub(a.c1, b.c1)}; }
inline Fe2 dbl2(const Fe2& a) { return add2(a, a); }
inline Fe2 neg2(const Fe2& a) {
  Fe z;
  std::memset(&z, 0, sizeof z);
  return Fe2{sub(z, a.c0), sub(z, a.c1)};
}
// Karatsuba: (a0 + a1 u)(b0 + b1 u) = a0 b0 - a1 b1 + ((a0 + a1)(b0 + b1) - a0 b0 - a1 b1) u
inline Fe2 mul2(const Fe2& a, const Fe2& b) {
  const Fe t0 = mul(a.c0, b.c0), t1 = mul(a.c1, b.c1);
  const Fe t2 = mul(add(a.c0, a.c1), add(b.c0, b.c1));
  return Fe2{sub(t0, t1), sub(sub(t2, t0), t1)};
}
inline Fe2 sqr2(const Fe2& a) {   // (a0 + a1)(a0 - a1) + 2 a0 a1 u
  return Fe2{mul(add(a.c0, a.c1), sub(a.c0, a.c1)), dbl(mul(a.c0, a.c1))};
}
inline Fe2 one2() {
  Fe2 r;
  r.c0 = one();
  std::memset(&r.c1, 0, sizeof r.c1);
  return r;
}
inline Fe2 zero2() {
  Fe2 r;
  std::memset(&r, 0, sizeof r);
  return r;
}
inline Fe2 inv2(const Fe2& a) {   // (a0 - a1 u) / (a0^2 + a1^2); inv2(0) = 0
  const Fe t = inv(add(sqr(a.c0), sqr(a.c1)));
  Fe z;
  std::memset(&z, 0, sizeof z);
  return Fe2{mul(a.c0, t), mul(sub(z, a.c1), t)};
}
inline bool eq2(const Fe2& a, const Fe2& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

inline bool is_identity2(const Jac2& p) { return is_zero2(p.z); }
inline Jac2 identity2() {
  Jac2 r;
  r.x = one2();
  r.y = one2();
  r.z = zero2();
  return r;
}
inline bool aff2_is_identity(const Aff2& a) { return is_zero2(a.x) && is_zero2(a.y); }
inline Jac2 from_aff2(const Aff2& a) {
  if (aff2_is_identity(a)) return identity2();
  return Jac2{a.x, a.y, one2()};
}

// dbl-2009-l, a = 0 (2M + 5S), the formulas of jdouble
inline Jac2 jdouble2(const Jac2& p) {
  if (is_identity2(p)) return p;
  const Fe2 A = sqr2(p.x);
  const Fe2 B = sqr2(p.y);
  const Fe2 C = sqr2(B);
  const Fe2 D = dbl2(sub2(sub2(sqr2(add2(p.x, B)), A), C));
  const Fe2 E = add2(dbl2(A), A);
  const Fe2 F = sqr2(E);
  Jac2 r;
  r.x = sub2(F, dbl2(D));
  r.y = sub2(mul2(E, sub2(D, r.x)), dbl2(dbl2(dbl2(C))));
  r.z = dbl2(mul2(p.y, p.z));
  return r;
}

// add-2007-bl with the case analysis of jadd
inline Jac2 jadd2(const Jac2& p, const Jac2& q) {
  if (is_identity2(p)) return q;
  if (is_identity2(q)) return p;
  const Fe2 Z1Z1 = sqr2(p.z);
  const Fe2 Z2Z2 = sqr2(q.z);
  const Fe2 U1 = mul2(p.x, Z2Z2);
  const Fe2 U2 = mul2(q.x, Z1Z1);
  const Fe2 S1 = mul2(mul2(p.y, q.z), Z2Z2);
  const Fe2 S2 = mul2(mul2(q.y, p.z), Z1Z1);
  const Fe2 H = sub2(U2, U1);
  const Fe2 rr = sub2(S2, S1);
  if (is_zero2(H)) {
    if (is_zero2(rr)) return jdouble2(p);
    return identity2();
  }
  const Fe2 I = sqr2(dbl2(H));
  const Fe2 J = mul2(H, I);
  const Fe2 r2 = dbl2(rr);
  const Fe2 V = mul2(U1, I);
  Jac2 r;
  r.x = sub2(sub2(sqr2(r2), J), dbl2(V));
  r.y = sub2(mul2(r2, sub2(V, r.x)), dbl2(mul2(S1, J)));
  r.z = mul2(sub2(sub2(sqr2(add2(p.z, q.z)), Z1Z1), Z2Z2), H);
  return r;
}

// madd-2007-bl (Jacobian + affine, 7M + 4S): the CPU MSM's bucket additions; q not the identity
inline Jac2 jmadd2(const Jac2& p, const Aff2& q) {
  if (is_identity2(p)) return from_aff2(q);
  const Fe2 Z1Z1 = sqr2(p.z);
  const Fe2 U2 = mul2(q.x, Z1Z1);
  const Fe2 S2 = mul2(q.y, mul2(p.z, Z1Z1));
  const Fe2 H = sub2(U2, p.x);
  const Fe2 rr0 = sub2(S2, p.y);
  if (is_zero2(H)) {
    if (is_zero2(rr0)) return jdouble2(p);
    return identity2();
  }
  const Fe2 HH = sqr2(H);
  const Fe2 I = dbl2(dbl2(HH));
  const Fe2 J = mul2(H, I);
  const Fe2 r2 = dbl2(rr0);
  const Fe2 V = mul2(p.x, I);
  Jac2 r;
  r.x = sub2(sub2(sqr2(r2), J), dbl2(V));
  r.y = sub2(mul2(r2, sub2(V, r.x)), dbl2(mul2(p.y, J)));
  r.z = sub2(sub2(sqr2(add2(p.z, H)), Z1Z1), HH);
  return r;
}

// (X, Y, Z) -> (X / Z^2, Y / Z^3, (R mod p, 0)), or the identity ((R, 0), (R, 0), (0, 0))
inline Jac2 normalise2(const Jac2& p) {
  if (is_identity2(p)) return identity2();
  const Fe2 zi = inv2(p.z);
  const Fe2 zi2 = sqr2(zi);
  Jac2 r;
  r.x = mul2(p.x, zi2);
  r.y = mul2(p.y, mul2(zi2, zi));
  r.z = one2();
  return r;
}

}  // namespace h64
}  // namespace msm_amd
