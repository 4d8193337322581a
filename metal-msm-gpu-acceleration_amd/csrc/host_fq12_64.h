// Host-only BN254 Fq6 / Fq12 arithmetic and the optimal ate pairing on the 4 x 64-bit limbs of host_fq64.h /
// host_fq2_64.h: the twin of bn254_fq12_29.hip.h, sharing none of its arithmetic.  Where the device code accumulates
// schoolbook sums in lazy columns, this is the usual Karatsuba tower on fully reduced values:
//   Fq6 = Fq2[v] / (v^3 - xi), xi = 9 + u;  Fq12 = Fq6[w] / (w^2 - v);  c_h.c_k is the coefficient of w^(2k + h).
// The Miller loop uses the same projective steps with the same scaling of T and of the lines, so a Miller product
// (MSM_AMD_PAIRING_MILLER_ONLY) has the same bytes on both sides; the GT element is unique anyway.
// Constants: tools/gen_fq12_constants.py host.
#pragma once
#include <vector>

#include "host_fq2_64.h"

namespace msm_amd {
namespace h64 {

struct Fe6 {
  Fe2 c0, c1, c2;
};
struct Fe12 {
  Fe6 c0, c1;
};

constexpr uint64_t kHostBnX = 4965661367192848881ull;
constexpr uint64_t kHostAtePos = 0xA1818041C0864428ull, kHostAteNeg = 0x0408100802100880ull;
enum : int { kRowXi = 0, kRowB3 = 2, kRowGamma = 4, kRowRadix = 34 };
inline Fe k64(int r) {
  static const uint64_t c[35][4] = {
#include "host_fq12_64_consts.inc"
  };
  Fe f;
  for (int i = 0; i < 4; ++i) f.v[i] = c[r][i];
  return f;
}
inline Fe2 k64_pair(int r) { return Fe2{k64(r), k64(r + 1)}; }
inline Fe2 gamma64(int k, int i) { return i == 0 ? one2() : k64_pair(kRowGamma + 2 * (5 * (k - 1) + (i - 1))); }

inline Fe2 conj2(const Fe2& a) {
  Fe z;
  std::memset(&z, 0, sizeof z);
  return Fe2{a.c0, sub(z, a.c1)};
}
inline Fe2 scale2(const Fe2& a, const Fe& s) { return Fe2{mul(a.c0, s), mul(a.c1, s)}; }
inline Fe2 mul_xi(const Fe2& a) {   // (9 + u)(a0 + a1 u) = 9 a0 - a1 + (9 a1 + a0) u
  const Fe2 a8 = dbl2(dbl2(dbl2(a))), a9 = add2(a8, a);
  return Fe2{sub(a9.c0, a.c1), add(a9.c1, a.c0)};
}

inline Fe6 add6(const Fe6& a, const Fe6& b) { return Fe6{add2(a.c0, b.c0), add2(a.c1, b.c1), add2(a.c2, b.c2)}; }
inline Fe6 sub6(const Fe6& a, const Fe6& b) { return Fe6{sub2(a.c0, b.c0), sub2(a.c1, b.c1), sub2(a.c2, b.c2)}; }
inline Fe6 neg6(const Fe6& a) { return Fe6{neg2(a.c0), neg2(a.c1), neg2(a.c2)}; }
inline Fe6 mul_v(const Fe6& a) { return Fe6{mul_xi(a.c2), a.c0, a.c1}; }
inline Fe6 mul6(const Fe6& a, const Fe6& b) {   // Karatsuba, six Fq2 products
  const Fe2 v0 = mul2(a.c0, b.c0), v1 = mul2(a.c1, b.c1), v2 = mul2(a.c2, b.c2);
  const Fe2 t0 = sub2(sub2(mul2(add2(a.c1, a.c2), add2(b.c1, b.c2)), v1), v2);
  const Fe2 t1 = sub2(sub2(mul2(add2(a.c0, a.c1), add2(b.c0, b.c1)), v0), v1);
  const Fe2 t2 = sub2(sub2(mul2(add2(a.c0, a.c2), add2(b.c0, b.c2)), v0), v2);
  return Fe6{add2(v0, mul_xi(t0)), add2(t1, mul_xi(v2)), add2(t2, v1)};
}
inline Fe6 scale6(const Fe6& a, const Fe2& s) { return Fe6{mul2(a.c0, s), mul2(a.c1, s), mul2(a.c2, s)}; }
inline Fe6 inv6(const Fe6& a) {
  const Fe2 A = sub2(sqr2(a.c0), mul_xi(mul2(a.c1, a.c2)));
  const Fe2 B = sub2(mul_xi(sqr2(a.c2)), mul2(a.c0, a.c1));
  const Fe2 C = sub2(sqr2(a.c1), mul2(a.c0, a.c2));
  const Fe2 F = add2(mul2(a.c0, A), mul_xi(add2(mul2(a.c2, B), mul2(a.c1, C))));
  return scale6(Fe6{A, B, C}, inv2(F));
}
inline Fe6 zero6() { return Fe6{zero2(), zero2(), zero2()}; }

inline Fe12 one12() { return Fe12{Fe6{one2(), zero2(), zero2()}, zero6()}; }
inline Fe12 mul12(const Fe12& a, const Fe12& b) {
  const Fe6 aa = mul6(a.c0, b.c0), bb = mul6(a.c1, b.c1);
  const Fe6 cc = mul6(add6(a.c0, a.c1), add6(b.c0, b.c1));
  return Fe12{add6(aa, mul_v(bb)), sub6(sub6(cc, aa), bb)};
}
inline Fe12 sqr12(const Fe12& a) {   // complex squaring: two Fq6 products
  const Fe6 ab = mul6(a.c0, a.c1);
  const Fe6 t = mul6(add6(a.c0, a.c1), add6(a.c0, mul_v(a.c1)));
  return Fe12{sub6(sub6(t, ab), mul_v(ab)), add6(ab, ab)};
}
inline Fe12 conj12(const Fe12& a) { return Fe12{a.c0, neg6(a.c1)}; }
inline Fe12 inv12(const Fe12& a) {
  const Fe6 t = inv6(sub6(mul6(a.c0, a.c0), mul_v(mul6(a.c1, a.c1))));
  return Fe12{mul6(a.c0, t), neg6(mul6(a.c1, t))};
}
// a^(p^k), k = 1 .. 3
inline Fe12 frob12(const Fe12& a, int k) {
  const Fe2* src[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
  Fe2 dst[6];
  for (int r = 0; r < 6; ++r) {
    const int i = 2 * (r % 3) + r / 3;   // the power of w
    dst[r] = mul2((k & 1) ? conj2(*src[r]) : *src[r], gamma64(k, i));
  }
  return Fe12{Fe6{dst[0], dst[1], dst[2]}, Fe6{dst[3], dst[4], dst[5]}};
}

// Granger-Scott squaring in the cyclotomic subgroup
inline void sqr4(const Fe2& a, const Fe2& b, Fe2& t0, Fe2& t1) {   // (a + b y)^2, y^2 = xi
  const Fe2 ab = mul2(a, b);
  t0 = sub2(sub2(mul2(add2(a, b), add2(mul_xi(b), a)), ab), mul_xi(ab));
  t1 = dbl2(ab);
}
inline Fe12 cyclo_sqr12(const Fe12& a) {
  const Fe2 &z0 = a.c0.c0, &z4 = a.c0.c1, &z3 = a.c0.c2, &z2 = a.c1.c0, &z1 = a.c1.c1, &z5 = a.c1.c2;
  Fe2 t0, t1, t2, t3, t4, t5;
  sqr4(z0, z1, t0, t1);
  sqr4(z2, z3, t2, t3);
  sqr4(z4, z5, t4, t5);
  auto three_minus = [](const Fe2& t, const Fe2& z) { return add2(dbl2(sub2(t, z)), t); };   // 3 t - 2 z
  auto three_plus = [](const Fe2& t, const Fe2& z) { return add2(dbl2(add2(t, z)), t); };     // 3 t + 2 z
  Fe12 r;
  r.c0.c0 = three_minus(t0, z0);
  r.c1.c1 = three_plus(t1, z1);
  r.c1.c0 = three_plus(mul_xi(t5), z2);
  r.c0.c2 = three_minus(t4, z3);
  r.c0.c1 = three_minus(t2, z4);
  r.c1.c2 = three_plus(t3, z5);
  return r;
}
inline Fe12 pow_x12(const Fe12& a) {
  Fe12 r = a;
  for (int b = 61; b >= 0; --b) {
    r = cyclo_sqr12(r);
    if ((kHostBnX >> b) & 1u) r = mul12(r, a);
  }
  return r;
}

// f^((p^12 - 1) / r), the exact exponent: easy part, then the base-p digits of (p^4 - p^2 + 1) / r gathered as
// y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36 (Devegili, Scott, Dahab)
inline Fe12 final_exp12(const Fe12& f0) {
  Fe12 f = mul12(conj12(f0), inv12(f0));
  f = mul12(frob12(f, 2), f);
  const Fe12 fx = pow_x12(f), fx2 = pow_x12(fx), fx3 = pow_x12(fx2);
  const Fe12 y0 = mul12(mul12(frob12(f, 1), frob12(f, 2)), frob12(f, 3));
  const Fe12 y1 = conj12(f), y2 = frob12(fx2, 2), y3 = conj12(frob12(fx, 1));
  const Fe12 y4 = conj12(mul12(fx, frob12(fx2, 1))), y5 = conj12(fx2), y6 = conj12(mul12(fx3, frob12(fx3, 1)));
  Fe12 t0 = mul12(mul12(cyclo_sqr12(y6), y4), y5);
  Fe12 t1 = mul12(mul12(y3, y5), t0);
  t0 = mul12(t0, y2);
  t1 = cyclo_sqr12(mul12(cyclo_sqr12(t1), t0));
  t0 = mul12(t1, y1);
  t1 = mul12(t1, y0);
  return mul12(cyclo_sqr12(t0), t1);
}

// ---- Miller loop ------------------------------------------------------------------------------------------------------------
struct Proj2 {
  Fe2 x, y, z;
};
struct Line12 {   // l0 + l1 w + l3 w^3
  Fe2 l0, l1, l3;
};
inline Fe12 mul_line12(const Fe12& f, const Line12& l) {
  const Fe12 s{Fe6{l.l0, zero2(), zero2()}, Fe6{l.l1, l.l3, zero2()}};
  return mul12(f, s);
}
inline Fe neg1(const Fe& a) {
  Fe z;
  std::memset(&z, 0, sizeof z);
  return sub(z, a);
}
// the steps of bn254_fq12_29.hip.h (double_step, add_step), value for value
inline Line12 double_step64(Proj2& T, const Fe& xp, const Fe& yp) {
  const Fe2 b = sqr2(T.y), c = sqr2(T.z);
  const Fe2 e = mul2(k64_pair(kRowB3), c);
  const Fe2 f = add2(dbl2(e), e);
  const Fe2 h = dbl2(mul2(T.y, T.z));
  const Fe2 j = sqr2(T.x);
  const Fe2 e2 = sqr2(dbl2(e));
  Line12 l{scale2(h, neg1(yp)), scale2(add2(dbl2(j), j), xp), sub2(e, b)};
  const Fe2 x3 = mul2(dbl2(mul2(T.x, T.y)), sub2(b, f));
  const Fe2 y3 = sub2(sqr2(add2(b, f)), add2(dbl2(e2), e2));
  T.z = mul2(dbl2(b), dbl2(h));
  T.x = x3;
  T.y = y3;
  return l;
}
inline Line12 add_step64(Proj2& T, const Fe2& qx, const Fe2& qy, const Fe& xp, const Fe& yp) {
  const Fe2 theta = sub2(T.y, mul2(qy, T.z)), lam = sub2(T.x, mul2(qx, T.z));
  const Fe2 c = sqr2(theta), d = sqr2(lam);
  const Fe2 e = mul2(lam, d), f = mul2(T.z, c), g = mul2(T.x, d);
  const Fe2 h = sub2(add2(e, f), dbl2(g));
  Line12 l{scale2(lam, yp), scale2(theta, neg1(xp)), sub2(mul2(theta, qx), mul2(lam, qy))};
  const Fe2 y3 = sub2(mul2(theta, sub2(g, h)), mul2(e, T.y));
  T.x = mul2(lam, h);
  T.y = y3;
  T.z = mul2(T.z, e);
  return l;
}

struct Pair64 {   // one pair, neither point the identity
  Fe xp, yp;
  Fe2 qx, qy;
};
// the product of the Miller values of m pairs, f squared once per step for all of them
inline Fe12 miller_product64(const Pair64* pairs, size_t m) {
  Fe12 f = one12();
  if (m == 0) return f;
  std::vector<Proj2> T(m);
  for (size_t i = 0; i < m; ++i) T[i] = Proj2{pairs[i].qx, pairs[i].qy, one2()};
  for (int b = 63; b >= 0; --b) {
    if (b != 63) f = sqr12(f);
    const bool pos = (kHostAtePos >> b) & 1u, neg = (kHostAteNeg >> b) & 1u;
    for (size_t i = 0; i < m; ++i) {
      const Pair64& p = pairs[i];
      f = mul_line12(f, double_step64(T[i], p.xp, p.yp));
      if (pos || neg) f = mul_line12(f, add_step64(T[i], p.qx, pos ? p.qy : neg2(p.qy), p.xp, p.yp));
    }
  }
  for (size_t i = 0; i < m; ++i) {
    const Pair64& p = pairs[i];
    const Fe2 q1x = mul2(conj2(p.qx), gamma64(1, 2)), q1y = mul2(conj2(p.qy), gamma64(1, 3));
    const Fe2 q2x = mul2(p.qx, gamma64(2, 2)), q2y = neg2(mul2(p.qy, gamma64(2, 3)));
    f = mul_line12(f, add_step64(T[i], q1x, q1y, p.xp, p.yp));
    f = mul_line12(f, add_step64(T[i], q2x, q2y, p.xp, p.yp));
  }
  return f;
}

// ---- records: 12 fields of 32 bytes in the tower order; layout 0 Montgomery, 1 canonical ------------------------------------
inline Fe field_from64(const uint8_t* p, int layout) {   // any 256-bit value, taken mod p
  Fe x;
  std::memcpy(&x, p, 32);
  Fe plain1;
  std::memset(&plain1, 0, sizeof plain1);
  plain1.v[0] = 1;
  const Fe xr = mul(x, k64(kRowRadix));                  // x 2^256: also the canonical -> Montgomery step
  return layout == 0 ? mul(xr, plain1) : xr;
}
inline void field_to64(uint8_t* p, const Fe& a, int layout) {
  Fe plain1;
  std::memset(&plain1, 0, sizeof plain1);
  plain1.v[0] = 1;
  const Fe r = layout == 0 ? a : mul(a, plain1);
  std::memcpy(p, &r, 32);
}
inline Fe12 gt_from_record64(const uint8_t* rec, int layout) {
  Fe2 c[6];
  for (int r = 0; r < 6; ++r) c[r] = Fe2{field_from64(rec + 64 * r, layout), field_from64(rec + 64 * r + 32, layout)};
  return Fe12{Fe6{c[0], c[1], c[2]}, Fe6{c[3], c[4], c[5]}};
}
inline void gt_to_record64(uint8_t* rec, const Fe12& a, int layout) {
  const Fe2* c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
  for (int r = 0; r < 6; ++r) {
    field_to64(rec + 64 * r, c[r]->c0, layout);
    field_to64(rec + 64 * r + 32, c[r]->c1, layout);
  }
}
inline bool is_one12(const Fe12& a) {
  const Fe12 o = one12();
  return std::memcmp(&a, &o, sizeof a) == 0;
}

}  // namespace h64
}  // namespace msm_amd
