// BN254 Fq2 = Fq[u] / (u^2 + 1) on the 29-bit-limb internal representation of bn254_fq29.hip.h: the field of the G2
// kernels (bn254_ec2_29.hip.h).  An element is two fe29 (c0 + c1 u) in the internal Montgomery domain rho = 2^261;
// the external form is the one of halo2curves / arkworks (c0, c1 each 8 x u32 little-endian, Montgomery R = 2^256).
//
// Bounds contract (multiples of p, per component; rho' = p / rho = 0.0059).  Every fq2 that enters a multiplication
// is NORMALISED: limbs 0..7 < 2^29 + 8, limb 8 < 2^28 (any value < 64 p), so every column sum of Fq29::mul / mul2
// stays below 2^63 whatever the value; the value bounds below only decide the output bounds.  tools/g2_bounds.py
// re-derives every figure this header and bn254_ec2_29.hip.h quote.
//   add(a, b)      : a + b limb-wise, NOT normalised (limbs < 2^30 + 16): norm() before a multiplication
//   sub<K>(a, b)   : a - b + K p, normalised; b < K p (K = 4, 8, 16 through the lifted constants of Fq29, K = 32
//                    through twice the K16E30 limbs: 2 kc(K16E30, i) - b_i > 0 for normalised b, < 2^32)
//   neg(a)         : 32 p - a, normalised; a < 32 p
//   mul(a, b)      : c0 = a0 b0 + a1 (32 p - b1), c1 = a0 b1 + a1 b0, each ONE double product (Fq29::mul2, masked
//                    quotient digits): 4 + 4 limb-product sets and 2 reductions, the cost of Karatsuba's three
//                    products and reductions but without its (a0 + a1)(b0 + b1) operands;  b1 < 32 p
//                    c0 < (1 + rho' (A0 B0 + 32 A1)) p,  c1 < (1 + rho' (A0 B1 + A1 B0)) p
//   sqr(a)         : c0 = (a0 + a1)(a0 - a1 + 32 p), c1 = (2 a0) a1: two single products;  a1 < 32 p
//                    c0 < (1 + rho' (A0 + A1)(A0 + 32)) p,  c1 < (1 + rho' 2 A0 A1) p
//   squash(a)      : a * (rho mod p) / rho = a, value < (1 + rho' A) p: brings any operand back to ~1 p
//   inv_fq(a)      : Fq inversion a^(p-2) on fe29 (0 -> 0); a a valid Fq29::mul operand, value < A p with A <= 32;
//                    result a multiplication output (exact limbs), value < (1 + 1.02 rho' A) p <= 1.2 p
//   inv(a)         : conj(a) (a0^2 + a1^2)^-1, ONE inv_fq (0 -> 0);  a normalised, a < 32 p
//                    n = norm_fq(a) < (1 + rho' 2 A^2) p <= 13.1 p,  n^-1 < (1 + 1.02 rho' 13.1) p < 1.08 p,
//                    c0 = a0 n^-1, c1 = (32 p - a1) n^-1: multiplication outputs (exact limbs) < (1 + rho' 32 * 1.08) p
//                    < 1.21 p
//   to_ext / is_zero_exact : any normalised operand < 64 p
#pragma once
#include "bn254_fq29.hip.h"

#if defined(__HIPCC__)
#define MSM_NO_UNROLL _Pragma("unroll 1")
#else
#define MSM_NO_UNROLL
#endif

namespace msm_amd {

struct fq2 {
  fe29 c0, c1;
};

struct Fq2 {
  MSM_HD static fq2 zero() { return fq2{Fq29::zero(), Fq29::zero()}; }
  MSM_HD static fq2 one() { return fq2{Fq29::one(), Fq29::zero()}; }
  MSM_HD static bool is_zero_limbs(const fq2& a) { return Fq29::is_zero_limbs(a.c0) && Fq29::is_zero_limbs(a.c1); }

  MSM_HD static fq2 add(const fq2& a, const fq2& b) { return fq2{Fq29::add(a.c0, b.c0), Fq29::add(a.c1, b.c1)}; }
  MSM_HD static fq2 norm(const fq2& a) { return fq2{Fq29::norm(a.c0), Fq29::norm(a.c1)}; }

  // a - b + K p on one component, normalised (see the contract above)
  template <int K>
  MSM_HD static fe29 sub1(const fe29& a, const fe29& b) {
    static_assert(K == 4 || K == 8 || K == 16 || K == 32, "lifted multiples: 4, 8, 16, 32 p");
    if (K == 4) return Fq29::norm(Fq29::sub<K4E30>(a, b));
    if (K == 8) return Fq29::norm(Fq29::sub<K8E30>(a, b));
    if (K == 16) return Fq29::norm(Fq29::sub<K16E30>(a, b));
    fe29 r;
    MSM_UNROLL for (int i = 0; i < 9; ++i) r.l[i] = (a.l[i] + 2u * Fq29::kc(K16E30, i)) - b.l[i];
    return Fq29::norm(r);
  }
  template <int K>
  MSM_HD static fq2 sub(const fq2& a, const fq2& b) {
    return fq2{sub1<K>(a.c0, b.c0), sub1<K>(a.c1, b.c1)};
  }
  MSM_HD static fq2 neg(const fq2& a) { return sub<32>(zero(), a); }

  MSM_HD static fq2 mul(const fq2& a, const fq2& b) {
    const fe29 nb1 = sub1<32>(Fq29::zero(), b.c1);
    return fq2{Fq29::mul2(a.c0, b.c0, a.c1, nb1), Fq29::mul2(a.c0, b.c1, a.c1, b.c0)};
  }
  MSM_HD static fq2 sqr(const fq2& a) {
    const fe29 s = Fq29::norm(Fq29::add(a.c0, a.c1));
    const fe29 d = sub1<32>(a.c0, a.c1);
    const fe29 t = Fq29::norm(Fq29::add(a.c0, a.c0));
    return fq2{Fq29::mul(s, d), Fq29::mul(t, a.c1)};
  }
  MSM_HD static fq2 squash(const fq2& a) { return fq2{Fq29::mul(a.c0, Fq29::one()), Fq29::mul(a.c1, Fq29::one())}; }

  // a0^2 + a1^2 (the norm to Fq; an element of Fq2 is invertible iff it is non-zero); a < 32 p: < (1 + rho' 2 A^2) p
  MSM_HD static fe29 norm_fq(const fq2& a) { return Fq29::mul2(a.c0, a.c0, a.c1, a.c1); }

  // Fq inversion a^-1 = a^(p - 2) by square-and-multiply over the fixed exponent, most significant bit first (the 7
  // leading zero bits of the top limb square `one`): 261 squarings, one multiplication per set bit.  The running power
  // r stays below 1.02 p before every multiplication (r < 1 + rho' 1.02 * 32 = 1.2 p after a multiplication by
  // a < 32 p, < 1.01 p after the next squaring), so every operand is a valid one, and the result -- bit 0 of p - 2 is
  // set, it ends on a multiplication -- is < (1 + rho' 1.02 A) p.  Set-up code (the table build): the loops are not
  // unrolled, the exponent limbs are immediates.
  MSM_HD static fe29 inv_fq(const fe29& a) {
    fe29 r = Fq29::one();
    MSM_NO_UNROLL for (int j = 8; j >= 0; --j) {
      uint32_t e = 0;   // limb j of p - 2 (p(0) >= 2: only limb 0 differs from p)
      MSM_UNROLL for (int k = 0; k < 9; ++k) e = (k == j) ? (Fq29::p(k) - (k == 0 ? 2u : 0u)) : e;
      MSM_NO_UNROLL for (int b = 28; b >= 0; --b) {
        r = Fq29::sqr(r);
        if ((e >> b) & 1u) r = Fq29::mul(r, a);
      }
    }
    return r;
  }

  // a^-1 = conj(a) / (a0^2 + a1^2); a normalised, < 32 p (see the contract above)
  MSM_HD static fq2 inv(const fq2& a) {
    const fe29 ninv = inv_fq(norm_fq(a));
    return fq2{Fq29::mul(a.c0, ninv), Fq29::mul(sub1<32>(Fq29::zero(), a.c1), ninv)};
  }

  // a == 0 needs both components zero; `bound`: a < bound p for the one-limb filter of each component
  MSM_HD static bool maybe_zero(const fq2& a, uint32_t bound) {
    return Fq29::maybe_zero(a.c0, bound) && Fq29::maybe_zero(a.c1, bound);
  }
  MSM_HD static bool is_zero_exact(const fq2& a) { return Fq29::is_zero_exact(a.c0) && Fq29::is_zero_exact(a.c1); }

  // external (Montgomery R = 2^256, canonical) <-> internal
  MSM_HD static fq2 from_ext(const u256& c0, const u256& c1) { return fq2{Fq29::from_ext(c0), Fq29::from_ext(c1)}; }
  MSM_HD static void to_ext(const fq2& a, u256& c0, u256& c1) {
    c0 = Fq29::to_ext(a.c0);
    c1 = Fq29::to_ext(a.c1);
  }
};

}  // namespace msm_amd
