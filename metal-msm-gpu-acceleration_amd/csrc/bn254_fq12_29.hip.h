// BN254 Fq6 / Fq12 and the steps of the optimal ate pairing on the 29-bit-limb Fq2 of bn254_fq2_29.hip.h: what
// k_pairing.hip runs one lane per group of pairs, and what msm_amd_test_fq12_op taps (on the device and on the host).
//
// Tower: Fq6 = Fq2[v] / (v^3 - xi), xi = 9 + u;  Fq12 = Fq6[w] / (w^2 - v).  An fq12 is kept as the six Fq2 coefficients of
// w^0 .. w^5 (v = w^2: the tower coefficient c_h.c_k is c[2k + h]); the 384-byte record and the 108-word raw record
// list the tower order c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2.
//
// How the products are formed.  A lifted subtraction adds its K p to the value, and a multiplication by xi = 9 + u
// multiplies it by ten, so a Karatsuba tower on lazy limbs is not closed under its own bounds.  Every product here is
// therefore a schoolbook sum of Fq2 products accumulated in the 64-bit columns of Fq29 and reduced ONCE (acc2_*): a
// component of an Fq2 product is two limb-product sets, at most six sets share one reduction.  The only subtractions
// are the negated imaginary parts of the second operands (8 p - b1) and the pre-multiplied xi b_j, both computed once
// per product.
//
// Bounds contract (multiples of p per Fq component; rho' = p / rho = 0.0059).  tools/fq12_bounds.py replays every function
// below on upper bounds and re-derives each figure in square brackets.  ELEMENT: every component normalised (limbs
// 0..7 < 2^29 + 8) and at most 4 p.  Every function takes elements and returns elements unless it says otherwise.
//   acc2_*       : six limb-product sets of normalised operands and the nine terms of the quotient digits: a column
//                  stays below [columns] 2^63.98; the reduced value is below (1 + rho' sum A_t B_t) p
//   second operand of an accumulated product: below 8 p (fq12_neg1 negates its imaginary part to 8 p - b1, exactly: see
//                  fq12_neg_exact);
//                  xi b = Fq2::mul(xi, b): [xi_b] 1.24 p
//   fq12_mul     : two reductions of six sets per component, added and normalised: [fq12_mul] 3.71 p
//   fq12_sqr     : symmetric: doubled first operands (8 p) on the cross terms; an even coefficient two reductions of two
//                  products, an odd one one reduction of three: [fq12_sqr] 3.71 p
//   fq6_mul      : one reduction of six sets: [fq6_mul] 1.86 p
//   fq12_mul_line: line coefficients below 8 p, one reduction: [fq12_mul_line] 2.14 p
//   fq12_cyclo_sqr (Granger-Scott, elements of the cyclotomic subgroup): 3 (a^2 + xi b^2) - 2 z as (3 a) a + (3 xi b) b +
//                  z (-2), five sets: [cyclo_even] 2.18 p;  3 (2 a b) + 2 z as (6 a) b + z 2, three sets: [cyclo_odd] 2.75 p
//   fq12_conj    : odd coefficients 4 p - c: at most 4 p (exactly 4 p for a zero component: why second operands take 8 p,
//                  and why 4 p - c is formed with the carry run through, fq12_neg_exact: the conjugate of a conjugate)
//   fq12_frob<K> : Fq2::mul(gamma, conj^K(c)): [fq12_frob] 1.22 p
//   fq12_inv     : c0^2 - v c1^2 + 4 p: [inv_t] 5.86 p (fq6_inv takes components below 8 p); fq6_inv: [fq6_inv] 1.25 p;
//                  the two closing products: [fq12_inv] 2.32 p
//   fq12_pow_x, fq12_final_exp: cyclotomic squarings, products, conjugates and Frobenius maps: elements throughout
//   double_step, add_step: T = (X, Y, Z) homogeneous with components at most 4 p in; out X [step_x] 3.11 p,
//                  Y [step_y] 1.07 p, Z [step_z] 1.83 p.  Q affine, y possibly a negation (at most 4 p); P canonical.
//                  Lines: l0 [line_l0] 1.09 p, l1 [line_l1] 1.19 p, l3 [line_l3] 5.31 p (below the 8 p of a second operand).
//                  Division-free, no exceptional case and no fault: T = Q in an addition step gives T = (0, 0, 0) and zero
//                  lines from there on; T = -Q gives the point at infinity (0, Y', 0) and the vertical line (0, l1, l3).
//   fq12_from_record / fq12_to_record: any 256-bit words in (Fq29::from_ext: < 1.04 p); canonical out
// A Miller value is a representative: it is defined up to factors of proper subfields, which the final exponentiation
// removes.  Only fq12_final_exp's result is a unique GT element.
#pragma once
#include "bn254_fq2_29.hip.h"

#if defined(__HIPCC__)
#define MSM_HD_OUTLINE __host__ __device__ inline __noinline__
#else
#define MSM_HD_OUTLINE inline __attribute__((noinline))
#endif

namespace msm_amd {

struct fq6 {
  fq2 c[3];   // of v^0, v^1, v^2
};
struct fq12 {
  fq2 c[6];   // of w^0 .. w^5
};
struct g2proj {   // homogeneous projective point of the twist
  fq2 x, y, z;
};
struct g1eval {   // the G1 point a line is evaluated at, canonical
  fe29 x, y;
};
struct g2aff {    // affine twist point; y may be a negation (<= 4 p)
  fq2 x, y;
};
struct line_coeffs {   // l0 + l1 w + l3 w^3
  fq2 l0, l1, l3;
};

enum : int { kGtMontLe = 0, kGtCanonLe = 1 };
constexpr uint32_t kGtBytes = 384, kFq12Words = 108;
constexpr uint64_t kBnX = 4965661367192848881ull;
// signed digits 63 .. 0 of 6x + 2 under its leading one (tools/gen_fq12_constants.py)
constexpr uint64_t kAtePos = 0xA1818041C0864428ull, kAteNeg = 0x0408100802100880ull;

struct Fq12K {
  enum : int { XI = 0, B3 = 2, GAMMA = 4, RADIX = 34, ROWS = 35 };
  MSM_HD static fe29 row(int r) {
    constexpr uint32_t c[ROWS][9] = {
#include "bn254_fq12_29_consts.inc"
    };
    fe29 f;
    MSM_UNROLL for (int i = 0; i < 9; ++i) f.l[i] = c[r][i];
    return f;
  }
  MSM_HD static fq2 pair(int r) { return fq2{row(r), row(r + 1)}; }
  MSM_HD static fq2 xi() { return pair(XI); }
  MSM_HD static fq2 b3() { return pair(B3); }
  // xi^(i (p^k - 1) / 6), k = 1 .. 3, i = 1 .. 5
  MSM_HD static fq2 gamma(int k, int i) { return pair(GAMMA + 2 * (5 * (k - 1) + (i - 1))); }
};

// ---- accumulated Fq2 products -------------------------------------------------------------------------------------------
struct Acc2 {
  uint64_t re[17], im[17];
};
MSM_HD void acc2_zero(Acc2& A) {
  MSM_UNROLL for (int k = 0; k < 17; ++k) A.re[k] = A.im[k] = 0;
}
MSM_HD void acc_fe(uint64_t (&A)[17], const fe29& a, const fe29& b) {
  MSM_UNROLL for (int k = 0; k < 17; ++k) {
    uint64_t s = A[k];
    MSM_UNROLL for (int i = 0; i < 9; ++i) {
      const int j = k - i;
      if (j >= 0 && j < 9) s += (uint64_t)a.l[i] * b.l[j];
    }
    A[k] = s;
  }
}
// A += a b, nb1 = K p - b.c1: two sets per component
MSM_HD void acc2_mul(Acc2& A, const fq2& a, const fq2& b, const fe29& nb1) {
  acc_fe(A.re, a.c0, b.c0);
  acc_fe(A.re, a.c1, nb1);
  acc_fe(A.im, a.c0, b.c1);
  acc_fe(A.im, a.c1, b.c0);
}
// A += a s, s in Fq: one set per component
MSM_HD void acc2_scale(Acc2& A, const fq2& a, const fe29& s) {
  acc_fe(A.re, a.c0, s);
  acc_fe(A.im, a.c1, s);
}
MSM_HD fq2 acc2_reduce(Acc2& A) { return fq2{Fq29::reduce_columns(A.re), Fq29::reduce_columns(A.im)}; }

// K p - b for EVERY normalised b <= K p, plain limbs out.  Fq2::sub1<K>(0, b) runs one parallel carry round over a K p
// whose limbs 0..7 are lifted by 2^30 and whose top limb is two short for it: when K p - b is below 2^233 (b = 4 p, the
// conjugate of a zero component; a line coefficient of 8 p - 1) nothing carries into the top limb and it wraps.  Here
// the carry runs through all nine limbs, so the contract's "at most 4 p" and "below 8 p" hold up to the last value.
template <int SEL>
MSM_HD fe29 fq12_neg_exact(const fe29& b) {
  fe29 r;
  uint32_t c = 0;
  MSM_UNROLL for (int i = 0; i < 8; ++i) {
    const uint32_t t = Fq29::kc(SEL, i) - b.l[i] + c;   // kc >= 2^30 > b.l[i]: no wrap
    r.l[i] = t & Fq29::MASK;
    c = t >> 29;
  }
  r.l[8] = Fq29::kc(SEL, 8) - b.l[8] + c;
  return r;
}
MSM_HD fe29 fq12_neg1(const fe29& b) { return fq12_neg_exact<K8E30>(b); }   // 8 p - b, b < 8 p
MSM_HD fe29 fq12_neg4(const fe29& b) { return fq12_neg_exact<K4E30>(b); }   // 4 p - b, b <= 4 p
MSM_HD fq2 fq2_neg8(const fq2& a) { return fq2{fq12_neg1(a.c0), fq12_neg1(a.c1)}; }
MSM_HD fq2 fq2_conj(const fq2& a) { return fq2{a.c0, fq12_neg4(a.c1)}; }   // a.c1 <= 4 p
MSM_HD fq2 fq2_mul_xi(const fq2& a) { return Fq2::mul(Fq12K::xi(), a); }
MSM_HD fq2 fq2_scale(const fq2& a, const fe29& s) { return fq2{Fq29::mul(a.c0, s), Fq29::mul(a.c1, s)}; }
MSM_HD fq2 fq2_add_n(const fq2& a, const fq2& b) { return Fq2::norm(Fq2::add(a, b)); }
// k a for k <= 7 (limbs stay below 2^32), normalised
MSM_HD fq2 fq2_times(const fq2& a, uint32_t k) {
  fq2 r;
  MSM_UNROLL for (int i = 0; i < 9; ++i) {
    r.c0.l[i] = a.c0.l[i] * k;
    r.c1.l[i] = a.c1.l[i] * k;
  }
  return Fq2::norm(r);
}

MSM_HD void fq12_set_one(fq12& a) {
  a.c[0] = Fq2::one();
  for (int i = 1; i < 6; ++i) a.c[i] = Fq2::zero();
}
// element-wise sum / difference (a - b + 4 p, b < 4 p): normalised, NOT elements (up to 8 p): squash before a product
MSM_HD void fq12_add(fq12& out, const fq12& a, const fq12& b) {
  for (int i = 0; i < 6; ++i) out.c[i] = fq2_add_n(a.c[i], b.c[i]);
}
MSM_HD void fq12_sub(fq12& out, const fq12& a, const fq12& b) {
  for (int i = 0; i < 6; ++i) out.c[i] = Fq2::sub<4>(a.c[i], b.c[i]);
}
MSM_HD void fq6_add(fq6& out, const fq6& a, const fq6& b) {
  for (int i = 0; i < 3; ++i) out.c[i] = fq2_add_n(a.c[i], b.c[i]);
}
MSM_HD void fq6_sub(fq6& out, const fq6& a, const fq6& b) {
  for (int i = 0; i < 3; ++i) out.c[i] = Fq2::sub<4>(a.c[i], b.c[i]);
}

// ---- products -------------------------------------------------------------------------------------------------------------
// the second operand of a product, prepared once: b_j, xi b_j and the negated imaginary parts of both
template <int N>
struct MulPrep {
  fq2 b[N], xb[N];
  fe29 nb[N], nxb[N];
};
template <int N>
MSM_HD void mul_prep(MulPrep<N>& p, const fq2* b) {
  MSM_NO_UNROLL for (int j = 0; j < N; ++j) {
    p.b[j] = b[j];
    p.nb[j] = fq12_neg1(b[j].c1);
    p.xb[j] = fq2_mul_xi(b[j]);
    p.nxb[j] = fq12_neg1(p.xb[j].c1);
  }
}

// out = a b in Fq2[t] / (t^N - xi) (N = 6: Fq12 over w; N = 3: Fq6 over v); three Fq2 products per reduction
template <int N>
MSM_HD void poly_mul(fq2* out, const fq2* a, const fq2* b) {
  MulPrep<N> p;
  mul_prep<N>(p, b);
  fq2 r[N];
  MSM_NO_UNROLL for (int k = 0; k < N; ++k) {
    fq2 part[N / 3];
    MSM_NO_UNROLL for (int h = 0; h < N / 3; ++h) {
      Acc2 A;
      acc2_zero(A);
      MSM_NO_UNROLL for (int t = 0; t < 3; ++t) {
        const int i = 3 * h + t;
        int j = k - i;
        const bool wrap = j < 0;
        if (wrap) j += N;
        acc2_mul(A, a[i], wrap ? p.xb[j] : p.b[j], wrap ? p.nxb[j] : p.nb[j]);
      }
      part[h] = acc2_reduce(A);
    }
    r[k] = N == 6 ? fq2_add_n(part[0], part[N / 3 - 1]) : part[0];
  }
  MSM_NO_UNROLL for (int k = 0; k < N; ++k) out[k] = r[k];
}

MSM_HD_OUTLINE void fq12_mul(fq12& out, const fq12& a, const fq12& b) { poly_mul<6>(out.c, a.c, b.c); }
MSM_HD_OUTLINE void fq6_mul(fq6& out, const fq6& a, const fq6& b) { poly_mul<3>(out.c, a.c, b.c); }

// Where the running f of a Miller loop lives: the squaring and the line multiplication reach its coefficients through
// get / set only.  Fq12Private: an fq12 in the lane's private memory.  Fq12Strided: word w of the 108-word value at
// base[w * stride] -- with base = array + lane and stride = 64 the word-major [word][lane] form in LDS, where the 64 lanes
// of a wave read 64 consecutive words (one per bank).  Coefficient i of w^i holds words 18 i .. 18 i + 17.
struct Fq12Private {
  fq12* p;
  MSM_HD fq2 get(int i) const { return p->c[i]; }
  MSM_HD void set(int i, const fq2& v) const { p->c[i] = v; }
};
struct Fq12Strided {
  uint32_t* base;
  uint32_t stride;
  MSM_HD fq2 get(int i) const {
    fq2 v;
    MSM_UNROLL for (int w = 0; w < 9; ++w) {
      v.c0.l[w] = base[(size_t)(18 * i + w) * stride];
      v.c1.l[w] = base[(size_t)(18 * i + 9 + w) * stride];
    }
    return v;
  }
  MSM_HD void set(int i, const fq2& v) const {
    MSM_UNROLL for (int w = 0; w < 9; ++w) {
      base[(size_t)(18 * i + w) * stride] = v.c0.l[w];
      base[(size_t)(18 * i + 9 + w) * stride] = v.c1.l[w];
    }
  }
};
template <class F>
MSM_HD void fq12_set_one_t(const F& f) {
  f.set(0, Fq2::one());
  for (int i = 1; i < 6; ++i) f.set(i, Fq2::zero());
}

// f <- f^2, the symmetric form: coefficient k sums a_i a_j over i <= j with i + j = k or k + 6 (the latter through
// xi a_j), the cross terms with the first operand doubled.  An odd k has three doubled products (one reduction), an even k
// two doubled products and two squares (two reductions of two products, added): 21 Fq2 products and 18 reductions where
// the product takes 36 and 24.
template <class F>
MSM_HD_OUTLINE void fq12_sqr_t(const F& f) {
  MulPrep<6> p;
  fq2 a[6];
  MSM_NO_UNROLL for (int i = 0; i < 6; ++i) a[i] = f.get(i);
  mul_prep<6>(p, a);
  fq2 r[6];
  MSM_NO_UNROLL for (int k = 0; k < 6; ++k) {
    const int per = (k & 1) ? 3 : 2;   // products per reduction
    Acc2 A;
    acc2_zero(A);
    fq2 sum = Fq2::zero();
    int have = 0;
    MSM_NO_UNROLL for (int i = 0; i < 6; ++i) {
      int j = k - i;
      const bool wrap = j < 0;
      if (wrap) j += 6;
      if (i > j) continue;
      acc2_mul(A, i == j ? a[i] : fq2_times(a[i], 2), wrap ? p.xb[j] : p.b[j], wrap ? p.nxb[j] : p.nb[j]);
      if (++have == per) {
        sum = fq2_add_n(sum, acc2_reduce(A));
        acc2_zero(A);
        have = 0;
      }
    }
    r[k] = sum;
  }
  MSM_NO_UNROLL for (int k = 0; k < 6; ++k) f.set(k, r[k]);
}
MSM_HD void fq12_sqr(fq12& out, const fq12& a) {
  out = a;
  fq12_sqr_t(Fq12Private{&out});
}

// f <- f (l0 + l1 w + l3 w^3): three Fq2 products per coefficient, one reduction
template <class F>
MSM_HD_OUTLINE void fq12_mul_line_t(const F& f, const line_coeffs& l) {
  fq2 m[3] = {l.l0, l.l1, l.l3}, xm[3];
  fe29 nm[3], nxm[3];
  MSM_NO_UNROLL for (int t = 0; t < 3; ++t) {
    nm[t] = fq12_neg1(m[t].c1);
    xm[t] = fq2_mul_xi(m[t]);
    nxm[t] = fq12_neg1(xm[t].c1);
  }
  fq2 r[6];
  MSM_NO_UNROLL for (int k = 0; k < 6; ++k) {
    Acc2 A;
    acc2_zero(A);
    MSM_NO_UNROLL for (int t = 0; t < 3; ++t) {
      const int d = t == 2 ? 3 : t;   // the power of w of m[t]
      int i = k - d;
      const bool wrap = i < 0;
      if (wrap) i += 6;
      acc2_mul(A, f.get(i), wrap ? xm[t] : m[t], wrap ? nxm[t] : nm[t]);
    }
    r[k] = acc2_reduce(A);
  }
  MSM_NO_UNROLL for (int k = 0; k < 6; ++k) f.set(k, r[k]);
}
MSM_HD void fq12_mul_line(fq12& f, const line_coeffs& l) { fq12_mul_line_t(Fq12Private{&f}, l); }

// a^(p^6): w -> -w
MSM_HD void fq12_conj(fq12& out, const fq12& a) {
  MSM_NO_UNROLL for (int i = 0; i < 6; ++i) out.c[i] = (i & 1) ? fq2{fq12_neg4(a.c[i].c0), fq12_neg4(a.c[i].c1)} : a.c[i];
}

// a^(p^K), K = 1, 2, 3: coefficient i becomes conj^K(a_i) gamma[K][i]
template <int K>
MSM_HD_OUTLINE void fq12_frob(fq12& out, const fq12& a) {
  out.c[0] = (K & 1) ? fq2_conj(a.c[0]) : a.c[0];
  MSM_NO_UNROLL for (int i = 1; i < 6; ++i) out.c[i] = Fq2::mul(Fq12K::gamma(K, i), (K & 1) ? fq2_conj(a.c[i]) : a.c[i]);
}

// Granger-Scott squaring of an element of the cyclotomic subgroup.  With the tower names z0 = c0.c0, z4 = c0.c1,
// z3 = c0.c2, z2 = c1.c0, z1 = c1.c1, z5 = c1.c2 and (t, t') = (a^2 + xi b^2, 2 a b) for the pairs (z0, z1), (z2, z3),
// (z4, z5):  z0' = 3 t01 - 2 z0, z1' = 3 t01' + 2 z1, z2' = 3 xi t45' + 2 z2, z3' = 3 t45 - 2 z3, z4' = 3 t23 - 2 z4,
// z5' = 3 t23' + 2 z5.  The small factors go into the first operands and into the constants 2, -2: one reduction each.
MSM_HD void cyclo_even(fq2& out, const fq2& a, const fq2& b, const fq2& z, const fe29& minus2) {   // 3 (a^2 + xi b^2) - 2 z
  const fq2 xb = fq2_mul_xi(b);
  Acc2 A;
  acc2_zero(A);
  acc2_mul(A, fq2_times(a, 3), a, fq12_neg1(a.c1));
  acc2_mul(A, fq2_times(xb, 3), b, fq12_neg1(b.c1));
  acc2_scale(A, z, minus2);
  out = acc2_reduce(A);
}
MSM_HD void cyclo_odd(fq2& out, const fq2& a, const fq2& b, const fq2& z, const fe29& two) {   // 3 (2 a b) + 2 z
  Acc2 A;
  acc2_zero(A);
  acc2_mul(A, fq2_times(a, 6), b, fq12_neg1(b.c1));
  acc2_scale(A, z, two);
  out = acc2_reduce(A);
}
MSM_HD_OUTLINE void fq12_cyclo_sqr(fq12& out, const fq12& a) {
  const fe29 two = Fq29::norm(Fq29::add(Fq29::one(), Fq29::one()));
  const fe29 minus2 = Fq2::sub1<4>(Fq29::zero(), two);
  const fq2 z0 = a.c[0], z4 = a.c[2], z3 = a.c[4], z2 = a.c[1], z1 = a.c[3], z5 = a.c[5];
  fq12 r;
  cyclo_even(r.c[0], z0, z1, z0, minus2);
  cyclo_odd(r.c[3], z0, z1, z1, two);
  cyclo_odd(r.c[1], fq2_mul_xi(z4), z5, z2, two);
  cyclo_even(r.c[4], z4, z5, z3, minus2);
  cyclo_even(r.c[2], z2, z3, z4, minus2);
  cyclo_odd(r.c[5], z2, z3, z5, two);
  out = r;
}

// a^x, a in the cyclotomic subgroup: 62 squarings, one multiplication per set bit under the leading one
MSM_HD_OUTLINE void fq12_pow_x(fq12& out, const fq12& a) {
  fq12 r = a;
  MSM_NO_UNROLL for (int b = 61; b >= 0; --b) {
    fq12_cyclo_sqr(r, r);
    if ((kBnX >> b) & 1u) fq12_mul(r, r, a);
  }
  out = r;
}

// ---- inversion through one inv_fq ---------------------------------------------------------------------------------------
// (a0 + a1 v + a2 v^2)^-1 = (A + B v + C v^2) / F:  A = a0^2 - xi a1 a2,  B = xi a2^2 - a0 a1,  C = a1^2 - a0 a2,
// F = a0 A + xi (a2 B + a1 C).  Components of a below 8 p, normalised.  Each of A, B, C, F is one reduction: the minus
// signs ride on first operands negated to 8 p - x.
MSM_HD_OUTLINE void fq6_inv(fq6& out, const fq6& a) {
  const fq2 a0 = a.c[0], a1 = a.c[1], a2 = a.c[2];
  const fq2 xa1 = fq2_mul_xi(a1), xa2 = fq2_mul_xi(a2), na0 = fq2_neg8(a0), nxa1 = fq2_neg8(xa1);
  const fe29 n0 = fq12_neg1(a0.c1), n1 = fq12_neg1(a1.c1), n2 = fq12_neg1(a2.c1);
  Acc2 S;
  acc2_zero(S);
  acc2_mul(S, a0, a0, n0);
  acc2_mul(S, nxa1, a2, n2);
  const fq2 A = acc2_reduce(S);
  acc2_zero(S);
  acc2_mul(S, xa2, a2, n2);
  acc2_mul(S, na0, a1, n1);
  const fq2 B = acc2_reduce(S);
  acc2_zero(S);
  acc2_mul(S, a1, a1, n1);
  acc2_mul(S, na0, a2, n2);
  const fq2 C = acc2_reduce(S);
  acc2_zero(S);
  acc2_mul(S, a0, A, fq12_neg1(A.c1));
  acc2_mul(S, xa2, B, fq12_neg1(B.c1));
  acc2_mul(S, xa1, C, fq12_neg1(C.c1));
  const fq2 Fi = Fq2::inv(acc2_reduce(S));
  out.c[0] = Fq2::mul(Fi, A);
  out.c[1] = Fq2::mul(Fi, B);
  out.c[2] = Fq2::mul(Fi, C);
}

// (c0 + c1 w)^-1 = (c0 - c1 w) / (c0^2 - v c1^2), c0 = (a0, a2, a4), c1 = (a1, a3, a5)
MSM_HD_OUTLINE void fq12_inv(fq12& out, const fq12& a) {
  fq6 c0, c1, t0, t1, t;
  for (int k = 0; k < 3; ++k) {
    c0.c[k] = a.c[2 * k];
    c1.c[k] = a.c[2 * k + 1];
  }
  fq6_mul(t0, c0, c0);
  fq6_mul(t1, c1, c1);
  // v (x0, x1, x2) = (xi x2, x0, x1); t = t0 - v t1 + 4 p (the contract's [inv_t])
  t.c[0] = Fq2::sub<4>(t0.c[0], fq2_mul_xi(t1.c[2]));
  t.c[1] = Fq2::sub<4>(t0.c[1], t1.c[0]);
  t.c[2] = Fq2::sub<4>(t0.c[2], t1.c[1]);
  fq6_inv(t0, t);
  fq6_mul(t1, c0, t0);
  for (int k = 0; k < 3; ++k) c1.c[k] = fq2_neg8(c1.c[k]);
  fq6_mul(t, c1, t0);
  for (int k = 0; k < 3; ++k) {
    out.c[2 * k] = t1.c[k];
    out.c[2 * k + 1] = t.c[k];
  }
}

// ---- the final exponentiation (p^12 - 1) / r = (p^6 - 1)(p^2 + 1) (p^4 - p^2 + 1) / r --------------------------------------
// Hard part by the base-p digits of (p^4 - p^2 + 1) / r (Devegili, Scott, Dahab): p^3 + (6x^2 + 1) p^2 + (-36x^3 - 18x^2
// - 12x + 1) p + (-36x^3 - 30x^2 - 18x - 2), gathered as y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36 with three powers by x.
// This is the exact exponent, not a multiple of it.  f = 0 (never a Miller value of valid points) gives 0.
MSM_HD_OUTLINE void fq12_final_exp(fq12& f) {
  fq12 t, u;
  fq12_inv(t, f);
  fq12_conj(u, f);
  fq12_mul(t, u, t);          // f^(p^6 - 1)
  fq12_frob<2>(u, t);
  fq12_mul(f, u, t);          // ... ^(p^2 + 1): in the cyclotomic subgroup, inverse = conjugate
  fq12 fx, fx2, fx3, y0, y;
  fq12_pow_x(fx, f);
  fq12_pow_x(fx2, fx);
  fq12_pow_x(fx3, fx2);
  fq12_frob<1>(y0, f);
  fq12_frob<2>(t, f);
  fq12_mul(y0, y0, t);
  fq12_frob<3>(t, f);
  fq12_mul(y0, y0, t);        // y0 = f^p f^(p^2) f^(p^3)
  fq12 t0, t1;
  fq12_frob<1>(t, fx3);
  fq12_mul(t, t, fx3);
  fq12_conj(y, t);            // y6 = 1 / (fx3 fx3^p)
  fq12_cyclo_sqr(t0, y);
  fq12_frob<1>(t, fx2);
  fq12_mul(t, t, fx);
  fq12_conj(y, t);            // y4 = 1 / (fx fx2^p)
  fq12_mul(t0, t0, y);
  fq12_conj(y, fx2);          // y5 = 1 / fx2
  fq12_mul(t0, t0, y);
  fq12_frob<1>(t, fx);
  fq12_conj(u, t);            // y3 = 1 / fx^p
  fq12_mul(t1, u, y);
  fq12_mul(t1, t1, t0);
  fq12_frob<2>(y, fx2);       // y2 = fx2^(p^2)
  fq12_mul(t0, t0, y);
  fq12_cyclo_sqr(t1, t1);
  fq12_mul(t1, t1, t0);
  fq12_cyclo_sqr(t1, t1);
  fq12_conj(y, f);            // y1 = 1 / f
  fq12_mul(t0, t1, y);
  fq12_mul(t1, t1, y0);
  fq12_cyclo_sqr(t0, t0);
  fq12_mul(f, t0, t1);
}

// ---- the steps of the Miller loop ---------------------------------------------------------------------------------------
// T <- 2 T and the tangent at T evaluated at P.  With b = Y^2, c = Z^2, e = 3 b' c, f = 3 e, h = 2 Y Z, j = X^2:
//   X' = 2 X Y (b - f),  Y' = (b + f)^2 - 3 (2 e)^2,  Z' = 4 b h;  line (-h y_P, 3 j x_P, e - b)
MSM_HD_OUTLINE void double_step(g2proj& T, line_coeffs& l, const g1eval& P) {
  const fq2 b = Fq2::sqr(T.y), c = Fq2::sqr(T.z);
  const fq2 e = Fq2::mul(Fq12K::b3(), c);
  const fq2 f = fq2_times(e, 3);
  const fq2 yz = Fq2::mul(T.y, T.z);
  const fq2 h = fq2_add_n(yz, yz);
  const fq2 j = Fq2::sqr(T.x);
  const fq2 xy = Fq2::mul(T.x, T.y);
  const fq2 e2 = Fq2::sqr(fq2_add_n(e, e));
  const fq2 s = Fq2::sqr(fq2_add_n(b, f));
  l.l0 = fq2_scale(h, Fq2::sub1<4>(Fq29::zero(), P.y));
  l.l1 = fq2_scale(fq2_times(j, 3), P.x);
  l.l3 = Fq2::sub<4>(e, b);
  T.x = Fq2::mul(fq2_add_n(xy, xy), Fq2::sub<8>(b, f));
  T.y = Fq2::squash(Fq2::sub<8>(s, fq2_times(e2, 3)));
  T.z = Fq2::mul(fq2_add_n(b, b), fq2_add_n(h, h));
}

// T <- T + Q and the line through them at P.  theta = Y - y_Q Z, lam = X - x_Q Z, c = theta^2, d = lam^2, e = lam d,
// f = Z c, g = X d, h = e + f - 2 g:  X' = lam h,  Y' = theta (g - h) - e Y,  Z' = Z e;
// line (lam y_P, -theta x_P, theta x_Q - lam y_Q)
MSM_HD_OUTLINE void add_step(g2proj& T, line_coeffs& l, const g2aff& Q, const g1eval& P) {
  const fq2 theta = Fq2::sub<4>(T.y, Fq2::mul(T.z, Q.y));
  const fq2 lam = Fq2::sub<4>(T.x, Fq2::mul(T.z, Q.x));
  const fq2 c = Fq2::sqr(theta), d = Fq2::sqr(lam);
  const fq2 e = Fq2::mul(lam, d);
  const fq2 f = Fq2::mul(T.z, c);
  const fq2 g = Fq2::mul(T.x, d);
  const fq2 h = Fq2::sub<8>(fq2_add_n(e, f), fq2_add_n(g, g));
  l.l0 = fq2_scale(lam, P.y);
  l.l1 = fq2_scale(theta, Fq2::sub1<4>(Fq29::zero(), P.x));
  l.l3 = Fq2::sub<4>(Fq2::mul(Q.x, theta), Fq2::mul(Q.y, lam));
  const fq2 t1 = Fq2::mul(theta, Fq2::sub<16>(g, h));
  T.x = Fq2::mul(lam, h);
  T.y = Fq2::squash(Fq2::sub<4>(t1, Fq2::mul(e, T.y)));
  T.z = Fq2::mul(T.z, e);
}

// pi(Q) and -pi^2(Q): the p-power Frobenius on the twist
MSM_HD void g2_frob_points(const g2aff& Q, g2aff& q1, g2aff& q2) {
  q1.x = Fq2::mul(Fq12K::gamma(1, 2), fq2_conj(Q.x));
  q1.y = Fq2::mul(Fq12K::gamma(1, 3), fq2_conj(Q.y));
  q2.x = Fq2::mul(Fq12K::gamma(2, 2), Q.x);
  q2.y = Fq2::sub<4>(Fq2::zero(), Fq2::mul(Fq12K::gamma(2, 3), Q.y));
}

// ---- records ----------------------------------------------------------------------------------------------------------------
MSM_HD fe29 fq12_fe_from(const u256& x, int layout) {
  return layout == kGtMontLe ? Fq29::from_ext(x) : Fq29::mul(Fq29::unpack256(x), Fq12K::row(Fq12K::RADIX));
}
MSM_HD u256 fq12_fe_to(const fe29& a, int layout) {
  if (layout == kGtMontLe) return Fq29::to_ext(a);
  fe29 one_plain = Fq29::zero();
  one_plain.l[0] = 1;
  return Fq29::pack256(Fq29::canonical(Fq29::mul(a, one_plain), 1));
}
// the record slot r = 3 h + k holds c[2 k + h]
MSM_HD int fq12_slot_to_w(int r) { return 2 * (r % 3) + r / 3; }

MSM_HD void fq12_from_record(fq12& a, const uint32_t* rec, int layout) {
  MSM_NO_UNROLL for (int r = 0; r < 6; ++r) {
    u256 x0, x1;
    for (int i = 0; i < 8; ++i) {
      x0.v[i] = rec[16 * r + i];
      x1.v[i] = rec[16 * r + 8 + i];
    }
    a.c[fq12_slot_to_w(r)] = fq2{fq12_fe_from(x0, layout), fq12_fe_from(x1, layout)};
  }
}
MSM_HD void fq12_to_record(uint32_t* rec, const fq12& a, int layout) {
  MSM_NO_UNROLL for (int r = 0; r < 6; ++r) {
    const fq2 c = a.c[fq12_slot_to_w(r)];
    const u256 x0 = fq12_fe_to(c.c0, layout), x1 = fq12_fe_to(c.c1, layout);
    for (int i = 0; i < 8; ++i) {
      rec[16 * r + i] = x0.v[i];
      rec[16 * r + 8 + i] = x1.v[i];
    }
  }
}
MSM_HD bool fq12_is_one(const fq12& a) {
  bool ok = Fq29::is_zero_exact(Fq2::sub1<4>(a.c[0].c0, Fq29::one())) && Fq29::is_zero_exact(a.c[0].c1);
  MSM_NO_UNROLL for (int i = 1; i < 6; ++i) ok = ok && Fq2::is_zero_exact(a.c[i]);
  return ok;
}

// raw 108-word records (tower order, limbs as they are)
MSM_HD void fq12_from_raw(fq12& a, const uint32_t* w) {
  MSM_NO_UNROLL for (int r = 0; r < 6; ++r) {
    fq2 c;
    for (int i = 0; i < 9; ++i) {
      c.c0.l[i] = w[18 * r + i];
      c.c1.l[i] = w[18 * r + 9 + i];
    }
    a.c[fq12_slot_to_w(r)] = c;
  }
}
template <class F>
MSM_HD void fq12_to_raw_t(uint32_t* w, const F& f) {
  MSM_NO_UNROLL for (int r = 0; r < 6; ++r) {
    const fq2 c = f.get(fq12_slot_to_w(r));
    for (int i = 0; i < 9; ++i) {
      w[18 * r + i] = c.c0.l[i];
      w[18 * r + 9 + i] = c.c1.l[i];
    }
  }
}
MSM_HD void fq12_to_raw(uint32_t* w, const fq12& a) {
  MSM_NO_UNROLL for (int r = 0; r < 6; ++r) {
    const fq2 c = a.c[fq12_slot_to_w(r)];
    for (int i = 0; i < 9; ++i) {
      w[18 * r + i] = c.c0.l[i];
      w[18 * r + 9 + i] = c.c1.l[i];
    }
  }
}

// ---- raw-limb test ops (msm_amd_test_fq12_op, msm_amd_test_fq12_op_host) -------------------------------------------------
// a, b, out: 108 words each.  An fq12 / fq6 sits in the tower order (fq6: the first 54 words).  LINE_MUL: b = l0, l1,
// l3 (54 words).  DOUBLE_STEP: a = T (X, Y, Z: 54 words), b = x_P, y_P (18 words); out = T' (54 words), then l0, l1, l3.
// ADD_STEP: the same with Q (x, y: 36 words) behind T in a.  FINAL_EXP: fq12_final_exp on the raw element a.
enum {
  FQ12OP_FQ6_MUL = 0, FQ12OP_MUL, FQ12OP_SQR, FQ12OP_CYCLO_SQR, FQ12OP_LINE_MUL, FQ12OP_FROB1, FQ12OP_FROB2, FQ12OP_FROB3,
  FQ12OP_CONJ, FQ12OP_INV, FQ12OP_POW_X, FQ12OP_DOUBLE_STEP, FQ12OP_ADD_STEP, FQ12OP_FINAL_EXP, FQ12OP_COUNT
};
MSM_HD fq2 fq12raw_fq2(const uint32_t* w) {
  fq2 r;
  for (int i = 0; i < 9; ++i) {
    r.c0.l[i] = w[i];
    r.c1.l[i] = w[9 + i];
  }
  return r;
}
MSM_HD void fq12raw_put_fq2(uint32_t* w, const fq2& a) {
  for (int i = 0; i < 9; ++i) {
    w[i] = a.c0.l[i];
    w[9 + i] = a.c1.l[i];
  }
}
MSM_HD void run_test_fq12_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  for (uint32_t i = 0; i < kFq12Words; ++i) out[i] = 0;
  fq12 x, y, r;
  if (op == FQ12OP_FQ6_MUL) {
    fq6 u, v, s;
    for (int k = 0; k < 3; ++k) {
      u.c[k] = fq12raw_fq2(a + 18 * k);
      v.c[k] = fq12raw_fq2(b + 18 * k);
    }
    fq6_mul(s, u, v);
    for (int k = 0; k < 3; ++k) fq12raw_put_fq2(out + 18 * k, s.c[k]);
    return;
  }
  if (op == FQ12OP_DOUBLE_STEP || op == FQ12OP_ADD_STEP) {
    g2proj T{fq12raw_fq2(a), fq12raw_fq2(a + 18), fq12raw_fq2(a + 36)};
    g1eval P;
    for (int i = 0; i < 9; ++i) {
      P.x.l[i] = b[i];
      P.y.l[i] = b[9 + i];
    }
    line_coeffs l;
    if (op == FQ12OP_DOUBLE_STEP) {
      double_step(T, l, P);
    } else {
      const g2aff Q{fq12raw_fq2(a + 54), fq12raw_fq2(a + 72)};
      add_step(T, l, Q, P);
    }
    fq12raw_put_fq2(out, T.x);
    fq12raw_put_fq2(out + 18, T.y);
    fq12raw_put_fq2(out + 36, T.z);
    fq12raw_put_fq2(out + 54, l.l0);
    fq12raw_put_fq2(out + 72, l.l1);
    fq12raw_put_fq2(out + 90, l.l3);
    return;
  }
  fq12_from_raw(x, a);
  switch (op) {
    case FQ12OP_MUL:
      fq12_from_raw(y, b);
      fq12_mul(r, x, y);
      break;
    case FQ12OP_SQR: fq12_sqr(r, x); break;
    case FQ12OP_CYCLO_SQR: fq12_cyclo_sqr(r, x); break;
    case FQ12OP_LINE_MUL: {
      const line_coeffs l{fq12raw_fq2(b), fq12raw_fq2(b + 18), fq12raw_fq2(b + 36)};
      r = x;
      fq12_mul_line(r, l);
      break;
    }
    case FQ12OP_FROB1: fq12_frob<1>(r, x); break;
    case FQ12OP_FROB2: fq12_frob<2>(r, x); break;
    case FQ12OP_FROB3: fq12_frob<3>(r, x); break;
    case FQ12OP_CONJ: fq12_conj(r, x); break;
    case FQ12OP_INV: fq12_inv(r, x); break;
    case FQ12OP_POW_X: fq12_pow_x(r, x); break;
    case FQ12OP_FINAL_EXP:
      r = x;
      fq12_final_exp(r);
      break;
    default: return;
  }
  fq12_to_raw(out, r);
}

}  // namespace msm_amd
