// Single-operation test bodies shared by the device test kernel (k_stage.hip) and the host-side test entry
// point msm_amd_test_op_host: the same source runs on a GPU lane and on a CPU core.  Mirrors the reference's
// one-thread test kernels (src/metal/shader/tests/*.h.metal, curves/bn254.h.metal) and adds the ops of the
// 29-bit-limb internal representation used by the hot kernels.
#pragma once
#include "bn254_ec29.hip.h"

namespace msm_amd {

// a, b, out: little-endian u256 arrays; element t uses 1 (integer/field ops) or 3 (points) consecutive u256.
MSM_HD void run_test_op(int op, const u256* a, const u256* b, u256* out, uint32_t t) {
  if (op <= 9 || (op >= 14 && op <= 21) || op >= 32) {
    const u256 x = a[t];
    const u256 y = b[t];
    u256 r = u256_zero();
    switch (op) {
      case 0: u256_add(r, x, y); break;
      case 1: u256_sub(r, x, y); break;
      case 2: r = u256_mul_u32(x, y.v[0]); break;
      case 3: r = u256_shl(x, y.v[0] & 255u); break;
      case 4: r = u256_shr(x, y.v[0] & 255u); break;
      case 5: r = Fq::add(x, y); break;
      case 6: r = Fq::sub(x, y); break;
      case 7: r = Fq::mul(x, y); break;
      case 8: r = Fq::neg(x); break;
      case 9: r = Fq::pow_u32(x, y.v[0]); break;
      default: {
        const fe29 xi = Fq29::from_ext(x);
        const fe29 yi = Fq29::from_ext(y);
        const fe29 y3 = Fq29::add(yi, Fq29::add(yi, yi));
        fe29 ri = Fq29::zero();
        switch (op) {
          case 14: ri = Fq29::mul(xi, yi); break;
          case 15: ri = Fq29::sqr(xi); break;
          case 16: ri = Fq29::norm(Fq29::sub<K4E30>(xi, yi)); break;
          case 17: ri = Fq29::norm(Fq29::sub<K8E30>(xi, yi)); break;
          case 18: ri = Fq29::norm(Fq29::sub<K8E31>(xi, y3)); break;
          case 19: ri = Fq29::norm(Fq29::sub<K16E30>(xi, yi)); break;
          case 20: ri = Fq29::norm(Fq29::sub<K16E31>(xi, y3)); break;
          case 21: ri = Fq29::unpack256(Fq29::pack_canonical(xi)); break;   // incl. the 32-byte storage form
#if defined(MSM_AMD_EXPERIMENTS)
          // build options measured and not shipped (HISTORY.md; -DMSM_AMD_EXPERIMENTS builds only): same values as mul / mul2 / sqr
          case 32: ri = Fq29::mul_karatsuba(xi, yi); break;
          case 33: {   // lockstep product-scanning chains: (x*y, y*y) side by side, their sum checked
            fe29 u, v;
            Fq29::mul_pair(xi, yi, yi, yi, u, v);
            ri = Fq29::norm(Fq29::add(u, v));
            break;
          }
          case 34: {   // (x*y + y*x, x*x) and the squaring pair
            fe29 u, v, w, z;
            Fq29::mul2_mul_pair(xi, yi, yi, xi, xi, xi, u, v);
            Fq29::sqr_pair(xi, yi, w, z);
            ri = Fq29::norm(Fq29::add(Fq29::add(u, v), Fq29::add(w, z)));
            break;
          }
          case 35: {   // three products side by side
            fe29 u, v, w;
            Fq29::mul_triple(xi, yi, xi, xi, yi, yi, u, v, w);
            ri = Fq29::norm(Fq29::add(u, Fq29::add(v, w)));
            break;
          }
          case 36: ri = Fq29::mul2_karatsuba_second(xi, yi, yi, xi); break;   // 2 x y
#endif
        }
        r = Fq29::to_ext(ri);
      }
    }
    out[t] = r;
    return;
  }
  const Jacobian* pa = reinterpret_cast<const Jacobian*>(a);
  const Jacobian* pb = reinterpret_cast<const Jacobian*>(b);
  Jacobian* po = reinterpret_cast<Jacobian*>(out);
  const Jacobian p = pa[t];
  Jacobian r = jac_identity();
  if (op == 10) {
    r = jac_add(p, pb[t]);
  } else if (op == 11) {
    r = jac_scalar_mul(p, b[t]);
  } else if (op == 12) {
    const Jacobian q = pb[t];
    if (jac_is_identity(q)) {
      r = p;
    } else {
      Affine qa;
      qa.x = q.x;
      qa.y = q.y;
      r = jac_madd(p, qa);
    }
  } else if (op == 13) {
    r = jac_double(p);
  } else if (op == 22) {   // internal representation: Jacobian + affine (b given with z = one or z = 0)
    const Jacobian q = pb[t];
    const PtI pi = pti_from_ext(p);
    if (jac_is_identity(q)) {
      r = pti_to_ext(pi);
    } else {
      Affine qa;
      qa.x = q.x;
      qa.y = q.y;
      const AffI qi = affi_from_ext(qa);
      r = pti_to_ext(pti_is_identity(pi) ? pti_from_affi(qi) : pti_madd(pi, qi));
    }
  } else if (op == 23) {   // internal representation: Jacobian + Jacobian
    r = pti_to_ext(pti_add(pti_from_ext(p), pti_from_ext(pb[t])));
  } else if (op == 24) {   // 64 chained mixed additions without leaving the lazy internal form: p + 64 q
    const Jacobian q = pb[t];
    PtI acc = pti_from_ext(p);
    if (!jac_is_identity(q)) {
      Affine qa;
      qa.x = q.x;
      qa.y = q.y;
      const AffI qi = affi_from_ext(qa);
      for (int i = 0; i < 64; ++i) acc = pti_is_identity(acc) ? pti_from_affi(qi) : pti_madd(acc, qi);
    }
    r = pti_to_ext(acc);
  } else if (op == 25) {   // 16 chained full additions: p + 16 q with q Jacobian
    const PtI qi = pti_from_ext(pb[t]);
    PtI acc = pti_from_ext(p);
    for (int i = 0; i < 16; ++i) acc = pti_add(acc, qi);
    r = pti_to_ext(acc);
  } else if (op == 26) {   // the start of every work item: a (affine, z = one) + b (affine) by pti_mmadd, with both
                           // operands lazily negated first (the bound-critical case), then 3 more mixed additions
                           // of -b: the result is -(a + b) - 3 b = -a - 4 b
    const Jacobian q = pb[t];
    if (jac_is_identity(p) || jac_is_identity(q)) {
      r = jac_is_identity(p) ? q : p;   // callers pass finite points; identities are returned unchanged
    } else {
      Affine pa, qa;
      pa.x = p.x;
      pa.y = p.y;
      qa.x = q.x;
      qa.y = q.y;
      AffI pi = affi_from_ext(pa), qi = affi_from_ext(qa);
      pi.y = Fq29::neg(pi.y);         // the accumulator's y: normalised when the point was stored (pti_from_affi)
      qi.y = Fq29::neg_wide(qi.y);    // the incoming base's y: un-normalised negation, as in accumulate_kernel
      PtI acc = pti_mmadd(pi.x, pi.y, qi);
      for (int i = 0; i < 3; ++i) acc = pti_is_identity(acc) ? pti_from_affi(qi) : pti_madd(acc, qi);
      r = pti_to_ext(acc);
    }
  }
  po[t] = r;
}

// ---- raw-limb ops (msm_amd_test_op_raw / _host, MSM_AMD_RAW_*): the internal limbs go in and come out exactly as
// given, so that a test can put operands at the edges of the bounds contract and see result limbs, not only values.
// Record of element t: a, b = kRawInWords u32 from t * kRawInWords, out = kRawOutWords u32 from t * kRawOutWords.
// Ops 0..kRawOpCount-1, kRawWideFirst.. (the wide-digit multiplication forms of the point additions) and kRawFoldFirst..
// (the same with the lifted subtraction folded into the reduction).
constexpr int kRawInWords = 36, kRawOutWords = 40, kRawOpCount = 20, kRawWideFirst = 32, kRawWideCount = 3,
              kRawFoldFirst = 44, kRawFoldCount = 2;

// mul_sub_np<K> / sqr_sub_np<K> (a = nullptr: the squaring of b) with K chosen at run time, for the raw ops
MSM_HD fe29 raw_fold(uint32_t sel, const fe29* a, const fe29& b, const fe29& x) {
  switch (sel) {
#define MSM_RAW_FOLD(K) case K: return a ? Fq29::mul_sub_np<K>(*a, b, x) : Fq29::sqr_sub_np<K>(b, x);
    MSM_RAW_FOLD(K4E30) MSM_RAW_FOLD(K8E30) MSM_RAW_FOLD(K8E31) MSM_RAW_FOLD(K16E30) MSM_RAW_FOLD(K16E31)
    MSM_RAW_FOLD(K12E30)
#undef MSM_RAW_FOLD
  }
  return Fq29::zero();
}

MSM_HD fe29 raw_fe(const uint32_t* w) {
  fe29 r;
  MSM_UNROLL for (int i = 0; i < 9; ++i) r.l[i] = w[i];
  return r;
}
MSM_HD void raw_put_fe(uint32_t* w, const fe29& f) {
  MSM_UNROLL for (int i = 0; i < 9; ++i) w[i] = f.l[i];
}
MSM_HD PtI raw_pt(const uint32_t* w) {
  PtI r;
  r.x = raw_fe(w);
  r.y = raw_fe(w + 9);
  r.zz = raw_fe(w + 18);
  r.zzz = raw_fe(w + 27);
  return r;
}
MSM_HD void raw_put_pt(uint32_t* w, const PtI& p) {
  raw_put_fe(w, p.x);
  raw_put_fe(w + 9, p.y);
  raw_put_fe(w + 18, p.zz);
  raw_put_fe(w + 27, p.zzz);
}

MSM_HD void run_test_op_raw(int op, const uint32_t* a_all, const uint32_t* b_all, uint32_t* out_all, uint32_t t) {
  const uint32_t* a = a_all + (size_t)t * kRawInWords;
  const uint32_t* b = b_all + (size_t)t * kRawInWords;
  uint32_t* out = out_all + (size_t)t * kRawOutWords;
  uint32_t r[kRawOutWords];
  MSM_UNROLL for (int i = 0; i < kRawOutWords; ++i) r[i] = 0;
  const fe29 a0 = raw_fe(a), a1 = raw_fe(a + 9), b0 = raw_fe(b), b1 = raw_fe(b + 9);
  bool vanished = false;
  switch (op) {
    case 0: raw_put_fe(r, Fq29::mul(a0, b0)); break;                // MSM_AMD_RAW_FE_MUL
    case 1: raw_put_fe(r, Fq29::sqr(a0)); break;                    // FE_SQR
    case 2: raw_put_fe(r, Fq29::mul2(a0, a1, b0, b1)); break;       // FE_MUL2: a0 * a1 + b0 * b1
    case 3: raw_put_fe(r, Fq29::sub<K4E30>(a0, b0)); break;         // FE_SUB_K4E30 ... FE_SUB_K16E31: not normalised
    case 4: raw_put_fe(r, Fq29::sub<K8E30>(a0, b0)); break;
    case 5: raw_put_fe(r, Fq29::sub<K8E31>(a0, b0)); break;
    case 6: raw_put_fe(r, Fq29::sub<K16E30>(a0, b0)); break;
    case 7: raw_put_fe(r, Fq29::sub<K16E31>(a0, b0)); break;
    case 8: raw_put_fe(r, Fq29::norm(a0)); break;                   // FE_NORM
    case 9: raw_put_fe(r, Fq29::neg(a0)); break;                    // FE_NEG
    case 10: raw_put_fe(r, Fq29::neg_wide(a0)); break;              // FE_NEG_WIDE
    case 11:                                                        // FE_CANONICAL: rounds = b0.l[0], at most 64
      raw_put_fe(r, Fq29::canonical(a0, (int)(b0.l[0] < 64u ? b0.l[0] : 64u)));
      break;
    case 12: {                                                      // FE_TO_EXT: 8 words little-endian
      const u256 e = Fq29::to_ext(a0);
      MSM_UNROLL for (int i = 0; i < 8; ++i) r[i] = e.v[i];
      break;
    }
    case 13: {                                                      // FE_PACK_UNPACK: limbs, then the packed words
      const u256 w = Fq29::pack256(a0);
      raw_put_fe(r, Fq29::unpack256(w));
      MSM_UNROLL for (int i = 0; i < 8; ++i) r[9 + i] = w.v[i];
      break;
    }
    case 14:                                                        // FE_ZERO: maybe_zero(a0, bound = b0.l[0]), exact
      r[0] = Fq29::maybe_zero(a0, b0.l[0]) ? 1u : 0u;
      r[1] = Fq29::is_zero_exact(a0) ? 1u : 0u;
      break;
    case 15: {   // PT_MADD: PtI a + AffI b (b = x, y: 18 words) through the head / tail pair of accumulate_kernel
      PtI p = raw_pt(a);
      AffI q;
      q.x = b0;
      q.y = b1;
      fe29 U2, S2;
      pti_madd_head(p, q.x, q.y, U2, S2);
      raw_put_pt(r, pti_madd_tail(p, U2, S2, [&]() { return q; }, vanished));
      r[36] = vanished ? 1u : 0u;
      break;
    }
    case 16: {   // PT_MMADD: (a0, a1) + AffI b by the head / tail pair
      AffI q;
      q.x = b0;
      q.y = b1;
      fe29 P, R;
      pti_mmadd_head(a0, a1, q.x, q.y, P, R);
      raw_put_pt(r, pti_mmadd_tail(a0, a1, P, R, [&]() { return q; }, vanished));
      r[36] = vanished ? 1u : 0u;
      break;
    }
    case 17:     // PT_ADD_NZ: PtI a + PtI b, neither the identity
      raw_put_pt(r, pti_add_nz(raw_pt(a), raw_pt(b), vanished));
      r[36] = vanished ? 1u : 0u;
      break;
    case 18: raw_put_pt(r, pti_add(raw_pt(a), raw_pt(b))); break;   // PT_ADD: identities allowed; no vanished flag
    case 19: raw_put_pt(r, pti_double(raw_pt(a))); break;           // PT_DOUBLE
    case 32: raw_put_fe(r, Fq29::mul_np(pin_limbs(a0), pin_limbs(b0))); break;   // FE_MUL_WIDE
    case 33: raw_put_fe(r, Fq29::sqr_np(pin_limbs(a0))); break;                  // FE_SQR_WIDE
    case 34:                                                                      // FE_MUL2_WIDE
      raw_put_fe(r, Fq29::mul2w_np(pin_limbs(a0), pin_limbs(a1), pin_limbs(b0), pin_limbs(b1)));
      break;
    case 40: {   // BASES_IN_PLACE: external records as accumulate_kernel<.., ExtBases> takes them (the image on E')
      // a[0..15], a[16..31], b[1..16]: three external records (x, y: 8 + 8 words); a[32]: bit k = negate record k;
      // b[0]: 0 = unpack record 0, 1 = affine start rec0 + rec1, 2 = (rec0 + rec1) + rec2 by the mixed addition
      Affine e[3];
      MSM_UNROLL for (int i = 0; i < 8; ++i) {
        e[0].x.v[i] = a[i];      e[0].y.v[i] = a[8 + i];
        e[1].x.v[i] = a[16 + i]; e[1].y.v[i] = a[24 + i];
        e[2].x.v[i] = b[1 + i];  e[2].y.v[i] = b[9 + i];
      }
      AffI q[3];
      MSM_UNROLL for (int k = 0; k < 3; ++k) {
        q[k] = affi_from_ext_iso(e[k]);
        if ((a[32] >> k) & 1u) q[k].y = neg_wide_iso(q[k].y);
      }
      if (b[0] == 0) {
        const AffI u = affi_from_ext_iso(e[0]);
        raw_put_fe(r, u.x);
        raw_put_fe(r + 9, u.y);
        r[18] = affine_words_zero(e[0]) ? 1u : 0u;
        raw_put_fe(r + 19, neg_wide_iso(u.y));
        break;
      }
      const PtI one = pti_from_affi(q[0]);
      fe29 P, R;
      pti_mmadd_head<true>(one.x, one.y, q[1].x, q[1].y, P, R);
      PtI acc = pti_mmadd_tail<true>(one.x, one.y, P, R, [&]() { return q[1]; }, vanished);
      if (b[0] == 2 && !vanished) {
        fe29 U2, S2;
        pti_madd_head(acc, q[2].x, q[2].y, U2, S2);
        acc = pti_madd_tail(acc, U2, S2, [&]() { return q[2]; }, vanished);
      }
      raw_put_pt(r, acc);
      r[36] = vanished ? 1u : 0u;
      break;
    }
    case 44: {                                                                    // FE_MUL_SUB: K = b1.l[0]
      const fe29 pa = pin_limbs(a0);
      raw_put_fe(r, raw_fold(b1.l[0], &pa, pin_limbs(a1), b0));
      break;
    }
    case 45: raw_put_fe(r, raw_fold(b1.l[0], nullptr, pin_limbs(a0), b0)); break;   // FE_SQR_SUB
  }
  MSM_UNROLL for (int i = 0; i < kRawOutWords; ++i) out[i] = r[i];
}

#if defined(MSM_AMD_EXPERIMENTS)
constexpr int kTestOpMax = 36;   // 27..31 exist on the host only (msm_host.hip), 32..36: the experimental multiplication forms
#else
constexpr int kTestOpMax = 31;
#endif
MSM_HD bool test_op_is_point(int op) { return (op >= 10 && op <= 13) || (op >= 22 && op <= 26); }

}  // namespace msm_amd
