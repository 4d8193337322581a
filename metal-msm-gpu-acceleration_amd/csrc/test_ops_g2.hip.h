// Raw-limb test ops of the G2 arithmetic (msm_amd_test_op_g2 on the device, msm_amd_test_op_g2_host on the host):
// limbs go in and come out unchanged, so the tests can put operands anywhere inside the bounds contract of
// bn254_fq2_29.hip.h / bn254_ec2_29.hip.h and compare device and host bit for bit.
// Records (u32 words): an operand is MSM_AMD_G2_RAW_IN_WORDS = 72 words, a result MSM_AMD_G2_RAW_OUT_WORDS = 80.
//   fq2    18 words: c0 limbs 0..8, c1 limbs 0..8
//   affine 36 words: x (fq2), y (fq2)
//   PtI2   72 words: X, Y, ZZ, ZZZ (fq2 each)
//   result: the fq2 or PtI2 in words 0.., word 72 = 1 if the addition reported a vanished sum
#pragma once
#include "bn254_ec2_29.hip.h"

namespace msm_amd {

enum {
  G2RAW_FQ2_MUL = 0,     // a, b fq2
  G2RAW_FQ2_SQR = 1,     // a fq2
  G2RAW_PT_MADD = 2,     // a PtI2 (not identity), b affine (not identity)
  G2RAW_PT_MMADD = 3,    // a, b affine (neither the identity)
  G2RAW_PT_ADD_NZ = 4,   // a, b PtI2 (neither the identity)
  G2RAW_PT_ADD = 5,      // a, b PtI2
  G2RAW_PT_DOUBLE = 6,   // a PtI2 (not identity)
  G2RAW_FQ2_INV = 7,     // a fq2 (non-zero, < 32 p)
  G2RAW_PT_TO_AFFINE = 8,   // a PtI2 (not identity) -> canonical affine x, y in words 0..35
  G2RAW_OPS = 9
};
constexpr int kG2RawIn = 72, kG2RawOut = 80;

MSM_HD fq2 g2raw_fq2(const uint32_t* w) {
  fq2 r;
  for (int i = 0; i < 9; ++i) {
    r.c0.l[i] = w[i];
    r.c1.l[i] = w[9 + i];
  }
  return r;
}
MSM_HD void g2raw_put_fq2(uint32_t* w, const fq2& a) {
  for (int i = 0; i < 9; ++i) {
    w[i] = a.c0.l[i];
    w[9 + i] = a.c1.l[i];
  }
}
MSM_HD PtI2 g2raw_pt(const uint32_t* w) {
  PtI2 r;
  r.x = g2raw_fq2(w);
  r.y = g2raw_fq2(w + 18);
  r.zz = g2raw_fq2(w + 36);
  r.zzz = g2raw_fq2(w + 54);
  return r;
}
MSM_HD void g2raw_put_pt(uint32_t* w, const PtI2& p) {
  g2raw_put_fq2(w, p.x);
  g2raw_put_fq2(w + 18, p.y);
  g2raw_put_fq2(w + 36, p.zz);
  g2raw_put_fq2(w + 54, p.zzz);
}

// one element: a, b point at kG2RawIn words each, out at kG2RawOut words
MSM_HD void run_test_op_g2(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  for (int i = 0; i < kG2RawOut; ++i) out[i] = 0;
  bool vanished = false;
  switch (op) {
    case G2RAW_FQ2_MUL: g2raw_put_fq2(out, Fq2::mul(g2raw_fq2(a), g2raw_fq2(b))); break;
    case G2RAW_FQ2_SQR: g2raw_put_fq2(out, Fq2::sqr(g2raw_fq2(a))); break;
    case G2RAW_PT_MADD: {
      Aff2I q;
      q.x = g2raw_fq2(b);
      q.y = g2raw_fq2(b + 18);
      g2raw_put_pt(out, pt2_madd(g2raw_pt(a), q, vanished));
      break;
    }
    case G2RAW_PT_MMADD: {
      Aff2I p, q;
      p.x = g2raw_fq2(a);
      p.y = g2raw_fq2(a + 18);
      q.x = g2raw_fq2(b);
      q.y = g2raw_fq2(b + 18);
      g2raw_put_pt(out, pt2_mmadd(p, q, vanished));
      break;
    }
    case G2RAW_PT_ADD_NZ: g2raw_put_pt(out, pt2_add_nz(g2raw_pt(a), g2raw_pt(b), vanished)); break;
    case G2RAW_PT_ADD: g2raw_put_pt(out, pt2_add(g2raw_pt(a), g2raw_pt(b))); break;
    case G2RAW_PT_DOUBLE: g2raw_put_pt(out, pt2_double(g2raw_pt(a))); break;
    case G2RAW_FQ2_INV: g2raw_put_fq2(out, Fq2::inv(g2raw_fq2(a))); break;
    case G2RAW_PT_TO_AFFINE: {
      const Aff2I r = pt2_to_affine(g2raw_pt(a));   // the canonical limbs aff2_pack stores
      g2raw_put_fq2(out, fq2{Fq29::canonical(r.x.c0, 1), Fq29::canonical(r.x.c1, 1)});
      g2raw_put_fq2(out + 18, fq2{Fq29::canonical(r.y.c0, 1), Fq29::canonical(r.y.c1, 1)});
      break;
    }
    default: break;
  }
  out[72] = vanished ? 1u : 0u;
}

}  // namespace msm_amd
