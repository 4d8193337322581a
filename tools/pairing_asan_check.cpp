// Stand-alone AddressSanitizer / UBSan check of the host side of the pairing calls: the two host twins, the planner tap and
// the host form of the raw Fq12 ops, linked straight from host_pairing.hip (tools/pairing_asan.sh builds and runs it; no
// GPU, no python).  Every buffer is a heap allocation of exactly the size the call may touch, so that a stray access is
// a report.  Points: fixed multiples of the generators, written out below.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/msm_amd.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) std::printf("FAILED: %s\n", what), ++failures;
}

// the EIP-197 generator of G2 as a MSM_AMD_G2_POINT_H2C_AFFINE record: x.c0, x.c1, y.c0, y.c1 in Montgomery form (R = 2^256)
const uint64_t kG2Gen[4][4] = {
    {0x8e83b5d102bc2026ull, 0xdceb1935497b0172ull, 0xfbb8264797811adfull, 0x19573841af96503bull},
    {0xafb4737da84c6140ull, 0x6043dd5a5802d8c4ull, 0x09e950fc52a02f86ull, 0x14fef0833aea7b6bull},
    {0x619dfa9d886be9f6ull, 0xfe7fd297f59e9b78ull, 0xff9e1a62231b7dfeull, 0x28fd7eebae9e4206ull},
    {0x64095b56c71856eeull, 0xdc57f922327d3cbbull, 0x55f935be33351076ull, 0x0da4a0e693fd6482ull}};

// k G1 for k = 3, 10, 17, 24, 31, 38 and 30 as MSM_AMD_POINT_H2C_AFFINE records (x, y in Montgomery form)
const uint64_t kG1Multiples[7][8] = {
    {0x9d831b4e248b11a0ull, 0x91f18c0677f54b7eull, 0x0ee5ea95bfda15d0ull, 0x10f0baf628c70539ull, 0xbe1523ea983653eaull, 0xe86e48177c629a1aull, 0x51cc9f8e6d2a214aull, 0x014925f0ca757913ull},   // 3 G1
    {0xefae235a7a6623a2ull, 0x6580918d8a6b9d2cull, 0x5ce689f5adba40cdull, 0x1d3b4e4758f7915dull, 0xf6964699b73f9538ull, 0xfdf8a694758d5fb6ull, 0xe123030281a4c0eaull, 0x2f34ffe0ea6f891full},   // 10 G1
    {0x6b631a89fd4a8782ull, 0xe9f5a35143bd9100ull, 0x2226cd679544ad66ull, 0x2198c12bdf3e2f8dull, 0xca1bb60571638fa8ull, 0xe3f5d64937933fd9ull, 0x7ab3b03276484cedull, 0x1b8124113fc7eff0ull},   // 17 G1
    {0x7524fe1015cd8451ull, 0x93150d22f877cf5aull, 0xafcb4c31866691fbull, 0x17ea18a6459b3e05ull, 0x2bd2653a29bff925ull, 0xe18fbe4bd17cb5e5ull, 0x3dbefdc85c3c91eaull, 0x27d502f232798646ull},   // 24 G1
    {0xbfa5ecd9e842c0faull, 0x84826d2f49429f19ull, 0xaad76e71c622c348ull, 0x2e2af936d193ef1bull, 0x314c7847e4d494a1ull, 0x3ac20242fe5ff346ull, 0x02289580856a62b4ull, 0x16e3e1a34126204aull},   // 31 G1
    {0xef26ca80bc35bea3ull, 0x4e9be27142a4c4a1ull, 0x30f00c635255994cull, 0x2fd088777a86ddd8ull, 0x10d0fabfd85da2cdull, 0x5be4f8efa05310bdull, 0x40cd639fed0d64d0ull, 0x1c72e6e0ca4b1f1aull},   // 38 G1
    {0xc63d389c9c88fd0aull, 0x4b218c5b6d676debull, 0x5c24066b335de460ull, 0x21f1edaad10face3ull, 0xc3046d1c52c74f2bull, 0x9f367699d709c79bull, 0x0873ca9f6213db85ull, 0x123af082ccf70722ull},   // 30 G1
};

}  // namespace

int main() {
  // G1 side: multiples of (1, 2); G2 side: the generator in every slot
  const size_t n = 6;
  std::vector<uint8_t> g1(n * 64);
  std::memcpy(g1.data(), kG1Multiples, n * 64);
  std::vector<uint8_t> g2one(128, 0);
  std::memcpy(g2one.data(), kG2Gen, 128);
  std::vector<uint8_t> g2(n * 128);
  for (size_t i = 0; i < n; ++i) std::memcpy(&g2[i * 128], g2one.data(), 128);

  for (int gt = MSM_AMD_GT_MONT_LE; gt <= MSM_AMD_GT_CANON_LE; ++gt) {
    for (size_t size : {(size_t)1, (size_t)2, (size_t)3, (size_t)6}) {
      const size_t groups = n / size;
      std::vector<uint8_t> out(groups * MSM_AMD_GT_BYTES), one(groups), mil(groups * MSM_AMD_GT_BYTES), fin(groups * MSM_AMD_GT_BYTES);
      expect(msm_amd_host_pairing_product(MSM_AMD_POINT_H2C_AFFINE, MSM_AMD_G2_POINT_H2C_AFFINE, g1.data(), g2.data(), groups,
                                          size, 0, gt, out.data(), one.data(), 3) == MSM_AMD_OK, "pairing product");
      expect(msm_amd_host_pairing_product(MSM_AMD_POINT_H2C_AFFINE, MSM_AMD_G2_POINT_H2C_AFFINE, g1.data(), g2.data(), groups,
                                          size, MSM_AMD_PAIRING_MILLER_ONLY, gt, mil.data(), nullptr, 2) == MSM_AMD_OK, "Miller products");
      expect(msm_amd_host_final_exponentiation(gt, mil.data(), groups, fin.data(), one.data(), 2) == MSM_AMD_OK, "final exponentiation");
      expect(out == fin, "Miller product + final exponentiation = pairing product");
      for (size_t g = 0; g < groups; ++g) expect(one[g] == 0, "no group is the unit");
    }
  }
  // bilinearity on exactly sized buffers: e(3 G1, Q) e(10 G1, Q) e(17 G1, Q) = e(30 G1, Q), pairs 0 .. 2 against one pair
  {
    std::vector<uint8_t> lhs(MSM_AMD_GT_BYTES), rhs(MSM_AMD_GT_BYTES);
    std::vector<uint8_t> p30(64);
    std::memcpy(p30.data(), kG1Multiples[6], 64);
    expect(msm_amd_host_pairing_product(0, 0, g1.data(), g2.data(), 1, 3, 0, 0, lhs.data(), nullptr, 1) == MSM_AMD_OK, "lhs");
    expect(msm_amd_host_pairing_product(0, 0, p30.data(), g2.data(), 1, 1, 0, 0, rhs.data(), nullptr, 1) == MSM_AMD_OK, "rhs");
    expect(lhs == rhs, "bilinear");
  }
  // group_size 0 reads no point; identities
  {
    std::vector<uint8_t> out(2 * MSM_AMD_GT_BYTES), one(2), zero1(64, 0), zero2(128, 0);
    expect(msm_amd_host_pairing_product(0, 0, nullptr, nullptr, 2, 0, 0, 1, out.data(), one.data(), 1) == MSM_AMD_OK && one[0] == 1 && one[1] == 1,
           "empty groups are the unit");
    expect(msm_amd_host_pairing_product(0, 0, zero1.data(), zero2.data(), 1, 1, 0, 1, out.data(), one.data(), 1) == MSM_AMD_OK && one[0] == 1,
           "identity pair");
    expect(msm_amd_host_pairing_product(0, 0, g1.data(), g2.data(), 1, 1, 2, 0, out.data(), one.data(), 1) == MSM_AMD_INPUT_ERROR, "unknown flag");
  }
  // planner tap and raw ops
  {
    uint32_t plan[4];
    expect(msm_amd_test_pairing_plan(3, 130, 4, 0, plan) == MSM_AMD_OK && plan[0] == 4 && plan[1] == 33 && plan[2] == 3 && plan[3] == 1, "plan");
    std::vector<uint32_t> a(MSM_AMD_FQ12_WORDS, 0), b(MSM_AMD_FQ12_WORDS, 0), out(MSM_AMD_FQ12_WORDS);
    a[0] = 5, b[0] = 7;
    for (int op = 0; op <= MSM_AMD_FQ12_OP_FINAL_EXP; ++op) expect(msm_amd_test_fq12_op_host(op, a.data(), b.data(), out.data()) == MSM_AMD_OK, "raw op");
    expect(msm_amd_test_fq12_op_host(14, a.data(), b.data(), out.data()) == MSM_AMD_INPUT_ERROR, "unknown op");
    // the batched form on exactly sized buffers: three records each way
    std::vector<uint32_t> a3(3 * MSM_AMD_FQ12_WORDS, 0), b3(3 * MSM_AMD_FQ12_WORDS, 0), out3(3 * MSM_AMD_FQ12_WORDS);
    for (int i = 0; i < 3; ++i) a3[i * MSM_AMD_FQ12_WORDS] = 5 + i, b3[i * MSM_AMD_FQ12_WORDS] = 7;
    expect(msm_amd_test_fq12_ops_host(MSM_AMD_FQ12_OP_MUL, a3.data(), b3.data(), out3.data(), 3) == MSM_AMD_OK, "raw ops");
    expect(msm_amd_test_fq12_ops_host(MSM_AMD_FQ12_OP_MUL, nullptr, nullptr, nullptr, 0) == MSM_AMD_OK, "raw ops, count 0");
  }
  std::printf(failures ? "pairing_asan_check: %d failure(s)\n" : "pairing_asan_check: ok\n", failures);
  return failures ? 1 : 0;
}
