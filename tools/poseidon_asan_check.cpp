// Stand-alone AddressSanitizer / UBSan check of the host side of the Poseidon calls: the constants generator, the four
// twins and the plan tap, linked straight from host_fr.hip (tools/poseidon_asan.sh builds and runs it; no GPU, no python).
// Every buffer is a heap allocation of exactly the size the call may touch, so that a stray access is a report.
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

// 7853200120776062878684798364095072458815029376092732009249414926327459813530 = poseidon([1, 2]), little-endian words
const uint64_t kHash12[4] = {0x9e19607a4417189aull, 0x2a3617f274324551ull, 0x3df64c6b9662e9cfull, 0x115cc0f5e7d69041ull};

std::vector<uint8_t> small(size_t count) {   // records 0, 1, 2, ..
  std::vector<uint8_t> v(count * 32, 0);
  for (size_t i = 0; i < count; ++i) v[i * 32] = (uint8_t)i, v[i * 32 + 1] = (uint8_t)(i >> 8);
  return v;
}

}  // namespace

int main() {
  const int canon = MSM_AMD_SCALAR_CANON_LE, mont = MSM_AMD_SCALAR_MONT_LE;
  const uint32_t r_p[6] = {0, 0, 56, 57, 56, 60};
  for (uint32_t t = 2; t <= 5; ++t) {
    for (int layout : {mont, canon}) {
      std::vector<uint8_t> ark((8 + r_p[t]) * t * 32), mds(t * t * 32);
      expect(msm_amd_poseidon_constants(t, 8, r_p[t], layout, ark.data(), mds.data()) == MSM_AMD_OK, "constants");
      const size_t n = 37;
      std::vector<uint8_t> states = small(n * t), out(n * t * 32), groups = small(n * (t - 1)), digests(n * 32);
      expect(msm_amd_host_poseidon_permute(t, 8, r_p[t], layout, ark.data(), mds.data(), states.data(), n, 3, out.data()) == MSM_AMD_OK,
             "permute");
      expect(msm_amd_host_poseidon_permute(t, 8, r_p[t], layout, ark.data(), mds.data(), states.data(), n, 1, states.data()) == MSM_AMD_OK &&
                 states == out,
             "permute in place");
      expect(msm_amd_host_poseidon_hash(t, 8, r_p[t], layout, ark.data(), mds.data(), nullptr, groups.data(), n, 16, digests.data()) ==
                 MSM_AMD_OK,
             "hash");
      if (t == 3 && layout == canon) {
        std::vector<uint8_t> in = small(3), one(32);   // records 0, 1, 2: hash the group (1, 2)
        expect(msm_amd_host_poseidon_hash(3, 8, 57, canon, ark.data(), mds.data(), nullptr, in.data() + 32, 1, 1, one.data()) == MSM_AMD_OK &&
                   std::memcmp(one.data(), kHash12, 32) == 0,
               "poseidon([1, 2])");
      }
      if (t >= 3) {
        const uint32_t a = t - 1;
        size_t leaves_n = 1, nodes = 0;
        for (int d = 0; d < 3; ++d) leaves_n *= a;
        for (size_t c = leaves_n / a; c >= 1; c /= a) nodes += c;
        std::vector<uint8_t> leaves = small(leaves_n), tree(nodes * 32), root(32);
        expect(msm_amd_host_poseidon_merkle_build(t, 8, r_p[t], layout, ark.data(), mds.data(), nullptr, leaves.data(), leaves_n, 3,
                                                  tree.data(), root.data()) == MSM_AMD_OK &&
                   std::memcmp(root.data(), tree.data() + (nodes - 1) * 32, 32) == 0,
               "merkle_build");
        std::vector<uint64_t> idx = {0, leaves_n - 1, leaves_n / 2};
        std::vector<uint8_t> paths(idx.size() * 3 * (a - 1) * 32);
        expect(msm_amd_host_poseidon_merkle_paths(t, layout, leaves.data(), leaves_n, tree.data(), idx.data(), idx.size(), 2,
                                                  paths.data()) == MSM_AMD_OK,
               "merkle_paths");
        idx[1] = leaves_n;
        expect(msm_amd_host_poseidon_merkle_paths(t, layout, leaves.data(), leaves_n, tree.data(), idx.data(), idx.size(), 2,
                                                  paths.data()) == MSM_AMD_INPUT_ERROR,
               "merkle_paths refuses an index = n_leaves");
        uint64_t counts[40];
        expect(msm_amd_test_poseidon_plan(t, leaves_n, 2, counts) == MSM_AMD_OK && counts[2] == nodes, "plan tap");
      }
    }
  }
  // the largest shape: 128 rounds, t = 5
  std::vector<uint8_t> ark(128 * 5 * 32), mds(25 * 32), state = small(5);
  expect(msm_amd_poseidon_constants(5, 64, 64, mont, ark.data(), mds.data()) == MSM_AMD_OK, "constants at 128 rounds");
  expect(msm_amd_host_poseidon_permute(5, 64, 64, mont, ark.data(), mds.data(), state.data(), 1, 1, state.data()) == MSM_AMD_OK,
         "permute at 128 rounds");
  expect(msm_amd_poseidon_constants(5, 64, 66, mont, ark.data(), mds.data()) == MSM_AMD_INPUT_ERROR, "129 rounds are refused");
  std::printf(failures ? "poseidon_asan_check: %d FAILED\n" : "poseidon_asan_check: ok\n", failures);
  return failures ? 1 : 0;
}
