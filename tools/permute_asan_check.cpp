// Stand-alone AddressSanitizer / UBSan check of the host side of halo2's permuted lookup columns: the twin
// msm_amd_host_fr_lookup_permute (the shared bodies of fr_permute.hip.h over the index of fr_lookup.hip.h) and the plan tap,
// linked straight from host_lookup.hip (tools/permute_asan.sh builds and runs it; no GPU, no python).  Every buffer is a heap
// allocation of exactly the size the call may touch, so that a stray access is a report.
#include <algorithm>
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

// canonical records of value(i), little-endian
template <class F>
std::vector<uint8_t> records(size_t count, F value) {
  std::vector<uint8_t> v(count * 32, 0);
  for (size_t i = 0; i < count; ++i) {
    const uint64_t x = value(i);
    std::memcpy(v.data() + i * 32, &x, 8);
  }
  return v;
}
uint64_t word0(const std::vector<uint8_t>& v, size_t i) {
  uint64_t x;
  std::memcpy(&x, v.data() + i * 32, 8);
  return x;
}
std::vector<uint64_t> sorted_words(const std::vector<uint8_t>& v, size_t from, size_t count) {
  std::vector<uint64_t> w(count);
  for (size_t i = 0; i < count; ++i) w[i] = word0(v, from + i);
  std::sort(w.begin(), w.end());
  return w;
}

}  // namespace

int main() {
  const int canon = MSM_AMD_SCALAR_CANON_LE, mont = MSM_AMD_SCALAR_MONT_LE;
  for (size_t n : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)257, (size_t)1000}) {
    for (uint32_t tile_log = 2; tile_log <= 11; ++tile_log) {
      uint64_t plan[4];
      expect(msm_amd_test_fr_permute_plan(n, 3, tile_log, plan) == MSM_AMD_OK && plan[0] >= 1 && plan[1] == 2 * plan[0] + 1 &&
                 plan[2] == 3 * ((n + ((size_t)1 << tile_log) - 1) >> tile_log) && plan[3] >= 16 * 3 * n,
             "plan");
    }
    for (int layout : {mont, canon}) {
      for (int threads : {1, 3, 16}) {
        // row j holds j / 2: pairs of equal rows.  Column 0 draws i * 7 mod the distinct values, column 1 is one value n
        // times, column 2 holds every row's value once
        const size_t n_vec = 3, distinct = (n + 1) / 2;
        const std::vector<uint8_t> table = records(n, [](size_t j) { return j / 2; });
        const std::vector<uint8_t> in = records(n * n_vec, [&](size_t i) {
          return i < n ? (i * 7) % distinct : i < 2 * n ? distinct - 1 : (i - 2 * n) / 2;
        });
        std::vector<uint8_t> a(n * n_vec * 32, 0xFF), s(n * n_vec * 32, 0xFF);
        uint64_t report[4] = {9, 9, 9, 9};
        expect(msm_amd_host_fr_lookup_permute(layout, table.data(), n, in.data(), n, n_vec, threads, a.data(), s.data(), report) ==
                   MSM_AMD_OK,
               "permute");
        expect(report[0] == 0 && report[1] == ~(uint64_t)0 && report[3] == n, "report");
        if (layout == canon)
          for (size_t v = 0; v < n_vec; ++v) {
            expect(sorted_words(a, v * n, n) == sorted_words(in, v * n, n), "A' is a permutation of A");
            expect(sorted_words(s, v * n, n) == sorted_words(table, 0, n), "S' is a permutation of S");
            expect(word0(a, v * n) == word0(s, v * n), "A'[0] = S'[0]");
            for (size_t i = v * n + 1; i < (v + 1) * n; ++i)
              expect(word0(a, i) == word0(s, i) || word0(a, i) == word0(a, i - 1), "A'[i] = S'[i] or A'[i] = A'[i-1]");
          }
        // each output alone, A' alone at other lengths, in place
        std::vector<uint8_t> a2(n * n_vec * 32, 0xEE), s2(n * n_vec * 32, 0xEE);
        expect(msm_amd_host_fr_lookup_permute(layout, table.data(), n, in.data(), n, n_vec, threads, a2.data(), nullptr, report) ==
                       MSM_AMD_OK && a2 == a, "A' alone");
        expect(msm_amd_host_fr_lookup_permute(layout, table.data(), n, in.data(), n, n_vec, threads, nullptr, s2.data(), report) ==
                       MSM_AMD_OK && s2 == s, "S' alone");
        for (size_t m : {(size_t)1, n + 5}) {
          std::vector<uint8_t> io = records(m * 2, [&](size_t i) { return (i * 3) % distinct; }), first = io;
          expect(msm_amd_host_fr_lookup_permute(layout, table.data(), n, io.data(), m, 2, threads, io.data(), nullptr, report) ==
                         MSM_AMD_OK, "in place");
          if (layout == canon) expect(sorted_words(io, 0, m) == sorted_words(first, 0, m), "in place: a permutation");
        }
        // a value that is in no row: both outputs stay
        std::vector<uint8_t> bad = in, a3(n * n_vec * 32, 0xEE), s3(n * n_vec * 32, 0xEE);
        const uint64_t outside = distinct + 3;
        std::memcpy(bad.data() + (n * n_vec - 1) * 32, &outside, 8);
        expect(msm_amd_host_fr_lookup_permute(layout, table.data(), n, bad.data(), n, n_vec, threads, a3.data(), s3.data(), report) ==
                       MSM_AMD_INPUT_ERROR && report[0] == 1 && report[1] == n * n_vec - 1, "a miss");
        expect(a3 == std::vector<uint8_t>(n * n_vec * 32, 0xEE) && s3 == a3, "a miss leaves the outputs");
      }
    }
  }
  uint64_t report[4];
  std::vector<uint8_t> one(32, 0), out(32);
  expect(msm_amd_host_fr_lookup_permute(canon, one.data(), 1, one.data(), 1, 1, 0, nullptr, nullptr, report) == MSM_AMD_INPUT_ERROR, "no output");
  expect(msm_amd_host_fr_lookup_permute(canon, one.data(), 1, nullptr, 0, 1, 0, out.data(), nullptr, report) == MSM_AMD_OK, "n = 0");
  if (failures) return 1;
  std::printf("permute_asan_check: ok\n");
  return 0;
}
