// Stand-alone AddressSanitizer / UBSan check of the host side of the sort of Fr records by canonical value and of the
// permuted lookup columns in value order: the twins msm_amd_host_fr_sort and msm_amd_host_fr_lookup_permute_as and the planner
// msm_amd_test_fr_sort_plan, linked straight from host_fr_sort.hip and host_lookup.hip (tools/sort_asan.sh builds and runs it;
// no GPU, no python).  Every buffer is a heap allocation of exactly the size the call may touch, so that a stray access is a
// report.
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
  for (uint32_t mask : {0u, 1u, 0x3u, 0x80000000u, 0x00020001u, 0xFFFFFFFFu}) {
    uint64_t plan[4];
    const uint64_t passes = (uint64_t)__builtin_popcount(mask);
    expect(msm_amd_test_fr_sort_plan(4097, 3, mask, plan) == MSM_AMD_OK && plan[0] == passes && plan[1] >= 1 + 3 * (3 * passes + 1) &&
               plan[2] == 2 && plan[3] >= 32 * 3 * 4097,
           "plan");
    expect(msm_amd_test_fr_sort_plan(0, 1, mask, plan) == MSM_AMD_INPUT_ERROR, "plan of nothing");
  }
  for (size_t n : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)257, (size_t)1000, (size_t)4097}) {
    for (int layout : {mont, canon}) {
      for (int threads : {1, 3, 16}) {
        // column 0: (i * 7919) mod 1000 -- many ties; column 1: one value; column 2: descending
        const size_t n_vec = 3;
        const std::vector<uint8_t> in = records(n * n_vec, [&](size_t i) {
          return i < n ? (i * 7919) % 1000 : i < 2 * n ? 5 : 3 * n - i;
        });
        std::vector<uint8_t> out(n * n_vec * 32, 0xFF);
        std::vector<uint32_t> perm(n * n_vec, 0xFFFFFFFFu);
        expect(msm_amd_host_fr_sort(layout, in.data(), n, n_vec, threads, out.data(), perm.data()) == MSM_AMD_OK, "sort");
        for (size_t v = 0; v < n_vec; ++v)
          for (size_t k = 0; k < n; ++k) {
            const uint32_t p = perm[v * n + k];
            expect(p < n, "perm in range");
            if (p >= n) continue;
            if (layout == canon) expect(word0(out, v * n + k) == word0(in, v * n + p), "out is the permuted input");
            if (k && layout == canon) {
              const uint64_t a = word0(in, v * n + perm[v * n + k - 1]), b = word0(in, v * n + p);
              expect(a < b || (a == b && perm[v * n + k - 1] < p), "ascending and stable");
            }
          }
        std::vector<uint8_t> out2(n * n_vec * 32, 0xEE);
        std::vector<uint32_t> perm2(n * n_vec, 0xEEEEEEEEu);
        expect(msm_amd_host_fr_sort(layout, in.data(), n, n_vec, threads, out2.data(), nullptr) == MSM_AMD_OK && out2 == out, "out alone");
        expect(msm_amd_host_fr_sort(layout, in.data(), n, n_vec, threads, nullptr, perm2.data()) == MSM_AMD_OK && perm2 == perm, "perm alone");
        std::vector<uint8_t> io = in;
        expect(msm_amd_host_fr_sort(layout, io.data(), n, n_vec, threads, io.data(), nullptr) == MSM_AMD_OK && io == out, "in place");

        // the permuted columns in value order: the table holds j / 2 in descending row order
        const size_t distinct = (n + 1) / 2;
        const std::vector<uint8_t> table = records(n, [&](size_t j) { return (n - 1 - j) / 2; });
        const std::vector<uint8_t> col = records(n * n_vec, [&](size_t i) {
          return i < n ? (i * 7) % distinct : i < 2 * n ? distinct - 1 : (i - 2 * n) / 2;
        });
        std::vector<uint8_t> a(n * n_vec * 32, 0xFF), s(n * n_vec * 32, 0xFF);
        uint64_t report[4] = {9, 9, 9, 9};
        expect(msm_amd_host_fr_lookup_permute_as(layout, MSM_AMD_PERMUTE_HALO2, table.data(), n, col.data(), n, n_vec, threads, a.data(),
                                                 s.data(), report) == MSM_AMD_OK,
               "permute_as");
        expect(report[0] == 0 && report[1] == ~(uint64_t)0 && report[3] == n, "report");
        if (layout == canon)
          for (size_t v = 0; v < n_vec; ++v) {
            std::vector<uint64_t> got(n);
            for (size_t i = 0; i < n; ++i) got[i] = word0(a, v * n + i);
            expect(got == sorted_words(col, v * n, n), "A' is A ascending");
            expect(sorted_words(s, v * n, n) == sorted_words(table, 0, n), "S' is a permutation of S");
            expect(word0(a, v * n) == word0(s, v * n), "A'[0] = S'[0]");
            for (size_t i = v * n + 1; i < (v + 1) * n; ++i)
              expect(word0(a, i) == word0(s, i) || word0(a, i) == word0(a, i - 1), "A'[i] = S'[i] or A'[i] = A'[i-1]");
          }
        std::vector<uint8_t> bad = col, a3(n * n_vec * 32, 0xEE), s3(n * n_vec * 32, 0xEE);
        const uint64_t outside = distinct + 3;
        std::memcpy(bad.data() + (n * n_vec - 1) * 32, &outside, 8);
        expect(msm_amd_host_fr_lookup_permute_as(layout, MSM_AMD_PERMUTE_HALO2, table.data(), n, bad.data(), n, n_vec, threads,
                                                 a3.data(), s3.data(), report) == MSM_AMD_INPUT_ERROR && report[0] == 1,
               "a miss");
        expect(a3 == std::vector<uint8_t>(n * n_vec * 32, 0xEE) && s3 == a3, "a miss leaves the outputs");
      }
    }
  }
  // the worked example of the header
  const uint64_t A[5] = {2, 2, 1, 2, 5}, S[5] = {5, 1, 2, 7, 1}, Ap[5] = {1, 2, 2, 2, 5}, Sp[5] = {1, 2, 7, 1, 5};
  const std::vector<uint8_t> ra = records(5, [&](size_t i) { return A[i]; }), rs = records(5, [&](size_t i) { return S[i]; });
  std::vector<uint8_t> a(5 * 32), s(5 * 32);
  uint64_t report[4];
  expect(msm_amd_host_fr_lookup_permute_as(canon, MSM_AMD_PERMUTE_HALO2, rs.data(), 5, ra.data(), 5, 1, 0, a.data(), s.data(), report) ==
             MSM_AMD_OK && a == records(5, [&](size_t i) { return Ap[i]; }) && s == records(5, [&](size_t i) { return Sp[i]; }),
         "the worked example");
  std::vector<uint8_t> one(32, 0), out(32);
  std::vector<uint32_t> p1(1);
  expect(msm_amd_host_fr_sort(canon, one.data(), 1, 1, 0, nullptr, nullptr) == MSM_AMD_INPUT_ERROR, "no output");
  expect(msm_amd_host_fr_sort(canon, nullptr, 0, 1, 0, out.data(), nullptr) == MSM_AMD_OK, "n = 0");
  expect(msm_amd_host_fr_sort(canon, one.data(), 1, 1, 0, out.data(), p1.data()) == MSM_AMD_OK && p1[0] == 0, "n = 1");
  if (failures) return 1;
  std::printf("sort_asan_check: ok\n");
  return 0;
}
