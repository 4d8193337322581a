// Stand-alone AddressSanitizer / UBSan check of the host side of the lookup calls: the multiplicities twin (index build and
// probes of fr_lookup.hip.h), the running sums, the shift and the plan tap, linked straight from host_lookup.hip and
// host_fr.hip (tools/lookup_asan.sh builds and runs it; no GPU, no python).  Every buffer is a heap allocation of exactly the
// size the call may touch, so that a stray access is a report.
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

}  // namespace

int main() {
  const int canon = MSM_AMD_SCALAR_CANON_LE, mont = MSM_AMD_SCALAR_MONT_LE;
  for (size_t n_rows : {(size_t)1, (size_t)2, (size_t)63, (size_t)64, (size_t)65, (size_t)257}) {
    uint64_t plan[4];
    expect(msm_amd_test_fr_lookup_plan(n_rows, 32, plan) == MSM_AMD_OK && plan[0] >= 2 * n_rows && !(plan[0] & (plan[0] - 1)), "plan");
    for (int layout : {mont, canon}) {
      for (int threads : {1, 3, 16}) {
        // row j holds j / 2: pairs of equal rows; input i holds i mod (n_rows / 2 + 1), the last value is in no row when
        // n_rows is even
        const std::vector<uint8_t> table = records(n_rows, [](size_t j) { return j / 2; });
        const size_t n = 333, n_vec = 3, distinct = (n_rows + 1) / 2;
        const std::vector<uint8_t> in = records(n * n_vec, [&](size_t i) { return i % (n_rows / 2 + 1); });
        std::vector<uint8_t> m(n_rows * 32, 0xFF);
        std::vector<uint32_t> idx(n * n_vec, 7);
        uint64_t report[4] = {9, 9, 9, 9};
        const int rc = msm_amd_host_fr_lookup_multiplicities(layout, MSM_AMD_LOOKUP_COUNT_MISSING, table.data(), n_rows, in.data(), n,
                                                             n_vec, threads, m.data(), idx.data(), report);
        expect(rc == MSM_AMD_OK, "multiplicities");
        uint64_t misses = 0, first = ~(uint64_t)0;
        for (size_t i = 0; i < n * n_vec; ++i) {
          const uint64_t v = i % (n_rows / 2 + 1);
          const bool hit = v < distinct;
          if (!hit) ++misses, first = first < i ? first : i;
          expect(idx[i] == (hit ? (uint32_t)(2 * v) : 0xFFFFFFFFu), "row index");
        }
        expect(report[0] == misses && report[1] == first, "misses");
        expect(report[2] == distinct, "rows hit");
        std::vector<uint8_t> strict(n_rows * 32, 0xEE);
        const int rs = msm_amd_host_fr_lookup_multiplicities(layout, MSM_AMD_LOOKUP_STRICT, table.data(), n_rows, in.data(), n, n_vec,
                                                             threads, strict.data(), nullptr, report);
        expect(rs == (misses ? MSM_AMD_INPUT_ERROR : MSM_AMD_OK), "strict");
        expect(misses ? strict == std::vector<uint8_t>(n_rows * 32, 0xEE) : strict == m, "strict m");
        if (layout == canon)
          for (size_t j = 0; j < n_rows; ++j) expect((j % 2 == 0) == (word0(m, j) != 0), "representative");
      }
    }
  }
  for (int layout : {mont, canon}) {
    for (size_t n : {(size_t)1, (size_t)511, (size_t)512, (size_t)513}) {
      const size_t n_vec = 3;
      const std::vector<uint8_t> in = records(n * n_vec, [](size_t i) { return i + 1; });
      std::vector<uint8_t> out(n * n_vec * 32), again = in, k = records(1, [](size_t) { return 5; }), shifted(n * n_vec * 32);
      expect(msm_amd_host_fr_prefix_sum(layout, MSM_AMD_FR_PREFIX_INCLUSIVE, in.data(), n, n_vec, 3, out.data()) == MSM_AMD_OK, "sum");
      expect(msm_amd_host_fr_prefix_sum(layout, MSM_AMD_FR_PREFIX_INCLUSIVE, again.data(), n, n_vec, 16, again.data()) == MSM_AMD_OK &&
                 again == out,
             "sum in place");
      expect(msm_amd_host_fr_prefix_sum(layout, MSM_AMD_FR_PREFIX_EXCLUSIVE, in.data(), n, n_vec, 1, out.data()) == MSM_AMD_OK, "exclusive");
      if (layout == canon) expect(word0(out, 0) == 0 && (n < 2 || word0(out, 1) == 1), "exclusive starts at 0");
      expect(msm_amd_host_fr_shift(layout, k.data(), in.data(), n * n_vec, 3, shifted.data()) == MSM_AMD_OK, "shift");
      if (layout == canon) expect(word0(shifted, n * n_vec - 1) == n * n_vec + 5, "shift value");
    }
  }
  if (failures) return 1;
  std::printf("lookup_asan_check: ok\n");
  return 0;
}
