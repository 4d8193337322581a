// Stand-alone AddressSanitizer / UBSan check of the host side of the multi-point polynomial calls: the twins
// msm_amd_host_fr_poly_eval_points and msm_amd_host_fr_poly_div_points, their shared argument check and the plan aid
// msm_amd_test_fr_poly_points_plan, linked straight from host_fr.hip (tools/multiopen_asan.sh builds and runs it; no GPU, no
// python).  Every buffer is a heap allocation of exactly the size the call may touch, so that a stray access is a report.
// What the twins compute is pinned to the big-integer model by tests/test_multiopen_host.py; here the results are held
// against each other (the values of the division and of the evaluation, the chain of single-point divisions by hand, in
// place and out of place, thread counts, the zero records at the top), over n <= 70, 257 and 513 with k = 1 .. 8, and every
// refused call must leave its outputs as they were.
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

// canonical records of small values, little-endian
std::vector<uint8_t> records(size_t count, uint64_t seed) {
  std::vector<uint8_t> v(count * 32, 0);
  uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
  for (size_t i = 0; i < count; ++i) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t w = x >> 8;
    std::memcpy(v.data() + i * 32, &w, 8);
  }
  return v;
}
bool all_bytes(const std::vector<uint8_t>& v, size_t from, size_t count, uint8_t byte) {
  for (size_t i = 0; i < count; ++i)
    if (v[from + i] != byte) return false;
  return true;
}

// the raw words 1 and r + 1 (canonical layout: both read as 1)
const uint64_t kR[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

}  // namespace

int main() {
  const int canon = MSM_AMD_SCALAR_CANON_LE, mont = MSM_AMD_SCALAR_MONT_LE;
  std::vector<size_t> sizes;
  for (size_t n = 1; n <= 70; ++n) sizes.push_back(n);
  sizes.push_back(257), sizes.push_back(513);
  for (size_t n : sizes) {
    for (size_t k = 1; k <= MSM_AMD_POLY_MAX_POINTS; ++k) {
      const int layout = (n + k) & 1 ? canon : mont;
      const size_t n_vec = n % 3 == 0 ? 3 : 1;
      const int threads = n & 2 ? 16 : 1;
      const std::vector<uint8_t> in = records(n * n_vec, n * 16 + k), z = records(k, n * 31 + k);
      std::vector<uint8_t> out(n * n_vec * 32, 0xFF), vals(n_vec * k * 32, 0xFF), y(n_vec * k * 32, 0xEE);
      expect(msm_amd_host_fr_poly_div_points(layout, z.data(), k, in.data(), n, n_vec, threads, out.data(), vals.data()) == MSM_AMD_OK,
             "div_points");
      expect(msm_amd_host_fr_poly_eval_points(layout, z.data(), k, in.data(), n, n_vec, threads, y.data()) == MSM_AMD_OK && y == vals,
             "eval_points gives the values of div_points");
      const size_t top = k < n ? k : n;
      for (size_t v = 0; v < n_vec; ++v) expect(all_bytes(out, ((v + 1) * n - top) * 32, top * 32, 0), "the top min(k, n) records are zero");
      // in place, without the values, other thread counts: the same bytes
      std::vector<uint8_t> io = in;
      expect(msm_amd_host_fr_poly_div_points(layout, z.data(), k, io.data(), n, n_vec, 17 - threads, io.data(), nullptr) == MSM_AMD_OK &&
                 io == out,
             "in place");
      if (k == 1) {
        std::vector<uint8_t> q1(n * n_vec * 32, 0xDD), r1(n_vec * 32, 0xDD);
        expect(msm_amd_host_fr_poly_div_linear(layout, z.data(), in.data(), n, n_vec, threads, q1.data(), r1.data()) == MSM_AMD_OK &&
                   q1 == out && r1 == vals,
               "k = 1 is the single-point division");
      }
      // dividing the quotient's chain by hand: k single-point divisions give the same bytes
      std::vector<uint8_t> chain = in;
      for (size_t j = 0; j < k; ++j)
        expect(msm_amd_host_fr_poly_div_linear(layout, z.data() + j * 32, chain.data(), n, n_vec, 3, chain.data(), nullptr) == MSM_AMD_OK,
               "div_linear");
      expect(chain == out, "the chain by hand");
      uint64_t plan[8];
      expect(msm_amd_test_fr_poly_points_plan(n, n_vec, k, 2, 1, plan) == MSM_AMD_OK && plan[5] < 4096 && plan[3] == 32 * plan[2],
             "plan");
    }
  }
  // every refused call leaves the outputs
  const size_t n = 8, k = 3;
  const std::vector<uint8_t> in = records(2 * n + 1, 5), z = records(9, 6);
  std::vector<uint8_t> out(n * 2 * 32, 0xFF), vals(2 * 9 * 32, 0xFF);
  const std::vector<uint8_t> out0 = out, vals0 = vals;
  const int bad = MSM_AMD_INPUT_ERROR;
  expect(msm_amd_host_fr_poly_div_points(2, z.data(), k, in.data(), n, 2, 0, out.data(), vals.data()) == bad, "layout");
  expect(msm_amd_host_fr_poly_eval_points(7, z.data(), k, in.data(), n, 2, 0, vals.data()) == bad, "layout");
  expect(msm_amd_host_fr_poly_div_points(canon, z.data(), 0, in.data(), n, 2, 0, out.data(), vals.data()) == bad, "k = 0");
  expect(msm_amd_host_fr_poly_div_points(canon, z.data(), 9, in.data(), n, 2, 0, out.data(), vals.data()) == bad, "k = 9");
  expect(msm_amd_host_fr_poly_eval_points(canon, z.data(), 0, in.data(), n, 2, 0, vals.data()) == bad, "k = 0");
  expect(msm_amd_host_fr_poly_eval_points(canon, z.data(), 9, in.data(), n, 2, 0, vals.data()) == bad, "k = 9");
  expect(msm_amd_host_fr_poly_div_points(canon, nullptr, k, in.data(), n, 2, 0, out.data(), vals.data()) == bad, "null z");
  expect(msm_amd_host_fr_poly_eval_points(canon, nullptr, k, in.data(), n, 2, 0, vals.data()) == bad, "null z");
  expect(msm_amd_host_fr_poly_div_points(canon, z.data(), k, nullptr, n, 2, 0, out.data(), vals.data()) == bad, "null in");
  expect(msm_amd_host_fr_poly_div_points(canon, z.data(), k, in.data(), n, 2, 0, nullptr, vals.data()) == bad, "null out");
  expect(msm_amd_host_fr_poly_eval_points(canon, z.data(), k, in.data(), n, 2, 0, nullptr) == bad, "null y");
  expect(msm_amd_host_fr_poly_div_points(canon, z.data(), k, in.data(), (size_t)1 << 32, 1, 0, out.data(), vals.data()) == bad, "n");
  std::vector<uint8_t> io = in;
  const std::vector<uint8_t> io0 = io;
  expect(msm_amd_host_fr_poly_div_points(canon, z.data(), k, io.data(), n, 2, 0, io.data() + 32, vals.data()) == bad, "overlap");
  expect(msm_amd_host_fr_poly_div_points(canon, z.data(), k, io.data() + 32, n, 2, 0, io.data(), vals.data()) == bad, "overlap");
  std::vector<uint8_t> same = records(3, 9);   // the raw words 1 and r + 1
  std::memset(same.data(), 0, 32), same[0] = 1;
  uint64_t r1[4] = {kR[0] + 1, kR[1], kR[2], kR[3]};
  std::memcpy(same.data() + 64, r1, 32);
  for (int layout : {canon, mont}) {
    expect(msm_amd_host_fr_poly_div_points(layout, same.data(), 3, in.data(), n, 2, 0, out.data(), vals.data()) == bad, "equal points");
    expect(msm_amd_host_fr_poly_div_points(layout, same.data(), 3, io.data(), n, 2, 0, io.data(), nullptr) == bad, "equal points, in place");
  }
  expect(out == out0 && vals == vals0 && io == io0, "a refused call writes nothing");
  expect(msm_amd_host_fr_poly_eval_points(canon, same.data(), 3, in.data(), n, 2, 0, vals.data()) == MSM_AMD_OK &&
             std::memcmp(vals.data(), vals.data() + 64, 32) == 0 && std::memcmp(vals.data() + 96, vals.data() + 160, 32) == 0,
         "the evaluation takes a repeated point");
  // nothing to do
  vals = vals0;
  expect(msm_amd_host_fr_poly_div_points(canon, z.data(), k, nullptr, 0, 2, 0, nullptr, vals.data()) == MSM_AMD_OK, "n = 0");
  expect(msm_amd_host_fr_poly_eval_points(canon, z.data(), k, nullptr, n, 0, 0, vals.data()) == MSM_AMD_OK && vals == vals0, "n_vec = 0");
  uint64_t plan[8];
  expect(msm_amd_test_fr_poly_points_plan(8, 1, 9, 9, 1, plan) == bad && msm_amd_test_fr_poly_points_plan(8, 1, 0, 9, 0, plan) == bad &&
             msm_amd_test_fr_poly_points_plan(8, 1, 3, 10, 0, plan) == bad && msm_amd_test_fr_poly_points_plan(8, 1, 3, 9, 0, nullptr) == bad,
         "plan arguments");
  if (failures) return 1;
  std::printf("multiopen_asan_check: ok\n");
  return 0;
}
