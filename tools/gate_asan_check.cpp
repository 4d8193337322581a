// Stand-alone AddressSanitizer / UBSan check of the host side of the gate polynomials: the twin msm_amd_host_fr_gate_eval, the
// shared check msm_amd_fr_gate_check and the plan aid msm_amd_test_fr_gate_plan, linked straight from host_fr.hip
// (tools/gate_asan.sh builds and runs it; no GPU, no python).  Every buffer is a heap allocation of exactly the size the call
// may touch, so that a stray access is a report: the columns end with the last record of the last column, `out` holds n
// records, the scale table `period`, the term list exactly its factors.  What the twin computes is pinned to the big-integer
// model by tests/test_gate_host.py; here its bytes are held against the chain of msm_amd_host_fr_map calls over columns
// rotated by hand (the vanilla PLONK gate with c one row on, folded by ACCUMULATE and scaled), over n = 1 .. 70, 255 .. 257 and
// 1000, both layouts and several thread counts, and every refused call must leave its output as it was.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <utility>
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

// r - 1, canonical
const uint64_t kRm1[4] = {0x43e1f593f0000000ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

struct Terms {
  std::vector<uint8_t> coeff;
  std::vector<uint32_t> len, col;
  std::vector<int32_t> rot;
  msm_amd_fr_gate_terms c;
  void add(const void* coeff32, std::initializer_list<std::pair<uint32_t, int32_t>> factors) {
    coeff.insert(coeff.end(), (const uint8_t*)coeff32, (const uint8_t*)coeff32 + 32);
    len.push_back((uint32_t)factors.size());
    for (auto f : factors) col.push_back(f.first), rot.push_back(f.second);
  }
  const msm_amd_fr_gate_terms* get() {
    c = {(uint32_t)len.size(), coeff.data(), len.data(), col.data(), rot.data()};
    return &c;
  }
};

// column `col` of `in` read `by` rows on, as a vector of its own
std::vector<uint8_t> rotated(const std::vector<uint8_t>& in, size_t n, size_t stride, size_t col, long long by) {
  std::vector<uint8_t> out(n * 32);
  for (size_t i = 0; i < n; ++i) {
    const size_t row = (size_t)((((long long)i + by) % (long long)n + (long long)n) % (long long)n);
    std::memcpy(out.data() + i * 32, in.data() + (col * stride + row) * 32, 32);
  }
  return out;
}

}  // namespace

int main() {
  const int canon = MSM_AMD_SCALAR_CANON_LE, mont = MSM_AMD_SCALAR_MONT_LE;
  std::vector<size_t> sizes;
  for (size_t n = 1; n <= 70; ++n) sizes.push_back(n);
  for (size_t n : {255, 256, 257, 1000}) sizes.push_back(n);
  for (size_t n : sizes) {
    for (int layout : {canon, mont}) {
      const size_t n_vec = 8, stride = n + (n & 1 ? 5 : 0);
      const int threads = n & 2 ? 16 : 1;
      const uint64_t rot_step = n % 3 + 1;
      const std::vector<uint8_t> in = records((n_vec - 1) * stride + n, n * 4 + layout);
      // the words 1 and r - 1: in CANON_LE the coefficients that cost no product, in MONT_LE the values R^-1 and -R^-1, which
      // cost one -- either way the chain below multiplies by the same records
      std::vector<uint8_t> one(32, 0), minus(32, 0);
      one[0] = 1;
      std::memcpy(minus.data(), kRm1, 32);
      Terms t;   // q_L a + q_R b + q_M a b - q_O c(+1) + q_C over columns q_L q_R q_M q_O q_C a b c
      t.add(one.data(), {{0, 0}, {5, 0}});
      t.add(one.data(), {{1, 0}, {6, 0}});
      t.add(one.data(), {{2, 0}, {5, 0}, {6, 0}});
      t.add(minus.data(), {{3, 0}, {7, 1}});
      t.add(one.data(), {{4, 0}});
      uint32_t degree = 0, offsets = 0;
      expect(msm_amd_fr_gate_check(t.get(), n_vec, n, rot_step, &degree, &offsets) == MSM_AMD_OK && degree == 3 &&
                 offsets == (rot_step % n ? 2u : 1u) && msm_amd_fr_gate_last_error()[0] == 0,
             "check");
      std::vector<uint8_t> out(n * 32, 0xFF);
      expect(msm_amd_host_fr_gate_eval(layout, 0, t.get(), in.data(), n, n_vec, stride, rot_step, nullptr, nullptr, 0, threads,
                                       out.data()) == MSM_AMD_OK,
             "gate_eval");
      // the chain a caller has without the call: coefficients `one` / `minus` enter through SCALE
      auto col = [&](size_t v) { return rotated(in, n, stride, v, 0); };
      auto map = [&](int op, const void* k, const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
        std::vector<uint8_t> r(n * 32);
        expect(msm_amd_host_fr_map(op, layout, k, a.data(), b.data(), nullptr, n, 3, r.data()) == MSM_AMD_OK, "map");
        return r;
      };
      const std::vector<uint8_t> c_next = rotated(in, n, stride, 7, (long long)rot_step);
      std::vector<uint8_t> sum = map(MSM_AMD_FR_SCALE, one.data(), map(MSM_AMD_FR_MUL, nullptr, col(0), col(5)), col(0));
      sum = map(MSM_AMD_FR_AXPY, one.data(), sum, map(MSM_AMD_FR_MUL, nullptr, col(1), col(6)));
      sum = map(MSM_AMD_FR_AXPY, one.data(), sum, map(MSM_AMD_FR_MUL, nullptr, map(MSM_AMD_FR_MUL, nullptr, col(2), col(5)), col(6)));
      sum = map(MSM_AMD_FR_AXPY, minus.data(), sum, map(MSM_AMD_FR_MUL, nullptr, col(3), c_next));
      sum = map(MSM_AMD_FR_AXPY, one.data(), sum, col(4));
      expect(sum == out, "the gate is the chain of maps");
      // other thread counts: the same bytes
      std::vector<uint8_t> again(n * 32, 0xEE);
      expect(msm_amd_host_fr_gate_eval(layout, 0, t.get(), in.data(), n, n_vec, stride, rot_step, nullptr, nullptr, 0, 17 - threads,
                                       again.data()) == MSM_AMD_OK && again == out,
             "thread counts");
      // ACCUMULATE and a scale of the largest period that divides n: (k out + v) s[i mod period]
      size_t period = 1;
      while (period < MSM_AMD_GATE_MAX_PERIOD && n % (period * 2) == 0) period *= 2;
      const std::vector<uint8_t> old = records(n, n + 7), k_acc = records(1, n + 8), scale = records(period, n + 9);
      std::vector<uint8_t> acc = old;
      expect(msm_amd_host_fr_gate_eval(layout, MSM_AMD_GATE_ACCUMULATE, t.get(), in.data(), n, n_vec, stride, rot_step, k_acc.data(),
                                       scale.data(), period, threads, acc.data()) == MSM_AMD_OK,
             "accumulate and scale");
      std::vector<uint8_t> tiled(n * 32);
      for (size_t i = 0; i < n; ++i) std::memcpy(tiled.data() + i * 32, scale.data() + (i % period) * 32, 32);
      expect(map(MSM_AMD_FR_MUL, nullptr, map(MSM_AMD_FR_AXPY, k_acc.data(), out, old), tiled) == acc, "k out + v, scaled");
      uint64_t plan[8];
      expect(msm_amd_test_fr_gate_plan(layout, MSM_AMD_GATE_ACCUMULATE, t.get(), n, n_vec, rot_step, period, plan) == MSM_AMD_OK &&
                 plan[0] == 1 && plan[1] == (n + 255) / 256 && plan[2] == 12 && plan[4] == offsets && plan[5] == period * 32 &&
                 plan[6] == 3,
             "plan");
    }
  }
  // rotations at the ends of int32 and a step of 2^40: the reduction must not overflow; n = 1: every row is row 0
  {
    const size_t n = 7;
    const std::vector<uint8_t> in = records(n, 3);
    std::vector<uint8_t> one(32, 0);
    one[0] = 1;
    Terms t;
    t.add(one.data(), {{0, INT_MIN}});
    std::vector<uint8_t> out(n * 32, 0xFF);
    expect(msm_amd_host_fr_gate_eval(canon, 0, t.get(), in.data(), n, 1, n, 1ull << 40, nullptr, nullptr, 0, 1, out.data()) == MSM_AMD_OK,
           "INT32_MIN");
    // -2^31 2^40 = -2^71 = -(2^71 mod 7) = -(2^(71 mod 3)) = -4 = 3 mod 7
    expect(out == rotated(in, n, n, 0, 3), "INT32_MIN at rot_step 2^40, n = 7");
    Terms far;
    far.add(one.data(), {{0, INT_MAX}, {0, -1}});
    expect(msm_amd_host_fr_gate_eval(canon, 0, far.get(), in.data(), 1, 1, 1, ~0ull, nullptr, nullptr, 0, 1, out.data()) == MSM_AMD_OK,
           "n = 1");
  }
  // every refused call leaves the output
  const size_t n = 16;
  const std::vector<uint8_t> in = records(2 * n, 5), rec = records(4, 6);
  std::vector<uint8_t> out(n * 32, 0xFF);
  const std::vector<uint8_t> out0 = out;
  const int bad = MSM_AMD_INPUT_ERROR;
  Terms good;
  good.add(rec.data(), {{0, 1}, {1, -1}});
  auto call = [&](int layout, uint32_t flags, const msm_amd_fr_gate_terms* t, const void* src, size_t rows, size_t n_vec, size_t stride,
                  uint64_t step, const void* k, const void* s, size_t period, void* dst) {
    return msm_amd_host_fr_gate_eval(layout, flags, t, src, rows, n_vec, stride, step, k, s, period, 2, dst);
  };
  expect(call(2, 0, good.get(), in.data(), n, 2, n, 1, nullptr, nullptr, 0, out.data()) == bad, "layout");
  expect(call(canon, 2, good.get(), in.data(), n, 2, n, 1, nullptr, nullptr, 0, out.data()) == bad, "flags");
  expect(call(canon, 1, good.get(), in.data(), n, 2, n, 1, nullptr, nullptr, 0, out.data()) == bad, "null k_acc");
  expect(call(canon, 0, nullptr, in.data(), n, 2, n, 1, nullptr, nullptr, 0, out.data()) == bad, "null list");
  expect(call(canon, 0, good.get(), nullptr, n, 2, n, 1, nullptr, nullptr, 0, out.data()) == bad, "null in");
  expect(call(canon, 0, good.get(), in.data(), n, 2, n, 1, nullptr, nullptr, 0, nullptr) == bad, "null out");
  expect(call(canon, 0, good.get(), in.data(), n, 2, n, 0, nullptr, nullptr, 0, out.data()) == bad, "rot_step = 0");
  expect(call(canon, 0, good.get(), in.data(), n, 1, n, 1, nullptr, nullptr, 0, out.data()) == bad, "column index");
  expect(call(canon, 0, good.get(), in.data(), n, 2, n - 1, 1, nullptr, nullptr, 0, out.data()) == bad, "stride");
  expect(call(canon, 0, good.get(), in.data(), (size_t)1 << 32, 2, (size_t)1 << 32, 1, nullptr, nullptr, 0, out.data()) == bad, "n");
  for (size_t period : {0, 3, 32, 512})
    expect(call(canon, 0, good.get(), in.data(), n, 2, n, 1, nullptr, rec.data(), period, out.data()) == bad, "period");
  Terms nine, long_term, empty;
  nine.add(rec.data(), {{0, 0}, {0, 1}, {0, 2}, {0, 3}, {0, 4}});
  nine.add(rec.data(), {{1, 5}, {1, 6}, {1, 7}, {1, 8}});
  long_term.add(rec.data(), {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}});
  expect(call(canon, 0, nine.get(), in.data(), n, 2, n, 1, nullptr, nullptr, 0, out.data()) == bad &&
             std::strstr(msm_amd_fr_gate_last_error(), "distinct offsets"),
         "nine offsets");
  expect(call(canon, 0, nine.get(), in.data(), 8, 2, n, 1, nullptr, nullptr, 0, out.data()) == MSM_AMD_OK, "eight offsets at n = 8");
  out = out0;
  expect(call(canon, 0, long_term.get(), in.data(), n, 2, n, 1, nullptr, nullptr, 0, out.data()) == bad, "nine factors");
  expect(call(canon, 0, empty.get(), in.data(), n, 2, n, 1, nullptr, nullptr, 0, out.data()) == bad, "no terms");
  std::vector<uint8_t> io = records(3 * n, 8);
  const std::vector<uint8_t> io0 = io;
  expect(call(canon, 0, good.get(), io.data(), n, 2, n, 1, nullptr, nullptr, 0, io.data()) == bad, "in place");
  expect(call(canon, 0, good.get(), io.data(), n, 2, n, 1, nullptr, nullptr, 0, io.data() + (2 * n - 1) * 32) == bad, "overlap");
  expect(call(canon, 0, good.get(), io.data() + n * 32, n, 2, n, 1, nullptr, nullptr, 0, io.data() + 32) == bad, "overlap");
  expect(out == out0 && io == io0, "a refused call writes nothing");
  // nothing to do
  expect(call(canon, 0, nullptr, nullptr, 0, 2, 0, 1, nullptr, nullptr, 0, nullptr) == MSM_AMD_OK, "n = 0");
  expect(call(canon, 0, nullptr, nullptr, n, 0, n, 1, nullptr, nullptr, 0, out.data()) == MSM_AMD_OK && out == out0, "n_vec = 0");
  uint64_t plan[8];
  expect(msm_amd_test_fr_gate_plan(canon, 0, good.get(), n, 2, 1, 3, plan) == bad &&
             msm_amd_test_fr_gate_plan(canon, 0, good.get(), n, 2, 1, 0, nullptr) == bad &&
             msm_amd_test_fr_gate_plan(canon, 4, good.get(), n, 2, 1, 0, plan) == bad,
         "plan arguments");
  if (failures) return 1;
  std::printf("gate_asan_check: ok\n");
  return 0;
}
