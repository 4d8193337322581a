// Host twins of the pairing calls (no ctx, no GPU) on host_fq12_64.h, threaded with host_threads.h over groups and over
// runs of pairs inside a group; the argument arithmetic the twins share with the host driver (calls_points.hip); the
// planner's test export and the host form of the raw-limb test ops.  The twin's ARITHMETIC is independent of the device
// path; its layout decoding is not: points are read with the loaders of the point calls (MulG1 / MulG2::load_base of
// mul_points.hip.h, the device's 29-bit code compiled for the host: any host layout -> canonical affine) and handed over
// in the external form both sides share.  A decoding error would be common to both; the tests' model encodes its own records.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "../../include/msm_amd.h"
#include "bn254_fq12_29.hip.h"
#include "host_fq12_64.h"
#include "host_pairing.h"
#include "host_threads.h"
#include "launch_pairing.h"
#include "mul_points.hip.h"

namespace msm_amd {

static_assert(MSM_AMD_GT_MONT_LE == kGtMontLe && MSM_AMD_GT_CANON_LE == kGtCanonLe && MSM_AMD_GT_BYTES == kGtBytes, "GT layouts");
static_assert(MSM_AMD_FQ12_WORDS == kFq12Words && MSM_AMD_FQ12_OP_FINAL_EXP + 1 == FQ12OP_COUNT, "raw fq12 ops");

bool pairing_gt_layout_known(int gt_layout) { return gt_layout == MSM_AMD_GT_MONT_LE || gt_layout == MSM_AMD_GT_CANON_LE; }

const char* pairing_shape_error(uint64_t n_groups, uint64_t group_size, uint32_t flags, int gt_layout, bool has_is_one) {
  if (flags & ~(uint32_t)MSM_AMD_PAIRING_MILLER_ONLY) return "unknown flags (MSM_AMD_PAIRING_MILLER_ONLY)";
  if (!pairing_gt_layout_known(gt_layout)) return "gt_layout must be MSM_AMD_GT_MONT_LE or MSM_AMD_GT_CANON_LE";
  if ((flags & MSM_AMD_PAIRING_MILLER_ONLY) && has_is_one) return "is_one must be NULL with MSM_AMD_PAIRING_MILLER_ONLY";
  if (n_groups > 0xFFFFFFFFull || group_size > 0xFFFFFFFFull || n_groups * group_size > 0xFFFFFFFFull)
    return "n_groups * group_size >= 2^32";
  return nullptr;
}

void pairing_knobs(uint32_t* pairs_per_lane, uint64_t* device_final_from, bool* f_in_lds) {
  *pairs_per_lane = 0;
  *device_final_from = kPairingDeviceFinalFrom;
  *f_in_lds = kPairingFInLds;
  if (const char* e = std::getenv("MSM_AMD_PAIRING_F_IN_LDS")) *f_in_lds = std::atoi(e) != 0;
  if (const char* e = std::getenv("MSM_AMD_PAIRING_PAIRS_PER_LANE")) *pairs_per_lane = (uint32_t)std::max(1, std::atoi(e));
  if (const char* e = std::getenv("MSM_AMD_PAIRING_DEVICE_FINAL_FROM")) *device_final_from = std::strtoull(e, nullptr, 10);
}

namespace {

h64::Fe fe_of(const fe29& canonical_internal) {
  const u256 x = Fq29::to_ext(canonical_internal);
  h64::Fe r;
  std::memcpy(&r, &x, sizeof r);
  return r;
}

// the pair of one record index, false when either point is the identity
bool load_pair(int l1, size_t s1, const uint8_t* g1, int l2, size_t s2, const uint8_t* g2, size_t rec, h64::Pair64* out) {
  const AffI p = MulG1::load_base(l1, g1 + rec * s1);
  const Aff2I q = MulG2::load_base(l2, g2 + rec * s2);
  if (MulG1::aff_is_identity(p) || MulG2::aff_is_identity(q)) return false;
  out->xp = fe_of(p.x);
  out->yp = fe_of(p.y);
  out->qx = h64::Fe2{fe_of(q.x.c0), fe_of(q.x.c1)};
  out->qy = h64::Fe2{fe_of(q.y.c0), fe_of(q.y.c1)};
  return true;
}

}  // namespace

void host_final_exponentiation(int gt_layout, const uint8_t* in, size_t n, int threads, uint8_t* out, uint8_t* is_one) {
  for_ranges(worker_count(threads, n), n, [&](unsigned, size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; ++i) {
      const h64::Fe12 e = h64::final_exp12(h64::gt_from_record64(in + i * kGtBytes, gt_layout));
      h64::gt_to_record64(out + i * kGtBytes, e, gt_layout);
      if (is_one) is_one[i] = h64::is_one12(e) ? 1 : 0;
    }
  });
}

}  // namespace msm_amd

extern "C" {

int msm_amd_host_pairing_product(int point_layout, int g2_point_layout, const void* g1_points, const void* g2_points,
                                 size_t n_groups, size_t group_size, uint32_t flags, int gt_layout, void* out_gt,
                                 uint8_t* is_one, int threads) {
  using namespace msm_amd;
  const size_t s1 = point_record_bytes(false, point_layout, kKindHost), s2 = point_record_bytes(true, g2_point_layout, kKindHost);
  if (s1 == 0 || s2 == 0 || pairing_shape_error(n_groups, group_size, flags, gt_layout, is_one != nullptr))
    return MSM_AMD_INPUT_ERROR;
  if (n_groups == 0) return MSM_AMD_OK;
  if (!out_gt || (group_size > 0 && (!g1_points || !g2_points))) return MSM_AMD_INPUT_ERROR;
  const uint8_t *g1 = (const uint8_t*)g1_points, *g2 = (const uint8_t*)g2_points;
  // runs of at most `run` pairs of one group: about four runs per thread over the whole call, f squared once per run
  const unsigned T = worker_count(threads, std::max<size_t>(1, n_groups * group_size));
  const size_t run = std::max<size_t>(1, (n_groups * group_size + 4 * (size_t)T - 1) / (4 * (size_t)T));
  const size_t runs_per_group = std::max<size_t>(1, (group_size + run - 1) / run);
  std::vector<h64::Fe12> partial(n_groups * runs_per_group);
  for_ranges(worker_count(threads, partial.size()), partial.size(), [&](unsigned, size_t lo, size_t hi) {
    std::vector<h64::Pair64> pairs;
    for (size_t w = lo; w < hi; ++w) {
      const size_t g = w / runs_per_group, first = (w % runs_per_group) * run;
      const size_t last = std::min(group_size, first + run);
      pairs.clear();
      for (size_t i = first; i < last; ++i) {
        h64::Pair64 p;
        if (load_pair(point_layout, s1, g1, g2_point_layout, s2, g2, g * group_size + i, &p)) pairs.push_back(p);
      }
      partial[w] = h64::miller_product64(pairs.data(), pairs.size());
    }
  });
  const bool miller_only = (flags & MSM_AMD_PAIRING_MILLER_ONLY) != 0;
  for_ranges(worker_count(threads, n_groups), n_groups, [&](unsigned, size_t lo, size_t hi) {
    for (size_t g = lo; g < hi; ++g) {
      h64::Fe12 f = partial[g * runs_per_group];
      for (size_t k = 1; k < runs_per_group; ++k) f = h64::mul12(f, partial[g * runs_per_group + k]);
      if (!miller_only) f = h64::final_exp12(f);
      h64::gt_to_record64((uint8_t*)out_gt + g * kGtBytes, f, gt_layout);
      if (is_one) is_one[g] = h64::is_one12(f) ? 1 : 0;
    }
  });
  return MSM_AMD_OK;
}

int msm_amd_host_final_exponentiation(int gt_layout, const void* in, size_t n, void* out, uint8_t* is_one, int threads) {
  using namespace msm_amd;
  if (!pairing_gt_layout_known(gt_layout) || n > 0xFFFFFFFFull) return MSM_AMD_INPUT_ERROR;
  if (n == 0) return MSM_AMD_OK;
  if (!in || !out) return MSM_AMD_INPUT_ERROR;
  host_final_exponentiation(gt_layout, (const uint8_t*)in, n, threads, (uint8_t*)out, is_one);
  return MSM_AMD_OK;
}

int msm_amd_test_pairing_plan(size_t n_groups, size_t group_size, uint32_t pairs_per_lane, uint64_t device_final_from,
                              uint32_t out[4]) {
  using namespace msm_amd;
  if (!out || n_groups > 0xFFFFFFFFull || group_size > 0xFFFFFFFFull || n_groups * group_size > 0xFFFFFFFFull)
    return MSM_AMD_INPUT_ERROR;
  const PairingPlan p = pairing_plan(n_groups, group_size, pairs_per_lane, device_final_from);
  out[0] = p.pairs_per_lane;
  out[1] = p.lanes_per_group;
  out[2] = p.fold_levels;
  out[3] = p.final_on_device;
  return MSM_AMD_OK;
}

int msm_amd_test_fq12_ops_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t count) {
  using namespace msm_amd;
  if (op < 0 || op >= FQ12OP_COUNT || count > kTestFq12OpsMax) return MSM_AMD_INPUT_ERROR;
  if (count == 0) return MSM_AMD_OK;
  if (!a || !b || !out) return MSM_AMD_INPUT_ERROR;
  for (size_t i = 0; i < count; ++i) run_test_fq12_op(op, a + i * kFq12Words, b + i * kFq12Words, out + i * kFq12Words);
  return MSM_AMD_OK;
}

int msm_amd_test_fq12_op_host(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (!a || !b || !out) return MSM_AMD_INPUT_ERROR;
  return msm_amd_test_fq12_ops_host(op, a, b, out, 1);
}

}  // extern "C"
