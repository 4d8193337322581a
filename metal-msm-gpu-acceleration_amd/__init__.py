"""Python binding of libmsm_amd.so for tests and bench.py (ctypes over the C ABI of include/msm_amd.h).

The product is the C/HIP library; this module only loads it and mirrors the reference's entry-point
names (`mopro_msm::metal::msm::{gpu_msm_h2c, metal_msm, setup_metal_state, ...}`, src/metal/msm.rs) so
that tests read like the reference's own.  There is NO CPU fallback: if the library is missing or no
gfx950 device is present the calls raise.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_size_t, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# MSM_AMD_LIB points development A/B runs at another build of the same library; the default is the in-tree one
LIB_PATH = os.environ.get("MSM_AMD_LIB") or os.path.join(_HERE, "libmsm_amd.so")

(OK, DEVICE_NOT_FOUND, LIBRARY_ERROR, FUNCTION_ERROR, PIPELINE_ERROR, INPUT_ERROR, FILE_OPEN_ERROR,
 DESERIALIZATION_ERROR, INVALID_DATA) = range(9)
SCALAR_MONT_LE, SCALAR_CANON_LE, SCALAR_CANON_BE32 = 0, 1, 2
POINT_H2C_AFFINE, POINT_ARK_PROJECTIVE, POINT_ARK_AFFINE, POINT_JAC_BE32, POINT_PREPARED, POINT_TABLES = 0, 1, 2, 3, 4, 5
POINT_BYTES = {POINT_H2C_AFFINE: 64, POINT_ARK_PROJECTIVE: 96, POINT_ARK_AFFINE: 72, POINT_JAC_BE32: 96}
(OP_UINT_ADD, OP_UINT_SUB, OP_UINT_PROD, OP_UINT_SHL, OP_UINT_SHR, OP_FP_ADD, OP_FP_SUB, OP_FP_MUL, OP_FP_NEG,
 OP_FP_POW, OP_EC_ADD, OP_EC_MUL, OP_EC_MADD, OP_EC_DBL, OP_FP29_MUL, OP_FP29_SQR, OP_FP29_SUB_K4E30,
 OP_FP29_SUB_K8E30, OP_FP29_SUB_K8E31, OP_FP29_SUB_K16E30, OP_FP29_SUB_K16E31, OP_FP29_ROUNDTRIP, OP_EC29_MADD,
 OP_EC29_ADD, OP_EC29_MADD_CHAIN, OP_EC29_ADD_CHAIN, OP_EC29_MMADD, OP_H64_FP_MUL, OP_H64_FP_ADD, OP_H64_FP_SUB,
 OP_H64_EC_ADD, OP_H64_EC_DBL, OP_FP29_MUL_KARATSUBA, OP_FP29_LOCKSTEP_PAIR, OP_FP29_LOCKSTEP_MIX,
 OP_FP29_LOCKSTEP_TRIPLE, OP_FP29_MUL2_KARATSUBA, OP_H64_FP_INV, OP_H64_FP_INV_FERMAT) = range(39)
# raw-limb test ops (MSM_AMD_RAW_*): records of RAW_IN_WORDS u32 per operand, RAW_OUT_WORDS per result
(RAW_FE_MUL, RAW_FE_SQR, RAW_FE_MUL2, RAW_FE_SUB_K4E30, RAW_FE_SUB_K8E30, RAW_FE_SUB_K8E31, RAW_FE_SUB_K16E30,
 RAW_FE_SUB_K16E31, RAW_FE_NORM, RAW_FE_NEG, RAW_FE_NEG_WIDE, RAW_FE_CANONICAL, RAW_FE_TO_EXT, RAW_FE_PACK_UNPACK,
 RAW_FE_ZERO, RAW_PT_MADD, RAW_PT_MMADD, RAW_PT_ADD_NZ, RAW_PT_ADD, RAW_PT_DOUBLE) = range(20)
RAW_FE_MUL_WIDE, RAW_FE_SQR_WIDE, RAW_FE_MUL2_WIDE = range(32, 35)   # the point additions' wide-digit forms
RAW_FE_SQRT = 36   # the Fq root of the decompression kernels (35 stays unknown)
RAW_BASES_IN_PLACE = 40   # external records as accumulate gathers them in place: unpack, affine start, mixed addition
RAW_FE_MUL_SUB, RAW_FE_SQR_SUB = 44, 45   # mul_sub_np<K> / sqr_sub_np<K>: the lifted subtraction folded into the reduction
RAW_IN_WORDS, RAW_OUT_WORDS = 36, 40
# BN254 G2 (MSM_AMD_G2_*): point layouts, raw-limb test ops and their record widths
G2_POINT_H2C_AFFINE, G2_POINT_ARK_AFFINE, G2_POINT_PREPARED, G2_POINT_TABLES = 0, 1, 2, 3
G2_PREPARED_BYTES = 128
G2_POINT_BYTES = {G2_POINT_H2C_AFFINE: 128, G2_POINT_ARK_AFFINE: 136}
(G2_RAW_FQ2_MUL, G2_RAW_FQ2_SQR, G2_RAW_PT_MADD, G2_RAW_PT_MMADD, G2_RAW_PT_ADD_NZ, G2_RAW_PT_ADD,
 G2_RAW_PT_DOUBLE, G2_RAW_FQ2_INV, G2_RAW_PT_TO_AFFINE) = range(9)
G2_RAW_FQ2_SQRT = 10   # the Fq2 root of the G2 decompression (9 stays unknown)
G2_RAW_IN_WORDS, G2_RAW_OUT_WORDS = 72, 80
# point validation (MSM_AMD_POINT_VALID ..., MSM_AMD_CHECK_*)
POINT_VALID, POINT_NOT_REDUCED, POINT_NOT_ON_CURVE, POINT_NOT_IN_SUBGROUP = range(4)
CHECK_CURVE, CHECK_SUBGROUP = 1, 2
# compressed points (MSM_AMD_COMPRESSED_*, MSM_AMD_POINT_BAD_ENCODING)
COMPRESSED_ARK, COMPRESSED_PARITY = 0, 1
POINT_BAD_ENCODING = 4
# batch scalar multiplication (MSM_AMD_MUL_BASE_*)
MUL_BASE_EACH, MUL_BASE_ONE = 0, 1
# number-theoretic transform over Fr (MSM_AMD_NTT_ROOT_*, MSM_AMD_NTT_FORWARD / _INVERSE)
NTT_ROOT_ARK, NTT_ROOT_H2C = 0, 1
NTT_FORWARD, NTT_INVERSE = 0, 1
# vectors over Fr (MSM_AMD_FR_*)
FR_ADD, FR_SUB, FR_MUL, FR_SCALE, FR_AXPY, FR_MULSUB_SCALE = range(6)
FR_PREFIX_INCLUSIVE, FR_PREFIX_EXCLUSIVE = 0, 1
LOOKUP_STRICT, LOOKUP_COUNT_MISSING = 0, 1
GATE_ACCUMULATE = 1            # MSM_AMD_GATE_*: flags of msm_amd_fr_gate_eval
GATE_MAX_OFFSETS = 8
MEM_HOST, MEM_DEVICE = 0, 1    # MSM_AMD_MEM_*: where the buffers of msm_amd_fr_sort, _build_sorted and _permute_as lie
PERMUTE_ROWS, PERMUTE_HALO2 = 0, 1   # MSM_AMD_PERMUTE_*: the arrangement of A', S'
LOOKUP_NOT_FOUND = 0xFFFFFFFF
MLE_LOW, MLE_HIGH = 0, 1
WIDTH_UNSIGNED, WIDTH_SIGNED = 0, 1
SUMCHECK_PRODUCT, SUMCHECK_EQ_AB_C = 0, 1
MLE_CALL_BIND, MLE_CALL_EVAL, MLE_CALL_EQ_TABLE, MLE_CALL_ROUND = range(4)
SUMCHECK_MAX_TABLES, SUMCHECK_MAX_TERMS, SUMCHECK_MAX_FACTORS = 16, 16, 6
SUMCHECK_NO_OUTER = 0xFFFFFFFF
# pairings (MSM_AMD_GT_*, MSM_AMD_PAIRING_*, MSM_AMD_FQ12_OP_*)
GT_MONT_LE, GT_CANON_LE = 0, 1
GT_BYTES = 384
PAIRING_MILLER_ONLY = 1
(FQ12_OP_FQ6_MUL, FQ12_OP_MUL, FQ12_OP_SQR, FQ12_OP_CYCLO_SQR, FQ12_OP_LINE_MUL, FQ12_OP_FROB1, FQ12_OP_FROB2,
 FQ12_OP_FROB3, FQ12_OP_CONJ, FQ12_OP_INV, FQ12_OP_POW_X, FQ12_OP_DOUBLE_STEP, FQ12_OP_ADD_STEP,
 FQ12_OP_FINAL_EXP) = range(14)
FQ12_WORDS = 108


def op_is_point(op):
    return 10 <= op <= 13 or 22 <= op <= 26 or op in (OP_H64_EC_ADD, OP_H64_EC_DBL)

# every symbol include/msm_amd.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "msm_amd_init", "msm_amd_init_reusable", "msm_amd_get_global", "msm_amd_destroy", "msm_amd_strerror",
    "msm_amd_last_error", "msm_amd_set_window_size", "msm_amd_auto_window_size", "msm_amd_auto_window_size_lone", "msm_amd_gpu_msm_h2c",
    "msm_amd_gpu_msm_h2c_sync", "msm_amd_cpu_dispatch_below", "msm_amd_host_register", "msm_amd_host_unregister",
    "msm_amd_metal_msm_ark", "msm_amd_msm", "msm_amd_msm_batch", "msm_amd_msm_best", "msm_amd_gpu_with_cpu",
    "msm_amd_reference_split", "msm_amd_msm_device",
    "msm_amd_msm_batch_device", "msm_amd_submit_batch_device", "msm_amd_wait_batch", "msm_amd_device_alloc", "msm_amd_device_free", "msm_amd_copy_to_device",
    "msm_amd_copy_to_host", "msm_amd_stream", "msm_amd_synchronize", "msm_amd_generate_instance",
    "msm_amd_prepare_buckets_indices", "msm_amd_sort_buckets_indices", "msm_amd_bucket_wise_accumulation",
    "msm_amd_sum_reduction", "msm_amd_final_accumulation", "msm_amd_test_op", "msm_amd_test_op_host",
    "msm_amd_test_op_raw", "msm_amd_test_op_raw_host",
    "msm_amd_last_timings",
    "msm_amd_algorithmic_bytes", "msm_amd_version",
    "msm_amd_instances_save", "msm_amd_instances_open", "msm_amd_instances_count", "msm_amd_instances_size",
    "msm_amd_instances_read", "msm_amd_instances_close", "msm_amd_instances_default_path", "msm_amd_to_wire",
    "msm_amd_from_wire", "msm_amd_sort_pairs_device", "msm_amd_bases_upload", "msm_amd_bases_prepare_device",
    "msm_amd_msm_prepared", "msm_amd_sum_points", "msm_amd_tables_build", "msm_amd_tables_build_device",
    "msm_amd_tables_info", "msm_amd_tables_free", "msm_amd_msm_tables",
    "msm_amd_set_wait_timeout_ms", "msm_amd_set_bases_cache", "msm_amd_bases_cache_stats", "msm_amd_test_hold",
    "msm_amd_test_release", "msm_amd_msm_batch_multi", "msm_amd_msm_batch_multi_device", "msm_amd_msm_range_multi", "msm_amd_shard_range",
    "msm_amd_submit_batch_multi_device", "msm_amd_wait_batch_multi", "msm_amd_bases_cache_invalidate",
    "msm_amd_set_bases_cache_verify",
    "msm_amd_scalar_bytes", "msm_amd_point_bytes", "msm_amd_shard_owner",
    "msm_amd_shard_count", "msm_amd_ctx_device", "msm_amd_pin_thread_to_device", "msm_amd_gather_init",
    "msm_amd_gather_size", "msm_amd_gather_all", "msm_amd_gather_last_error", "msm_amd_gather_destroy",
    "msm_amd_host_msm", "msm_amd_tuned_split", "msm_amd_host_threads", "msm_amd_generate_instance_host", "msm_amd_test_op_ifma",
    "msm_amd_test_last_plan", "msm_amd_test_stage_copy", "msm_amd_test_fill_workspaces",
    "msm_amd_test_g2_last_plan", "msm_amd_test_g2_stage_copy",
    "msm_amd_g2_point_bytes", "msm_amd_msm_g2", "msm_amd_msm_g2_device", "msm_amd_host_msm_g2",
    "msm_amd_test_g2_progression", "msm_amd_test_op_g2", "msm_amd_test_op_g2_host",
    "msm_amd_g2_bases_upload", "msm_amd_g2_bases_prepare_device", "msm_amd_msm_g2_prepared",
    "msm_amd_g2_tables_build", "msm_amd_g2_tables_build_device", "msm_amd_g2_tables_info", "msm_amd_g2_tables_free",
    "msm_amd_msm_g2_tables", "msm_amd_test_g2_tables_read", "msm_amd_test_g2_table_host",
    "msm_amd_check_points", "msm_amd_check_points_device", "msm_amd_g2_check_points", "msm_amd_g2_check_points_device",
    "msm_amd_host_check_points", "msm_amd_host_g2_check_points",
    "msm_amd_compressed_bytes", "msm_amd_decompress_points", "msm_amd_decompress_points_device",
    "msm_amd_g2_decompress_points", "msm_amd_g2_decompress_points_device", "msm_amd_host_decompress_points",
    "msm_amd_host_g2_decompress_points", "msm_amd_compress_points", "msm_amd_compress_points_device",
    "msm_amd_g2_compress_points", "msm_amd_g2_compress_points_device", "msm_amd_host_compress_points",
    "msm_amd_host_g2_compress_points",
    "msm_amd_mul_points", "msm_amd_mul_points_device", "msm_amd_g2_mul_points", "msm_amd_g2_mul_points_device",
    "msm_amd_host_mul_points", "msm_amd_host_g2_mul_points", "msm_amd_test_mul_plan",
    "msm_amd_test_mul_stage", "msm_amd_test_mul_stage_host",
    "msm_amd_ntt_domain_build", "msm_amd_ntt_domain_info", "msm_amd_ntt_domain_free", "msm_amd_ntt", "msm_amd_ntt_device",
    "msm_amd_host_ntt",
    "msm_amd_test_ntt_plan", "msm_amd_test_ntt_slots", "msm_amd_test_ntt_passes", "msm_amd_test_host_ntt_levels",
    "msm_amd_test_ntt_twiddles",
    "msm_amd_ntt_points", "msm_amd_ntt_points_device", "msm_amd_host_ntt_points",
    "msm_amd_test_ntt_points_levels", "msm_amd_test_host_ntt_points_levels",
    "msm_amd_fr_map", "msm_amd_fr_map_device", "msm_amd_host_fr_map",
    "msm_amd_fr_batch_inverse", "msm_amd_fr_batch_inverse_device", "msm_amd_host_fr_batch_inverse",
    "msm_amd_fr_prefix_product", "msm_amd_fr_prefix_product_device", "msm_amd_host_fr_prefix_product",
    "msm_amd_test_fr_plan",
    "msm_amd_fr_poly_eval", "msm_amd_fr_poly_eval_device", "msm_amd_host_fr_poly_eval",
    "msm_amd_fr_poly_div_linear", "msm_amd_fr_poly_div_linear_device", "msm_amd_host_fr_poly_div_linear",
    "msm_amd_fr_lincomb", "msm_amd_fr_lincomb_device", "msm_amd_host_fr_lincomb",
    "msm_amd_fr_matrix_build", "msm_amd_fr_matrix_info", "msm_amd_fr_matrix_free", "msm_amd_fr_matvec",
    "msm_amd_fr_matvec_device", "msm_amd_host_fr_matvec", "msm_amd_test_fr_matrix_plan",
    "msm_amd_fr_mle_bind", "msm_amd_fr_mle_bind_device", "msm_amd_host_fr_mle_bind",
    "msm_amd_fr_mle_eval", "msm_amd_fr_mle_eval_device", "msm_amd_host_fr_mle_eval",
    "msm_amd_fr_eq_table", "msm_amd_fr_eq_table_device", "msm_amd_host_fr_eq_table",
    "msm_amd_fr_sumcheck_round", "msm_amd_fr_sumcheck_round_device", "msm_amd_host_fr_sumcheck_round",
    "msm_amd_test_fr_mle_plan",
    "msm_amd_fr_sumcheck_terms_degree", "msm_amd_fr_sumcheck_round_terms",
    "msm_amd_host_fr_sumcheck_round_terms", "msm_amd_fr_sumcheck_step_terms",
    "msm_amd_host_fr_sumcheck_step_terms", "msm_amd_test_fr_sumcheck_terms_plan",
    "msm_amd_scalar_width", "msm_amd_scalar_width_device", "msm_amd_host_scalar_width",
    "msm_amd_msm_bounded", "msm_amd_msm_bounded_device", "msm_amd_msm_batch_bounded_device",
    "msm_amd_submit_batch_bounded_device", "msm_amd_msm_g2_bounded", "msm_amd_msm_g2_bounded_device",
    "msm_amd_host_msm_bounded", "msm_amd_host_msm_g2_bounded", "msm_amd_auto_window_size_bounded",
    "msm_amd_poseidon_constants", "msm_amd_poseidon_params_build", "msm_amd_poseidon_params_info",
    "msm_amd_poseidon_params_free", "msm_amd_poseidon_permute", "msm_amd_poseidon_permute_device",
    "msm_amd_host_poseidon_permute", "msm_amd_poseidon_hash", "msm_amd_poseidon_hash_device", "msm_amd_host_poseidon_hash",
    "msm_amd_poseidon_merkle_build", "msm_amd_poseidon_merkle_build_device", "msm_amd_host_poseidon_merkle_build",
    "msm_amd_poseidon_merkle_paths", "msm_amd_poseidon_merkle_paths_device", "msm_amd_host_poseidon_merkle_paths",
    "msm_amd_test_poseidon_plan",
    "msm_amd_pairing_product", "msm_amd_pairing_product_device", "msm_amd_host_pairing_product",
    "msm_amd_final_exponentiation", "msm_amd_final_exponentiation_device", "msm_amd_host_final_exponentiation",
    "msm_amd_test_pairing_plan", "msm_amd_test_fq12_op", "msm_amd_test_fq12_op_host", "msm_amd_test_fq12_ops",
    "msm_amd_test_fq12_ops_host",
    "msm_amd_fr_prefix_sum", "msm_amd_fr_prefix_sum_device", "msm_amd_host_fr_prefix_sum",
    "msm_amd_fr_shift", "msm_amd_fr_shift_device", "msm_amd_host_fr_shift",
    "msm_amd_fr_lookup_build", "msm_amd_fr_lookup_build_device", "msm_amd_fr_lookup_info", "msm_amd_fr_lookup_free",
    "msm_amd_fr_lookup_multiplicities", "msm_amd_fr_lookup_multiplicities_device", "msm_amd_host_fr_lookup_multiplicities",
    "msm_amd_test_fr_lookup_plan",
    "msm_amd_fr_lookup_permute", "msm_amd_host_fr_lookup_permute", "msm_amd_test_fr_permute_plan",
    "msm_amd_fr_sort", "msm_amd_host_fr_sort", "msm_amd_test_fr_sort_plan",
    "msm_amd_fr_lookup_build_sorted", "msm_amd_fr_lookup_sorted", "msm_amd_test_fr_lookup_image",
    "msm_amd_fr_lookup_permute_as", "msm_amd_host_fr_lookup_permute_as",
    "msm_amd_fr_poly_eval_points", "msm_amd_fr_poly_div_points", "msm_amd_host_fr_poly_eval_points",
    "msm_amd_host_fr_poly_div_points", "msm_amd_test_fr_poly_points_plan",
    "msm_amd_fr_gate_check", "msm_amd_fr_gate_last_error", "msm_amd_fr_gate_eval", "msm_amd_host_fr_gate_eval",
    "msm_amd_test_fr_gate_plan",
]

# stage tap (msm_amd_test_last_plan: word order of MSM_AMD_TP_*; msm_amd_test_stage_copy: MSM_AMD_STAGE_*)
TEST_PLAN_FIELDS = ("c", "W", "W_digits", "n", "n_scalars", "lb", "nb", "CH", "hb", "mb", "fb", "Q", "tiled", "ballot",
                    "wide_digits", "lone", "total_items", "multi_count", "deferred", "red_group", "rb_threads",
                    "instances", "workspace", "front_threads", "fused_front", "packed")
(STAGE_DIGITS, STAGE_SORTED, STAGE_BUCKET_SIZE, STAGE_BUCKET_START, STAGE_ITEM_START, STAGE_WIN_ITEMS, STAGE_ORDER,
 STAGE_MULTI_LIST, STAGE_BUCKETS, STAGE_PARTIAL) = range(10)


AFTER_SORT_FN = ctypes.CFUNCTYPE(None, c_void_p)   # msm_amd_after_sort_fn


class Timings(ctypes.Structure):
    _fields_ = [("convert_ms", c_float), ("digits_ms", c_float), ("sort_ms", c_float), ("accumulate_ms", c_float),
                ("reduce_ms", c_float), ("final_ms", c_float), ("total_gpu_ms", c_float), ("n", c_uint32),
                ("window_size", c_uint32), ("num_windows", c_uint32), ("reserved", c_uint32),
                ("accumulate_kernel_ms", c_float), ("reserved2", c_float * 3)]


class CheckReport(ctypes.Structure):   # msm_amd_check_report
    _fields_ = [("n_checked", c_uint64), ("n_invalid", c_uint64), ("n_identity", c_uint64), ("first_invalid", c_uint64),
                ("first_reason", c_uint32), ("by_reason", c_uint32 * 4), ("device_ms", c_float)]

    def as_dict(self) -> dict:
        """first_invalid is None when every record is valid (UINT64_MAX in the C struct)."""
        first = None if self.first_invalid == 0xFFFFFFFFFFFFFFFF else self.first_invalid
        return {"n_checked": self.n_checked, "n_invalid": self.n_invalid, "n_identity": self.n_identity,
                "first_invalid": first, "first_reason": self.first_reason, "by_reason": list(self.by_reason),
                "device_ms": self.device_ms}


class DecompressReport(ctypes.Structure):   # msm_amd_decompress_report
    _fields_ = [("n_checked", c_uint64), ("n_invalid", c_uint64), ("n_identity", c_uint64), ("first_invalid", c_uint64),
                ("first_reason", c_uint32), ("by_reason", c_uint32 * 5), ("device_ms", c_float)]
    as_dict = CheckReport.as_dict


class MsmError(RuntimeError):
    """Counterpart of MetalError (src/metal/abstraction/errors.rs:4-19)."""

    def __init__(self, status, detail=""):
        self.status = status
        super().__init__(f"msm_amd status {status}: {_lib().msm_amd_strerror(status).decode()} {detail}")


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = ctypes.CDLL(LIB_PATH)
        L.msm_amd_strerror.restype = c_char_p
        L.msm_amd_strerror.argtypes = [c_int]
        L.msm_amd_last_error.restype = c_char_p
        L.msm_amd_last_error.argtypes = [c_void_p]
        L.msm_amd_version.restype = c_char_p
        L.msm_amd_init.argtypes = [c_int, POINTER(c_void_p)]
        L.msm_amd_bases_upload.argtypes = [c_void_p, c_int, c_void_p, c_size_t, POINTER(c_void_p)]
        L.msm_amd_bases_prepare_device.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_void_p]
        L.msm_amd_msm_prepared.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
        L.msm_amd_tables_build.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_uint32, POINTER(c_void_p)]
        L.msm_amd_tables_build_device.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_uint32, POINTER(c_void_p)]
        L.msm_amd_tables_info.argtypes = [c_void_p, c_void_p, POINTER(c_size_t), POINTER(c_uint32), POINTER(c_uint32),
                                          POINTER(c_size_t)]
        L.msm_amd_tables_free.argtypes = [c_void_p, c_void_p]
        L.msm_amd_msm_tables.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
        L.msm_amd_sum_points.argtypes = [c_void_p, c_size_t, c_void_p]
        L.msm_amd_sort_pairs_device.argtypes = [c_void_p, c_void_p, c_size_t, c_uint32, POINTER(c_float)]
        L.msm_amd_instances_save.argtypes = [c_char_p, c_size_t, POINTER(c_size_t), POINTER(c_void_p),
                                             POINTER(c_void_p)]
        L.msm_amd_instances_open.argtypes = [c_char_p, POINTER(c_void_p)]
        L.msm_amd_instances_count.argtypes = [c_void_p]
        L.msm_amd_instances_count.restype = c_size_t
        L.msm_amd_instances_size.argtypes = [c_void_p, c_size_t]
        L.msm_amd_instances_size.restype = c_size_t
        L.msm_amd_instances_read.argtypes = [c_void_p, c_size_t, c_void_p, c_void_p]
        L.msm_amd_instances_close.argtypes = [c_void_p]
        L.msm_amd_instances_close.restype = None
        L.msm_amd_instances_default_path.argtypes = [c_char_p, c_uint32, c_uint32, c_char_p, c_size_t]
        L.msm_amd_instances_default_path.restype = c_size_t
        L.msm_amd_to_wire.argtypes = [c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
        L.msm_amd_from_wire.argtypes = [c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
        L.msm_amd_init_reusable.argtypes = [POINTER(c_void_p)]
        L.msm_amd_get_global.argtypes = [POINTER(c_void_p)]
        L.msm_amd_destroy.argtypes = [c_void_p]
        L.msm_amd_destroy.restype = None
        L.msm_amd_set_window_size.argtypes = [c_void_p, c_uint32]
        L.msm_amd_auto_window_size.argtypes = [c_size_t]
        L.msm_amd_auto_window_size.restype = c_uint32
        L.msm_amd_auto_window_size_lone.argtypes = [c_size_t]
        L.msm_amd_auto_window_size_lone.restype = c_uint32
        L.msm_amd_gpu_msm_h2c.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
        L.msm_amd_metal_msm_ark.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
        L.msm_amd_gpu_msm_h2c_sync.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, AFTER_SORT_FN, c_void_p, c_void_p]
        L.msm_amd_host_register.argtypes = [c_void_p, c_void_p, c_size_t]
        L.msm_amd_host_unregister.argtypes = [c_void_p, c_void_p]
        L.msm_amd_cpu_dispatch_below.argtypes = []
        L.msm_amd_cpu_dispatch_below.restype = c_size_t
        L.msm_amd_msm.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
        L.msm_amd_msm_batch.argtypes = [c_void_p, c_int, c_int, c_size_t, POINTER(c_void_p), POINTER(c_void_p),
                                        POINTER(c_size_t), c_void_p]
        L.msm_amd_msm_best.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
        L.msm_amd_gpu_with_cpu.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_int, c_void_p]
        L.msm_amd_reference_split.argtypes = [c_size_t]
        L.msm_amd_reference_split.restype = c_size_t
        L.msm_amd_msm_device.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
        L.msm_amd_msm_batch_device.argtypes = [c_void_p, c_int, c_int, c_size_t, POINTER(c_void_p),
                                               POINTER(c_void_p), POINTER(c_size_t), c_void_p]
        L.msm_amd_submit_batch_device.argtypes = [c_void_p, c_int, c_int, c_size_t, POINTER(c_void_p),
                                                  POINTER(c_void_p), POINTER(c_size_t), c_void_p, POINTER(c_int)]
        L.msm_amd_wait_batch.argtypes = [c_void_p, c_int]
        L.msm_amd_device_alloc.argtypes = [c_void_p, c_size_t, POINTER(c_void_p)]
        L.msm_amd_device_free.argtypes = [c_void_p, c_void_p]
        L.msm_amd_copy_to_device.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t]
        L.msm_amd_copy_to_host.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t]
        L.msm_amd_stream.argtypes = [c_void_p]
        L.msm_amd_stream.restype = c_void_p
        L.msm_amd_synchronize.argtypes = [c_void_p]
        L.msm_amd_generate_instance.argtypes = [c_void_p, c_uint64, c_size_t, c_int, c_void_p, c_void_p]
        L.msm_amd_prepare_buckets_indices.argtypes = [c_void_p, c_void_p, c_size_t, c_uint32, c_uint32, c_void_p]
        L.msm_amd_sort_buckets_indices.argtypes = [c_void_p, c_void_p, c_size_t]
        L.msm_amd_bucket_wise_accumulation.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_uint32,
                                                       c_void_p]
        L.msm_amd_sum_reduction.argtypes = [c_void_p, c_void_p, c_uint32, c_uint32, c_void_p]
        L.msm_amd_final_accumulation.argtypes = [c_void_p, c_uint32, c_uint32, c_void_p]
        L.msm_amd_test_op.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t]
        L.msm_amd_test_op_host.argtypes = [c_int, c_void_p, c_void_p, c_void_p, c_size_t]
        L.msm_amd_test_op_raw.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t]
        L.msm_amd_test_op_raw_host.argtypes = [c_int, c_void_p, c_void_p, c_void_p, c_size_t]
        L.msm_amd_last_timings.argtypes = [c_void_p, POINTER(Timings)]
        L.msm_amd_algorithmic_bytes.argtypes = [c_size_t, c_uint32, c_int]
        L.msm_amd_algorithmic_bytes.restype = c_uint64
        L.msm_amd_set_wait_timeout_ms.argtypes = [c_void_p, c_uint32]
        L.msm_amd_set_bases_cache.argtypes = [c_void_p, c_size_t]
        L.msm_amd_bases_cache_stats.argtypes = [c_void_p, POINTER(c_uint64)]
        L.msm_amd_bases_cache_invalidate.argtypes = [c_void_p, c_void_p]
        L.msm_amd_set_bases_cache_verify.argtypes = [c_void_p, c_int]
        L.msm_amd_test_hold.argtypes = [c_void_p, c_uint32, POINTER(c_void_p)]
        L.msm_amd_test_release.argtypes = [c_void_p, c_void_p]
        L.msm_amd_test_last_plan.argtypes = [c_void_p, c_uint32, c_void_p, c_size_t]
        L.msm_amd_test_stage_copy.argtypes = [c_void_p, c_uint32, c_int, c_void_p, POINTER(c_size_t)]
        L.msm_amd_test_fill_workspaces.argtypes = [c_void_p, ctypes.c_uint8]
        L.msm_amd_test_g2_last_plan.argtypes = [c_void_p, c_void_p, c_size_t]
        L.msm_amd_test_g2_stage_copy.argtypes = [c_void_p, c_int, c_void_p, POINTER(c_size_t)]
        L.msm_amd_msm_batch_multi.argtypes = [POINTER(c_void_p), c_size_t, c_int, c_int, c_size_t, POINTER(c_void_p),
                                              POINTER(c_void_p), POINTER(c_size_t), c_void_p]
        L.msm_amd_msm_batch_multi_device.argtypes = L.msm_amd_msm_batch_multi.argtypes
        L.msm_amd_submit_batch_multi_device.argtypes = L.msm_amd_msm_batch_multi.argtypes + [POINTER(c_void_p)]
        L.msm_amd_wait_batch_multi.argtypes = [c_void_p]
        L.msm_amd_msm_range_multi.argtypes = [POINTER(c_void_p), c_size_t, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                              c_void_p]
        L.msm_amd_shard_range.argtypes = [c_size_t, c_size_t, c_size_t, POINTER(c_size_t), POINTER(c_size_t)]
        L.msm_amd_shard_range.restype = None
        L.msm_amd_scalar_bytes.argtypes = [c_int]
        L.msm_amd_scalar_bytes.restype = c_size_t
        L.msm_amd_point_bytes.argtypes = [c_int]
        L.msm_amd_point_bytes.restype = c_size_t
        L.msm_amd_shard_owner.argtypes = [c_size_t, c_size_t]
        L.msm_amd_shard_owner.restype = c_size_t
        L.msm_amd_shard_count.argtypes = [c_size_t, c_size_t, c_size_t]
        L.msm_amd_shard_count.restype = c_size_t
        L.msm_amd_ctx_device.argtypes = [c_void_p]
        L.msm_amd_pin_thread_to_device.argtypes = [c_int]
        L.msm_amd_gather_init.argtypes = [POINTER(c_int), c_int, POINTER(c_void_p)]
        L.msm_amd_gather_size.argtypes = [c_void_p]
        L.msm_amd_gather_all.argtypes = [c_void_p, POINTER(c_void_p), c_size_t, POINTER(c_void_p)]
        L.msm_amd_gather_last_error.argtypes = [c_void_p]
        L.msm_amd_gather_last_error.restype = c_char_p
        L.msm_amd_gather_destroy.argtypes = [c_void_p]
        L.msm_amd_gather_destroy.restype = None
        L.msm_amd_host_msm.argtypes = [c_int, c_int, c_void_p, c_void_p, c_size_t, c_int, c_void_p]
        L.msm_amd_g2_point_bytes.argtypes = [c_int]
        L.msm_amd_g2_point_bytes.restype = c_size_t
        L.msm_amd_msm_g2.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
        L.msm_amd_msm_g2_device.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
        L.msm_amd_host_msm_g2.argtypes = [c_int, c_int, c_void_p, c_void_p, c_size_t, c_int, c_void_p]
        L.msm_amd_test_g2_progression.argtypes = [c_void_p, c_void_p, c_size_t, c_int, c_void_p]
        L.msm_amd_test_op_g2.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t]
        L.msm_amd_test_op_g2_host.argtypes = [c_int, c_void_p, c_void_p, c_void_p, c_size_t]
        L.msm_amd_g2_bases_upload.argtypes = [c_void_p, c_int, c_void_p, c_size_t, POINTER(c_void_p)]
        L.msm_amd_g2_bases_prepare_device.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_void_p]
        L.msm_amd_msm_g2_prepared.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
        L.msm_amd_g2_tables_build.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_uint32, POINTER(c_void_p)]
        L.msm_amd_g2_tables_build_device.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_uint32, POINTER(c_void_p)]
        L.msm_amd_g2_tables_info.argtypes = [c_void_p, c_void_p, POINTER(c_size_t), POINTER(c_uint32),
                                             POINTER(c_uint32), POINTER(c_size_t)]
        L.msm_amd_g2_tables_free.argtypes = [c_void_p, c_void_p]
        L.msm_amd_msm_g2_tables.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
        L.msm_amd_test_g2_tables_read.argtypes = [c_void_p, c_void_p, c_uint32, c_size_t, c_size_t, c_void_p]
        L.msm_amd_test_g2_table_host.argtypes = [c_int, c_void_p, c_size_t, c_uint32, c_uint32, c_int, c_void_p]
        L.msm_amd_check_points.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_uint32, c_void_p, POINTER(CheckReport)]
        L.msm_amd_check_points_device.argtypes = L.msm_amd_check_points.argtypes
        L.msm_amd_g2_check_points.argtypes = L.msm_amd_check_points.argtypes
        L.msm_amd_g2_check_points_device.argtypes = L.msm_amd_check_points.argtypes
        L.msm_amd_host_check_points.argtypes = [c_int, c_void_p, c_size_t, c_uint32, c_int, c_void_p, POINTER(CheckReport)]
        L.msm_amd_host_g2_check_points.argtypes = L.msm_amd_host_check_points.argtypes
        L.msm_amd_compressed_bytes.argtypes = [c_int, c_int]
        L.msm_amd_compressed_bytes.restype = c_size_t
        for name in ("msm_amd_decompress_points", "msm_amd_decompress_points_device", "msm_amd_g2_decompress_points",
                     "msm_amd_g2_decompress_points_device"):
            getattr(L, name).argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_int, c_void_p, c_void_p,
                                         POINTER(DecompressReport)]
        for name in ("msm_amd_host_decompress_points", "msm_amd_host_g2_decompress_points"):
            getattr(L, name).argtypes = [c_int, c_void_p, c_size_t, c_int, c_int, c_void_p, c_void_p,
                                         POINTER(DecompressReport)]
        for name in ("msm_amd_compress_points", "msm_amd_compress_points_device", "msm_amd_g2_compress_points",
                     "msm_amd_g2_compress_points_device"):
            getattr(L, name).argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_int, c_void_p, POINTER(c_uint64)]
        for name in ("msm_amd_host_compress_points", "msm_amd_host_g2_compress_points"):
            getattr(L, name).argtypes = [c_int, c_void_p, c_size_t, c_int, c_int, c_void_p, POINTER(c_uint64)]
        for name in ("msm_amd_mul_points", "msm_amd_mul_points_device", "msm_amd_g2_mul_points",
                     "msm_amd_g2_mul_points_device"):
            getattr(L, name).argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_int, c_void_p]
        for name in ("msm_amd_host_mul_points", "msm_amd_host_g2_mul_points"):
            getattr(L, name).argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p]
        L.msm_amd_test_mul_plan.argtypes = [c_int, POINTER(c_uint32)]
        L.msm_amd_test_mul_stage.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
        L.msm_amd_test_mul_stage_host.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
        L.msm_amd_ntt_domain_build.argtypes = [c_void_p, c_int, c_uint32, POINTER(c_void_p)]
        L.msm_amd_ntt_domain_info.argtypes = [c_void_p, c_void_p, POINTER(c_int), POINTER(c_uint32), POINTER(c_size_t),
                                              c_void_p]
        L.msm_amd_ntt_domain_free.argtypes = [c_void_p, c_void_p]
        L.msm_amd_ntt.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t]
        L.msm_amd_ntt_device.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                         POINTER(c_float)]
        L.msm_amd_host_ntt.argtypes = [c_int, c_uint32, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_int]
        L.msm_amd_test_ntt_plan.argtypes = [c_uint32, c_uint32, POINTER(c_uint32)]
        L.msm_amd_test_ntt_slots.argtypes = [c_uint32, c_uint32, c_uint32, c_uint64, POINTER(c_uint64)]
        L.msm_amd_test_ntt_passes.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                              c_uint32]
        L.msm_amd_test_host_ntt_levels.argtypes = [c_int, c_uint32, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                                   c_uint32, c_int]
        L.msm_amd_test_ntt_twiddles.argtypes = [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]
        if hasattr(L, "msm_amd_ntt_points"):   # (an MSM_AMD_LIB build from before the point transform still loads)
            L.msm_amd_ntt_points.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]
            L.msm_amd_ntt_points_device.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p,
                                                    POINTER(c_float)]
            L.msm_amd_host_ntt_points.argtypes = [c_int, c_uint32, c_int, c_int, c_void_p, c_int, c_void_p, c_int]
            L.msm_amd_test_ntt_points_levels.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_uint32, c_int,
                                                         c_void_p]
            L.msm_amd_test_host_ntt_points_levels.argtypes = [c_int, c_uint32, c_int, c_int, c_void_p, c_uint32, c_int,
                                                              c_void_p, c_int]
        L.msm_amd_fr_map.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
        L.msm_amd_fr_map_device.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                            c_void_p, POINTER(c_float)]
        L.msm_amd_host_fr_map.argtypes = [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]
        L.msm_amd_fr_batch_inverse.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_void_p, POINTER(c_uint64)]
        L.msm_amd_fr_batch_inverse_device.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_void_p, POINTER(c_uint64),
                                                      POINTER(c_float)]
        L.msm_amd_host_fr_batch_inverse.argtypes = [c_int, c_void_p, c_size_t, c_int, c_void_p, POINTER(c_uint64)]
        L.msm_amd_fr_prefix_product.argtypes = [c_void_p, c_int, c_int, c_void_p, c_size_t, c_size_t, c_void_p]
        L.msm_amd_fr_prefix_product_device.argtypes = [c_void_p, c_int, c_int, c_void_p, c_size_t, c_size_t, c_void_p,
                                                       POINTER(c_float)]
        L.msm_amd_host_fr_prefix_product.argtypes = [c_int, c_int, c_void_p, c_size_t, c_size_t, c_int, c_void_p]
        L.msm_amd_test_fr_plan.argtypes = [c_size_t, c_size_t, c_uint32, POINTER(c_uint64)]
        L.msm_amd_fr_prefix_sum.argtypes = L.msm_amd_fr_prefix_product.argtypes
        L.msm_amd_fr_prefix_sum_device.argtypes = L.msm_amd_fr_prefix_product_device.argtypes
        L.msm_amd_host_fr_prefix_sum.argtypes = L.msm_amd_host_fr_prefix_product.argtypes
        L.msm_amd_fr_shift.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
        L.msm_amd_fr_shift_device.argtypes = L.msm_amd_fr_shift.argtypes + [POINTER(c_float)]
        L.msm_amd_host_fr_shift.argtypes = [c_int, c_void_p, c_void_p, c_size_t, c_int, c_void_p]
        L.msm_amd_fr_lookup_build.argtypes = [c_void_p, c_int, c_void_p, c_size_t, POINTER(c_void_p)]
        L.msm_amd_fr_lookup_build_device.argtypes = L.msm_amd_fr_lookup_build.argtypes + [POINTER(c_float)]
        L.msm_amd_fr_lookup_info.argtypes = [c_void_p, c_void_p] + [POINTER(c_size_t)] * 5
        L.msm_amd_fr_lookup_free.argtypes = [c_void_p, c_void_p]
        L.msm_amd_fr_lookup_multiplicities.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_size_t,
                                                       c_void_p, c_void_p, POINTER(c_uint64)]
        L.msm_amd_fr_lookup_multiplicities_device.argtypes = L.msm_amd_fr_lookup_multiplicities.argtypes + [POINTER(c_float)]
        L.msm_amd_host_fr_lookup_multiplicities.argtypes = [c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_size_t,
                                                            c_int, c_void_p, c_void_p, POINTER(c_uint64)]
        L.msm_amd_test_fr_lookup_plan.argtypes = [c_size_t, c_uint32, POINTER(c_uint64)]
        L.msm_amd_fr_lookup_permute.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p,
                                                POINTER(c_uint64)]
        L.msm_amd_host_fr_lookup_permute.argtypes = [c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, c_int, c_void_p,
                                                     c_void_p, POINTER(c_uint64)]
        L.msm_amd_test_fr_permute_plan.argtypes = [c_size_t, c_size_t, c_uint32, POINTER(c_uint64)]
        L.msm_amd_fr_sort.argtypes = [c_void_p, c_int, c_int, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p,
                                      POINTER(c_float)]
        L.msm_amd_host_fr_sort.argtypes = [c_int, c_void_p, c_size_t, c_size_t, c_int, c_void_p, c_void_p]
        L.msm_amd_test_fr_sort_plan.argtypes = [c_size_t, c_size_t, c_uint32, POINTER(c_uint64)]
        L.msm_amd_fr_lookup_build_sorted.argtypes = [c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, POINTER(c_void_p),
                                                     POINTER(c_float)]
        L.msm_amd_fr_lookup_sorted.argtypes = [c_void_p, c_void_p, POINTER(c_int)]
        L.msm_amd_test_fr_lookup_image.argtypes = [c_void_p, c_void_p, POINTER(c_void_p)]
        L.msm_amd_fr_lookup_permute_as.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_size_t,
                                                   c_void_p, c_void_p, POINTER(c_uint64), POINTER(c_float)]
        L.msm_amd_host_fr_lookup_permute_as.argtypes = [c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, c_int,
                                                        c_void_p, c_void_p, POINTER(c_uint64)]
        L.msm_amd_fr_poly_eval.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]
        L.msm_amd_fr_poly_eval_device.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p,
                                                  POINTER(c_float)]
        L.msm_amd_host_fr_poly_eval.argtypes = [c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_int, c_void_p]
        L.msm_amd_fr_poly_div_linear.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, c_void_p]
        L.msm_amd_fr_poly_div_linear_device.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p,
                                                        c_void_p, POINTER(c_float)]
        L.msm_amd_host_fr_poly_div_linear.argtypes = [c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_int, c_void_p,
                                                      c_void_p]
        L.msm_amd_fr_poly_eval_points.argtypes = [c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_size_t,
                                                  c_void_p, POINTER(c_float)]
        L.msm_amd_fr_poly_div_points.argtypes = [c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_size_t,
                                                 c_void_p, c_void_p, POINTER(c_float)]
        L.msm_amd_host_fr_poly_eval_points.argtypes = [c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, c_int,
                                                       c_void_p]
        L.msm_amd_host_fr_poly_div_points.argtypes = [c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, c_int,
                                                      c_void_p, c_void_p]
        L.msm_amd_test_fr_poly_points_plan.argtypes = [c_size_t, c_size_t, c_size_t, c_uint32, c_int, POINTER(c_uint64)]
        L.msm_amd_fr_lincomb.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]
        L.msm_amd_fr_lincomb_device.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p,
                                                POINTER(c_float)]
        L.msm_amd_host_fr_lincomb.argtypes = [c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_int, c_void_p]
        L.msm_amd_fr_matrix_build.argtypes = [c_void_p, c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p,
                                              POINTER(c_void_p)]
        L.msm_amd_fr_matrix_info.argtypes = [c_void_p, c_void_p] + [POINTER(c_size_t)] * 5
        L.msm_amd_fr_matrix_free.argtypes = [c_void_p, c_void_p]
        L.msm_amd_fr_matvec.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
        L.msm_amd_fr_matvec_device.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p, POINTER(c_float)]
        L.msm_amd_host_fr_matvec.argtypes = [c_int, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                             c_void_p]
        L.msm_amd_test_fr_matrix_plan.argtypes = [c_size_t, c_void_p, c_uint32, c_uint32, POINTER(c_uint64), c_void_p,
                                                  c_size_t]
        L.msm_amd_fr_mle_bind.argtypes = [c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, c_size_t,
                                          c_void_p]
        L.msm_amd_fr_mle_bind_device.argtypes = L.msm_amd_fr_mle_bind.argtypes + [POINTER(c_float)]
        L.msm_amd_host_fr_mle_bind.argtypes = [c_int, c_int, c_void_p, c_size_t, c_void_p, c_size_t, c_size_t, c_size_t, c_int,
                                               c_void_p]
        L.msm_amd_fr_mle_eval.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_void_p]
        L.msm_amd_fr_mle_eval_device.argtypes = L.msm_amd_fr_mle_eval.argtypes + [POINTER(c_float)]
        L.msm_amd_host_fr_mle_eval.argtypes = [c_int, c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t, c_int, c_void_p]
        L.msm_amd_fr_eq_table.argtypes = [c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]
        L.msm_amd_fr_eq_table_device.argtypes = L.msm_amd_fr_eq_table.argtypes + [POINTER(c_float)]
        L.msm_amd_host_fr_eq_table.argtypes = [c_int, c_int, c_void_p, c_size_t, c_int, c_void_p]
        L.msm_amd_fr_sumcheck_round.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, c_size_t, c_size_t,
                                                c_void_p]
        L.msm_amd_fr_sumcheck_round_device.argtypes = L.msm_amd_fr_sumcheck_round.argtypes + [POINTER(c_float)]
        L.msm_amd_host_fr_sumcheck_round.argtypes = [c_int, c_int, c_int, c_void_p, c_size_t, c_size_t, c_size_t, c_int,
                                                     c_void_p]
        L.msm_amd_test_fr_mle_plan.argtypes = [c_int, c_int, c_int, c_size_t, c_size_t, c_uint32, c_uint32, c_uint32,
                                               POINTER(c_uint64)]
        if hasattr(L, "msm_amd_fr_sumcheck_round_terms"):   # (an MSM_AMD_LIB build from before the term lists still loads)
            tp = c_void_p                                   # const msm_amd_fr_sumcheck_terms*
            L.msm_amd_fr_sumcheck_terms_degree.argtypes = [tp, c_size_t, POINTER(c_uint32)]
            L.msm_amd_fr_sumcheck_round_terms.argtypes = [c_void_p, c_int, c_int, c_int, tp, c_void_p, c_size_t, c_size_t, c_size_t,
                                                          c_void_p, POINTER(c_float)]
            L.msm_amd_host_fr_sumcheck_round_terms.argtypes = [c_int, c_int, tp, c_void_p, c_size_t, c_size_t, c_size_t, c_int,
                                                               c_void_p]
            L.msm_amd_fr_sumcheck_step_terms.argtypes = [c_void_p, c_int, c_int, c_int, tp, c_void_p, c_void_p, c_size_t, c_size_t,
                                                         c_size_t, c_void_p, c_void_p, POINTER(c_float)]
            L.msm_amd_host_fr_sumcheck_step_terms.argtypes = [c_int, c_int, tp, c_void_p, c_void_p, c_size_t, c_size_t, c_size_t,
                                                              c_int, c_void_p, c_void_p]
            L.msm_amd_test_fr_sumcheck_terms_plan.argtypes = [tp, c_size_t, c_size_t, c_uint32, c_int, POINTER(c_uint64)]
        if hasattr(L, "msm_amd_fr_gate_eval"):   # (an MSM_AMD_LIB build from before the gate polynomials still loads)
            tp = c_void_p                        # const msm_amd_fr_gate_terms*
            L.msm_amd_fr_gate_check.argtypes = [tp, c_size_t, c_size_t, c_uint64, POINTER(c_uint32), POINTER(c_uint32)]
            L.msm_amd_fr_gate_last_error.argtypes = []
            L.msm_amd_fr_gate_last_error.restype = c_char_p
            L.msm_amd_fr_gate_eval.argtypes = [c_void_p, c_int, c_int, c_uint32, tp, c_void_p, c_size_t, c_size_t, c_size_t,
                                               c_uint64, c_void_p, c_void_p, c_size_t, c_void_p, POINTER(c_float)]
            L.msm_amd_host_fr_gate_eval.argtypes = [c_int, c_uint32, tp, c_void_p, c_size_t, c_size_t, c_size_t, c_uint64,
                                                    c_void_p, c_void_p, c_size_t, c_int, c_void_p]
            L.msm_amd_test_fr_gate_plan.argtypes = [c_int, c_uint32, tp, c_size_t, c_size_t, c_uint64, c_size_t,
                                                    POINTER(c_uint64)]
        if hasattr(L, "msm_amd_poseidon_constants"):   # (an MSM_AMD_LIB build from before the Poseidon calls still loads)
            shape = [c_uint32, c_uint32, c_uint32, c_int, c_void_p, c_void_p]   # t, r_f, r_p, layout, ark, mds
            L.msm_amd_poseidon_constants.argtypes = shape
            L.msm_amd_poseidon_params_build.argtypes = [c_void_p] + shape + [c_void_p]
            L.msm_amd_poseidon_params_info.argtypes = [c_void_p, c_void_p] + [POINTER(c_uint32)] * 3 + [POINTER(c_size_t)]
            L.msm_amd_poseidon_params_free.argtypes = [c_void_p, c_void_p]
            L.msm_amd_poseidon_permute.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]
            L.msm_amd_poseidon_permute_device.argtypes = L.msm_amd_poseidon_permute.argtypes + [POINTER(c_float)]
            L.msm_amd_host_poseidon_permute.argtypes = shape + [c_void_p, c_size_t, c_int, c_void_p]
            L.msm_amd_poseidon_hash.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
            L.msm_amd_poseidon_hash_device.argtypes = L.msm_amd_poseidon_hash.argtypes + [POINTER(c_float)]
            L.msm_amd_host_poseidon_hash.argtypes = shape + [c_void_p, c_void_p, c_size_t, c_int, c_void_p]
            L.msm_amd_poseidon_merkle_build.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
            L.msm_amd_poseidon_merkle_build_device.argtypes = L.msm_amd_poseidon_merkle_build.argtypes + [POINTER(c_float)]
            L.msm_amd_host_poseidon_merkle_build.argtypes = shape + [c_void_p, c_void_p, c_size_t, c_int, c_void_p, c_void_p]
            L.msm_amd_poseidon_merkle_paths.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t,
                                                        c_void_p]
            L.msm_amd_poseidon_merkle_paths_device.argtypes = L.msm_amd_poseidon_merkle_paths.argtypes + [POINTER(c_float)]
            L.msm_amd_host_poseidon_merkle_paths.argtypes = [c_uint32, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_int,
                                                             c_void_p]
            L.msm_amd_test_poseidon_plan.argtypes = [c_uint32, c_size_t, c_uint32, POINTER(c_uint64)]
        if hasattr(L, "msm_amd_pairing_product"):   # (an MSM_AMD_LIB build from before the pairing calls still loads)
            shape = [c_int, c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_uint32, c_int, c_void_p, c_void_p]
            L.msm_amd_pairing_product.argtypes = [c_void_p] + shape
            L.msm_amd_pairing_product_device.argtypes = [c_void_p] + shape + [POINTER(c_float)]
            L.msm_amd_host_pairing_product.argtypes = shape + [c_int]
            L.msm_amd_final_exponentiation.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_void_p, c_void_p]
            L.msm_amd_final_exponentiation_device.argtypes = L.msm_amd_final_exponentiation.argtypes + [POINTER(c_float)]
            L.msm_amd_host_final_exponentiation.argtypes = [c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_int]
            L.msm_amd_test_pairing_plan.argtypes = [c_size_t, c_size_t, c_uint32, c_uint64, POINTER(c_uint32)]
            L.msm_amd_test_fq12_op.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p]
            L.msm_amd_test_fq12_op_host.argtypes = [c_int, c_void_p, c_void_p, c_void_p]
            L.msm_amd_test_fq12_ops.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t]
            L.msm_amd_test_fq12_ops_host.argtypes = [c_int, c_void_p, c_void_p, c_void_p, c_size_t]
        L.msm_amd_generate_instance_host.argtypes = [c_uint64, c_size_t, c_int, c_void_p, c_void_p, c_int]
        L.msm_amd_test_op_ifma.argtypes = [c_int, c_void_p, c_void_p, c_void_p, c_size_t]
        if hasattr(L, "msm_amd_scalar_width"):   # (an MSM_AMD_LIB build from before the bounded-width calls still loads)
            L.msm_amd_scalar_width.argtypes = [c_void_p, c_int, c_void_p, c_size_t, c_int, POINTER(c_uint32), POINTER(c_uint64)]
            L.msm_amd_scalar_width_device.argtypes = L.msm_amd_scalar_width.argtypes
            L.msm_amd_host_scalar_width.argtypes = [c_int, c_void_p, c_size_t, c_int, c_int, POINTER(c_uint32), POINTER(c_uint64)]
            L.msm_amd_msm_bounded.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_uint32, c_int, c_void_p]
            L.msm_amd_msm_bounded_device.argtypes = L.msm_amd_msm_bounded.argtypes
            L.msm_amd_msm_batch_bounded_device.argtypes = [c_void_p, c_int, c_int, c_size_t, c_void_p, c_void_p, c_void_p,
                                                           c_uint32, c_int, c_void_p]
            L.msm_amd_submit_batch_bounded_device.argtypes = L.msm_amd_msm_batch_bounded_device.argtypes + [POINTER(c_int)]
            L.msm_amd_msm_g2_bounded.argtypes = L.msm_amd_msm_bounded.argtypes
            L.msm_amd_msm_g2_bounded_device.argtypes = L.msm_amd_msm_bounded.argtypes
            L.msm_amd_host_msm_bounded.argtypes = [c_int, c_int, c_void_p, c_void_p, c_size_t, c_uint32, c_int, c_int, c_void_p]
            L.msm_amd_host_msm_g2_bounded.argtypes = L.msm_amd_host_msm_bounded.argtypes
            L.msm_amd_auto_window_size_bounded.argtypes = [c_size_t, c_uint32, c_int]
            L.msm_amd_auto_window_size_bounded.restype = c_uint32
        L.msm_amd_tuned_split.argtypes = [c_size_t]
        L.msm_amd_tuned_split.restype = c_size_t
        _LIB = L
    return _LIB


def lib():
    return _lib()


def _u32buf(seq):
    arr = (c_uint32 * len(seq))(*seq)
    return arr


class MsmConfig:
    """MetalMsmConfig (msm.rs:59-63): device + stream + kernels.  `setup_metal_state()` makes one."""

    def __init__(self, device=-1, _handle=None, _owned=True):
        self._owned = _owned
        if _handle is not None:
            self.h = _handle
            return
        h = c_void_p()
        st = _lib().msm_amd_init(device, ctypes.byref(h))
        if st != OK:
            raise MsmError(st)
        self.h = h

    def _check(self, st):
        if st != OK:
            raise MsmError(st, _lib().msm_amd_last_error(self.h).decode())

    def close(self):
        if self.h and self._owned:
            _lib().msm_amd_destroy(self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- whole MSM -------------------------------------------------------------------------
    def set_window_size(self, c):
        self._check(_lib().msm_amd_set_window_size(self.h, c))

    def msm(self, scalars: bytes, points: bytes, n: int, scalar_layout=SCALAR_MONT_LE,
            point_layout=POINT_H2C_AFFINE) -> bytes:
        out = ctypes.create_string_buffer(96)
        self._check(_lib().msm_amd_msm(self.h, scalar_layout, point_layout, scalars, points, n, out))
        return out.raw

    def msm_batch(self, scalars_list, points_list, ns, scalar_layout=SCALAR_MONT_LE,
                  point_layout=POINT_H2C_AFFINE):
        k = len(ns)
        sp = (c_void_p * k)(*[ctypes.cast(ctypes.c_char_p(s), c_void_p) for s in scalars_list])
        if point_layout in (POINT_PREPARED, POINT_TABLES):    # device pointers / table handles, not host bytes
            pp = (c_void_p * k)(*points_list)
        else:
            pp = (c_void_p * k)(*[ctypes.cast(ctypes.c_char_p(p), c_void_p) for p in points_list])
        nn = (c_size_t * k)(*ns)
        out = ctypes.create_string_buffer(96 * k)
        self._check(_lib().msm_amd_msm_batch(self.h, scalar_layout, point_layout, k, sp, pp, nn, out))
        return [out.raw[96 * i:96 * i + 96] for i in range(k)]

    def msm_batch_device(self, d_scalars, d_points, ns, scalar_layout=SCALAR_MONT_LE,
                         point_layout=POINT_H2C_AFFINE):
        k = len(ns)
        sp = (c_void_p * k)(*d_scalars)
        pp = (c_void_p * k)(*d_points)
        nn = (c_size_t * k)(*ns)
        out = ctypes.create_string_buffer(96 * k)
        self._check(_lib().msm_amd_msm_batch_device(self.h, scalar_layout, point_layout, k, sp, pp, nn, out))
        return [out.raw[96 * i:96 * i + 96] for i in range(k)]

    def submit_batch_device(self, d_scalars, d_points, ns, scalar_layout=SCALAR_MONT_LE,
                            point_layout=POINT_H2C_AFFINE):
        """Enqueue a batch; returns a handle for wait_batch (pipelined form of msm_batch_device)."""
        k = len(ns)
        sp = (c_void_p * k)(*d_scalars)
        pp = (c_void_p * k)(*d_points)
        nn = (c_size_t * k)(*ns)
        out = ctypes.create_string_buffer(96 * k)
        ticket = c_int(-1)
        self._check(_lib().msm_amd_submit_batch_device(self.h, scalar_layout, point_layout, k, sp, pp, nn, out,
                                                       ctypes.byref(ticket)))
        return (ticket.value, out, k)

    def wait_batch(self, handle):
        ticket, out, k = handle
        self._check(_lib().msm_amd_wait_batch(self.h, ticket))
        return [out.raw[96 * i:96 * i + 96] for i in range(k)]

    # ---- scalars of bounded width: magnitudes below 2^bits (WIDTH_SIGNED: min(s, r - s)).  A record beyond the bound
    # raises MsmError(INPUT_ERROR) after the GPU work and leaves `out` (a caller's ctypes buffer, optional) untouched.
    def scalar_width(self, scalars: bytes, n: int, sign=WIDTH_UNSIGNED, scalar_layout=SCALAR_MONT_LE):
        """(bits, {"zeros", "negatives", "widest"}) of n host scalars."""
        return _width_result(lambda b, st: self._check(
            _lib().msm_amd_scalar_width(self.h, scalar_layout, scalars, n, sign, b, st)))

    def scalar_width_device(self, d_scalars, n: int, sign=WIDTH_UNSIGNED, scalar_layout=SCALAR_MONT_LE):
        return _width_result(lambda b, st: self._check(
            _lib().msm_amd_scalar_width_device(self.h, scalar_layout, d_scalars, n, sign, b, st)))

    def msm_bounded(self, scalars: bytes, points, n: int, bits: int, sign=WIDTH_UNSIGNED, scalar_layout=SCALAR_MONT_LE,
                    point_layout=POINT_H2C_AFFINE, out=None) -> bytes:
        """points: host bytes, or the device pointer / table handle of POINT_PREPARED / POINT_TABLES."""
        out = ctypes.create_string_buffer(96) if out is None else out
        self._check(_lib().msm_amd_msm_bounded(self.h, scalar_layout, point_layout, scalars, points, n, bits, sign, out))
        return out.raw[:96]

    def msm_bounded_device(self, d_scalars, d_points, n: int, bits: int, sign=WIDTH_UNSIGNED, scalar_layout=SCALAR_MONT_LE,
                           point_layout=POINT_H2C_AFFINE, out=None) -> bytes:
        out = ctypes.create_string_buffer(96) if out is None else out
        self._check(_lib().msm_amd_msm_bounded_device(self.h, scalar_layout, point_layout, d_scalars, d_points, n, bits, sign,
                                                      out))
        return out.raw[:96]

    def msm_batch_bounded_device(self, d_scalars, d_points, ns, bits: int, sign=WIDTH_UNSIGNED,
                                 scalar_layout=SCALAR_MONT_LE, point_layout=POINT_H2C_AFFINE, out=None):
        k = len(ns)
        sp, pp, nn = (c_void_p * k)(*d_scalars), (c_void_p * k)(*d_points), (c_size_t * k)(*ns)
        out = ctypes.create_string_buffer(96 * k) if out is None else out
        self._check(_lib().msm_amd_msm_batch_bounded_device(self.h, scalar_layout, point_layout, k, sp, pp, nn, bits, sign, out))
        return [out.raw[96 * i:96 * i + 96] for i in range(k)]

    def submit_batch_bounded_device(self, d_scalars, d_points, ns, bits: int, sign=WIDTH_UNSIGNED,
                                    scalar_layout=SCALAR_MONT_LE, point_layout=POINT_H2C_AFFINE, out=None):
        """Returns a handle for wait_batch, which raises for a violated bound."""
        k = len(ns)
        sp, pp, nn = (c_void_p * k)(*d_scalars), (c_void_p * k)(*d_points), (c_size_t * k)(*ns)
        out = ctypes.create_string_buffer(96 * k) if out is None else out
        ticket = c_int(-1)
        self._check(_lib().msm_amd_submit_batch_bounded_device(self.h, scalar_layout, point_layout, k, sp, pp, nn, bits, sign,
                                                               out, ctypes.byref(ticket)))
        return (ticket.value, out, k)

    def msm_g2_bounded(self, scalars: bytes, points: bytes, n: int, bits: int, sign=WIDTH_UNSIGNED,
                       scalar_layout=SCALAR_MONT_LE, point_layout=G2_POINT_H2C_AFFINE, out=None) -> bytes:
        out = ctypes.create_string_buffer(192) if out is None else out
        self._check(_lib().msm_amd_msm_g2_bounded(self.h, scalar_layout, point_layout, scalars, points, n, bits, sign, out))
        return out.raw[:192]

    def msm_g2_bounded_device(self, d_scalars, d_points, n: int, bits: int, sign=WIDTH_UNSIGNED,
                              scalar_layout=SCALAR_MONT_LE, point_layout=G2_POINT_H2C_AFFINE, out=None) -> bytes:
        """d_points: device records, a prepared array (G2_POINT_PREPARED) or a table handle (G2_POINT_TABLES)."""
        out = ctypes.create_string_buffer(192) if out is None else out
        self._check(_lib().msm_amd_msm_g2_bounded_device(self.h, scalar_layout, point_layout, d_scalars, d_points, n, bits,
                                                         sign, out))
        return out.raw[:192]

    def set_wait_timeout_ms(self, ms: int):
        """Upper bound of every host wait for the GPU (0 = none); a wait that reaches it raises PIPELINE_ERROR."""
        self._check(_lib().msm_amd_set_wait_timeout_ms(self.h, ms))

    def set_bases_cache(self, max_bytes: int):
        """Opt-in cache of converted bases for the host-slice entry points (0 = off)."""
        self._check(_lib().msm_amd_set_bases_cache(self.h, max_bytes))

    def bases_cache_invalidate(self, data=None):
        """The caller's word that the points array `data` (a bytes object handed over earlier; None: every array)
        changed in place: its cache entries are dropped."""
        ptr = None if data is None else ctypes.cast(ctypes.c_char_p(data), c_void_p)
        self._check(_lib().msm_amd_bases_cache_invalidate(self.h, ptr))

    def set_bases_cache_verify(self, full: bool):
        self._check(_lib().msm_amd_set_bases_cache_verify(self.h, 1 if full else 0))

    def bases_cache_stats(self):
        st = (c_uint64 * 5)()
        self._check(_lib().msm_amd_bases_cache_stats(self.h, st))
        return {"hits": st[0], "misses": st[1], "invalidations": st[2], "bytes": st[3], "entries": st[4]}

    def test_hold(self, max_ms: int):
        h = c_void_p()
        self._check(_lib().msm_amd_test_hold(self.h, max_ms, ctypes.byref(h)))
        return h

    def test_release(self, handle):
        self._check(_lib().msm_amd_test_release(self.h, handle))

    def test_last_plan(self, j=0) -> dict:
        """Plan and plan counters of instance j of the batch this ctx last waited for (stage tap)."""
        out = (c_uint32 * len(TEST_PLAN_FIELDS))()
        self._check(_lib().msm_amd_test_last_plan(self.h, j, out, len(out)))
        return dict(zip(TEST_PLAN_FIELDS, out))

    def test_stage_copy(self, which, j=0) -> bytes:
        """One workspace buffer (STAGE_*) of instance j of the batch this ctx last waited for (stage tap)."""
        nbytes = c_size_t(0)
        self._check(_lib().msm_amd_test_stage_copy(self.h, j, which, None, ctypes.byref(nbytes)))
        out = ctypes.create_string_buffer(max(1, nbytes.value))
        self._check(_lib().msm_amd_test_stage_copy(self.h, j, which, out, ctypes.byref(nbytes)))
        return out.raw[:nbytes.value]

    def test_fill_workspaces(self, byte: int):
        """Fill the point-valued workspace buffers with one byte (stale-data tests)."""
        self._check(_lib().msm_amd_test_fill_workspaces(self.h, byte))

    def test_g2_last_plan(self) -> dict:
        """Plan and plan counters of the last G2 MSM of this ctx (stage tap)."""
        out = (c_uint32 * len(TEST_PLAN_FIELDS))()
        self._check(_lib().msm_amd_test_g2_last_plan(self.h, out, len(out)))
        return dict(zip(TEST_PLAN_FIELDS, out))

    def test_g2_stage_copy(self, which) -> bytes:
        """One buffer (STAGE_*) of the last G2 MSM of this ctx; buckets and partials as 192-byte Jacobian records."""
        nbytes = c_size_t(0)
        self._check(_lib().msm_amd_test_g2_stage_copy(self.h, which, None, ctypes.byref(nbytes)))
        out = ctypes.create_string_buffer(max(1, nbytes.value))
        self._check(_lib().msm_amd_test_g2_stage_copy(self.h, which, out, ctypes.byref(nbytes)))
        return out.raw[:nbytes.value]

    def device(self) -> int:
        return _lib().msm_amd_ctx_device(self.h)

    def host_register(self, data: bytes):
        """Page-lock the memory of a bytes object (keep it alive until host_unregister): DMA uploads."""
        addr = ctypes.cast(ctypes.c_char_p(data), c_void_p)
        self._check(_lib().msm_amd_host_register(self.h, addr, len(data)))

    def host_unregister(self, data: bytes):
        self._check(_lib().msm_amd_host_unregister(self.h, ctypes.cast(ctypes.c_char_p(data), c_void_p)))

    # ---- device memory ---------------------------------------------------------------------
    def alloc(self, nbytes) -> int:
        p = c_void_p()
        self._check(_lib().msm_amd_device_alloc(self.h, nbytes, ctypes.byref(p)))
        return p.value

    def free(self, dptr):
        self._check(_lib().msm_amd_device_free(self.h, c_void_p(dptr)))

    def to_device(self, dptr, data: bytes):
        self._check(_lib().msm_amd_copy_to_device(self.h, c_void_p(dptr), data, len(data)))

    def to_host(self, dptr, nbytes) -> bytes:
        out = ctypes.create_string_buffer(nbytes)
        self._check(_lib().msm_amd_copy_to_host(self.h, out, c_void_p(dptr), nbytes))
        return out.raw

    def generate_instance(self, seed, n, scalars_mont=True):
        """Device-resident synthetic instance: returns (d_points, d_scalars)."""
        dp = self.alloc(64 * n)
        ds = self.alloc(32 * n)
        self._check(_lib().msm_amd_generate_instance(self.h, seed, n, 1 if scalars_mont else 0, c_void_p(dp),
                                                     c_void_p(ds)))
        return dp, ds

    def stream(self) -> int:
        return _lib().msm_amd_stream(self.h)

    def synchronize(self):
        self._check(_lib().msm_amd_synchronize(self.h))

    def timings(self) -> Timings:
        t = Timings()
        self._check(_lib().msm_amd_last_timings(self.h, ctypes.byref(t)))
        return t

    # ---- stages (reference wire layout: lists of u32) ----------------------------------------
    def prepare_buckets_indices(self, scalars_be32, n, window_size, num_windows):
        out = (c_uint32 * (n * num_windows * 2))()
        self._check(_lib().msm_amd_prepare_buckets_indices(self.h, _u32buf(scalars_be32), n, window_size,
                                                           num_windows, out))
        return [(out[2 * i], out[2 * i + 1]) for i in range(n * num_windows)]

    def sort_buckets_indices(self, pairs):
        flat = [v for pr in pairs for v in pr]
        buf = _u32buf(flat)
        self._check(_lib().msm_amd_sort_buckets_indices(self.h, buf, len(pairs)))
        return [(buf[2 * i], buf[2 * i + 1]) for i in range(len(pairs))]

    # ---- persistent bases (the reference re-uploads them per call, msm.rs:152-153) -----------
    def bases_upload(self, points: bytes, n: int, point_layout=POINT_H2C_AFFINE) -> int:
        """Convert once, keep resident; returns a device pointer to pass with POINT_PREPARED (free with .free)."""
        p = c_void_p()
        self._check(_lib().msm_amd_bases_upload(self.h, point_layout, points, n, ctypes.byref(p)))
        return p.value

    def bases_prepare_device(self, d_points, n, point_layout=POINT_H2C_AFFINE) -> int:
        out = self.alloc(64 * n)
        self._check(_lib().msm_amd_bases_prepare_device(self.h, point_layout, c_void_p(d_points), n, c_void_p(out)))
        return out

    def msm_prepared(self, scalars: bytes, d_prepared, n, scalar_layout=SCALAR_MONT_LE) -> bytes:
        out = ctypes.create_string_buffer(96)
        self._check(_lib().msm_amd_msm_prepared(self.h, scalar_layout, scalars, c_void_p(d_prepared), n, out))
        return out.raw

    # ---- precomputed window tables for fixed bases (beyond the reference) --------
    def tables_build(self, points: bytes, n: int, point_layout=POINT_H2C_AFFINE, window_size=0) -> int:
        """Returns a table handle: pass it as the points pointer with POINT_TABLES, free with tables_free."""
        h = c_void_p()
        self._check(_lib().msm_amd_tables_build(self.h, point_layout, points, n, window_size, ctypes.byref(h)))
        return h.value

    def tables_build_device(self, d_points, n, point_layout=POINT_H2C_AFFINE, window_size=0) -> int:
        h = c_void_p()
        self._check(_lib().msm_amd_tables_build_device(self.h, point_layout, c_void_p(d_points), n, window_size,
                                                       ctypes.byref(h)))
        return h.value

    def tables_info(self, tables):
        n, nbytes, c, W = c_size_t(), c_size_t(), c_uint32(), c_uint32()
        self._check(_lib().msm_amd_tables_info(self.h, c_void_p(tables), ctypes.byref(n), ctypes.byref(c),
                                               ctypes.byref(W), ctypes.byref(nbytes)))
        return {"n": n.value, "window_size": c.value, "num_windows": W.value, "device_bytes": nbytes.value}

    def tables_free(self, tables):
        self._check(_lib().msm_amd_tables_free(self.h, c_void_p(tables)))

    def msm_tables(self, scalars: bytes, tables, scalar_layout=SCALAR_MONT_LE) -> bytes:
        out = ctypes.create_string_buffer(96)
        self._check(_lib().msm_amd_msm_tables(self.h, c_void_p(tables), scalar_layout, scalars, out))
        return out.raw

    def sort_pairs_device(self, d_pairs, n_pairs, key_bits=32) -> float:
        """In-place device sort of (key, value) u32 pairs; returns the device time in ms."""
        ms = c_float()
        self._check(_lib().msm_amd_sort_pairs_device(self.h, c_void_p(d_pairs), n_pairs, key_bits, ctypes.byref(ms)))
        return ms.value

    def bucket_wise_accumulation(self, sorted_pairs, points_be32, n_points, total_buckets):
        flat = [v for pr in sorted_pairs for v in pr]
        out = (c_uint32 * (total_buckets * 24))()
        self._check(_lib().msm_amd_bucket_wise_accumulation(self.h, _u32buf(flat) if flat else None,
                                                            len(sorted_pairs), _u32buf(points_be32), n_points,
                                                            total_buckets, out))
        return [list(out[24 * i:24 * i + 24]) for i in range(total_buckets)]

    def sum_reduction(self, buckets_be32, buckets_size, num_windows):
        out = (c_uint32 * (num_windows * 24))()
        self._check(_lib().msm_amd_sum_reduction(self.h, _u32buf(buckets_be32), buckets_size, num_windows, out))
        return [list(out[24 * i:24 * i + 24]) for i in range(num_windows)]

    def test_op(self, op, a, b, count):
        per = 24 if op_is_point(op) else 8
        out = (c_uint32 * (count * per))()
        self._check(_lib().msm_amd_test_op(self.h, op, _u32buf(a), _u32buf(b), out, count))
        return list(out)

    def test_op_raw(self, op, a, b, count):
        """Raw-limb op (MSM_AMD_RAW_*) on the device: a, b flat u32 lists of count * RAW_IN_WORDS; returns
        count * RAW_OUT_WORDS u32."""
        out = (c_uint32 * (count * RAW_OUT_WORDS))()
        self._check(_lib().msm_amd_test_op_raw(self.h, op, _raw_in(a, count), _raw_in(b, count), out, count))
        return list(out)


    # ---- BN254 G2 --------------------------------------------------------------------------------
    def msm_g2(self, scalars: bytes, points: bytes, n: int, scalar_layout=SCALAR_MONT_LE,
               point_layout=G2_POINT_H2C_AFFINE) -> bytes:
        """One blocking G2 MSM on the GPU from host buffers: 192-byte normalised Jacobian (Montgomery LE)."""
        out = ctypes.create_string_buffer(192)
        self._check(_lib().msm_amd_msm_g2(self.h, scalar_layout, point_layout, scalars, points, n, out))
        return out.raw

    def msm_g2_device(self, d_scalars, d_points, n: int, scalar_layout=SCALAR_MONT_LE,
                      point_layout=G2_POINT_H2C_AFFINE) -> bytes:
        """msm_g2 with scalars and points already in device memory (pointers from alloc / to_device); d_points may
        also be a prepared array (G2_POINT_PREPARED) or a table handle (G2_POINT_TABLES)."""
        out = ctypes.create_string_buffer(192)
        self._check(_lib().msm_amd_msm_g2_device(self.h, scalar_layout, point_layout, d_scalars, d_points, n, out))
        return out.raw

    # ---- persistent G2 bases and precomputed G2 window tables (bases_upload ... msm_tables on G2) ----
    def g2_bases_upload(self, points: bytes, n: int, point_layout=G2_POINT_H2C_AFFINE) -> int:
        """Convert once, keep resident; returns a device pointer to pass with G2_POINT_PREPARED (free with .free)."""
        p = c_void_p()
        self._check(_lib().msm_amd_g2_bases_upload(self.h, point_layout, points, n, ctypes.byref(p)))
        return p.value

    def g2_bases_prepare_device(self, d_points, n, point_layout=G2_POINT_H2C_AFFINE) -> int:
        out = self.alloc(G2_PREPARED_BYTES * n)
        try:
            self._check(_lib().msm_amd_g2_bases_prepare_device(self.h, point_layout, c_void_p(d_points), n,
                                                               c_void_p(out)))
        except MsmError:
            self.free(out)
            raise
        return out

    def msm_g2_prepared(self, scalars: bytes, d_prepared, n, scalar_layout=SCALAR_MONT_LE) -> bytes:
        out = ctypes.create_string_buffer(192)
        self._check(_lib().msm_amd_msm_g2_prepared(self.h, scalar_layout, scalars, c_void_p(d_prepared), n, out))
        return out.raw

    def g2_tables_build(self, points: bytes, n: int, point_layout=G2_POINT_H2C_AFFINE, window_size=0) -> int:
        """Returns a G2 table handle: pass it as the points pointer with G2_POINT_TABLES, free with g2_tables_free."""
        h = c_void_p()
        self._check(_lib().msm_amd_g2_tables_build(self.h, point_layout, points, n, window_size, ctypes.byref(h)))
        return h.value

    def g2_tables_build_device(self, d_points, n, point_layout=G2_POINT_H2C_AFFINE, window_size=0) -> int:
        h = c_void_p()
        self._check(_lib().msm_amd_g2_tables_build_device(self.h, point_layout, c_void_p(d_points), n, window_size,
                                                          ctypes.byref(h)))
        return h.value

    def g2_tables_info(self, tables):
        n, nbytes, c, W = c_size_t(), c_size_t(), c_uint32(), c_uint32()
        self._check(_lib().msm_amd_g2_tables_info(self.h, c_void_p(tables), ctypes.byref(n), ctypes.byref(c),
                                                  ctypes.byref(W), ctypes.byref(nbytes)))
        return {"n": n.value, "window_size": c.value, "num_windows": W.value, "device_bytes": nbytes.value}

    def g2_tables_free(self, tables):
        self._check(_lib().msm_amd_g2_tables_free(self.h, c_void_p(tables)))

    def msm_g2_tables(self, scalars: bytes, tables, scalar_layout=SCALAR_MONT_LE) -> bytes:
        out = ctypes.create_string_buffer(192)
        self._check(_lib().msm_amd_msm_g2_tables(self.h, c_void_p(tables), scalar_layout, scalars, out))
        return out.raw

    def g2_tables_read(self, tables, w, first, count) -> bytes:
        """Test aid: `count` entries of window w from point `first` on, G2_POINT_H2C_AFFINE records."""
        out = ctypes.create_string_buffer(128 * count)
        self._check(_lib().msm_amd_test_g2_tables_read(self.h, c_void_p(tables), w, first, count, out))
        return out.raw

    # ---- point validation (range, on-curve, G2 subgroup) -------------------------------------------
    def _check_host_buffers(self, fn, points, n, checks, point_layout, want_reasons):
        rep = CheckReport()
        reasons = ctypes.create_string_buffer(max(n, 1)) if want_reasons else None
        self._check(fn(self.h, point_layout, points, n, checks, reasons, ctypes.byref(rep)))
        return rep.as_dict(), (reasons.raw[:n] if want_reasons else None)

    def _check_device(self, fn, d_points, n, checks, point_layout, d_reasons):
        rep = CheckReport()
        self._check(fn(self.h, point_layout, c_void_p(d_points), n, checks, c_void_p(d_reasons), ctypes.byref(rep)))
        return rep.as_dict()

    def check_points(self, points: bytes, n: int, checks=CHECK_CURVE, point_layout=POINT_H2C_AFFINE, reasons=True):
        """Judge n G1 points (a host layout) on the GPU: (report dict, n reason bytes or None)."""
        return self._check_host_buffers(_lib().msm_amd_check_points, points, n, checks, point_layout, reasons)

    def check_points_device(self, d_points, n: int, checks=CHECK_CURVE, point_layout=POINT_H2C_AFFINE, d_reasons=None):
        """The same on device-resident points; d_reasons: n bytes of device memory or None.  Returns the report."""
        return self._check_device(_lib().msm_amd_check_points_device, d_points, n, checks, point_layout, d_reasons)

    def g2_check_points(self, points: bytes, n: int, checks=CHECK_CURVE | CHECK_SUBGROUP,
                        point_layout=G2_POINT_H2C_AFFINE, reasons=True):
        """Judge n G2 points on the GPU (CHECK_SUBGROUP: [r] P = O): (report dict, n reason bytes or None)."""
        return self._check_host_buffers(_lib().msm_amd_g2_check_points, points, n, checks, point_layout, reasons)

    def g2_check_points_device(self, d_points, n: int, checks=CHECK_CURVE | CHECK_SUBGROUP,
                               point_layout=G2_POINT_H2C_AFFINE, d_reasons=None):
        return self._check_device(_lib().msm_amd_g2_check_points_device, d_points, n, checks, point_layout, d_reasons)

    # ---- compressed points -------------------------------------------------------------------------
    def decompress_points(self, data: bytes, n: int, fmt=COMPRESSED_ARK, point_layout=POINT_H2C_AFFINE, g2=False,
                          reasons=True):
        """Decompress n records (32 B, G2: 64 B) on the GPU from host memory: (points bytes, report dict, n reason
        bytes or None).  point_layout: an affine host layout of the group."""
        fn = _lib().msm_amd_g2_decompress_points if g2 else _lib().msm_amd_decompress_points
        out = ctypes.create_string_buffer(max(1, n * decompressed_bytes(point_layout, g2)))
        rs = ctypes.create_string_buffer(max(n, 1)) if reasons else None
        rep = DecompressReport()
        self._check(fn(self.h, fmt, data, n, point_layout, out, rs, ctypes.byref(rep)))
        return out.raw[:n * decompressed_bytes(point_layout, g2)], rep.as_dict(), (rs.raw[:n] if reasons else None)

    def decompress_points_device(self, d_in, n: int, d_out, fmt=COMPRESSED_ARK, point_layout=POINT_PREPARED, g2=False,
                                 d_reasons=None) -> dict:
        """The same between device buffers; also takes POINT_PREPARED / G2_POINT_PREPARED (MSM-ready bases in one
        pass).  Returns the report."""
        fn = _lib().msm_amd_g2_decompress_points_device if g2 else _lib().msm_amd_decompress_points_device
        rep = DecompressReport()
        self._check(fn(self.h, fmt, c_void_p(d_in), n, point_layout, c_void_p(d_out), c_void_p(d_reasons),
                       ctypes.byref(rep)))
        return rep.as_dict()

    def compress_points(self, points: bytes, n: int, fmt=COMPRESSED_ARK, point_layout=POINT_H2C_AFFINE, g2=False):
        """Compress n affine points (a host layout) on the GPU: (records bytes, n_bad)."""
        fn = _lib().msm_amd_g2_compress_points if g2 else _lib().msm_amd_compress_points
        size = 64 if g2 else 32
        out = ctypes.create_string_buffer(max(1, n * size))
        bad = c_uint64(0)
        self._check(fn(self.h, point_layout, points, n, fmt, out, ctypes.byref(bad)))
        return out.raw[:n * size], bad.value

    def compress_points_device(self, d_in, n: int, d_out, fmt=COMPRESSED_ARK, point_layout=POINT_H2C_AFFINE,
                               g2=False) -> int:
        fn = _lib().msm_amd_g2_compress_points_device if g2 else _lib().msm_amd_compress_points_device
        bad = c_uint64(0)
        self._check(fn(self.h, point_layout, c_void_p(d_in), n, fmt, c_void_p(d_out), ctypes.byref(bad)))
        return bad.value

    # ---- batch scalar multiplication --------------------------------------------------------------
    def mul_points(self, scalars: bytes, points: bytes, n: int, base_mode=MUL_BASE_EACH, scalar_layout=SCALAR_MONT_LE,
                   point_layout=POINT_H2C_AFFINE, point_layout_out=POINT_H2C_AFFINE, g2=False) -> bytes:
        """out[i] = [s_i] P_i (MUL_BASE_EACH: n point records) or [s_i] P (MUL_BASE_ONE: one record) on the GPU from
        host memory: n affine records of point_layout_out."""
        fn = _lib().msm_amd_g2_mul_points if g2 else _lib().msm_amd_mul_points
        size = decompressed_bytes(point_layout_out, g2)
        out = ctypes.create_string_buffer(max(1, n * size))
        self._check(fn(self.h, scalar_layout, point_layout, base_mode, scalars, points, n, point_layout_out, out))
        return out.raw[:n * size]

    def mul_points_device(self, d_scalars, d_points, n: int, d_out, base_mode=MUL_BASE_EACH, scalar_layout=SCALAR_MONT_LE,
                          point_layout=POINT_H2C_AFFINE, point_layout_out=POINT_PREPARED, g2=False) -> None:
        """The same between device buffers; points and output may also be POINT_PREPARED / G2_POINT_PREPARED records
        (a generated array is MSM-ready at once)."""
        fn = _lib().msm_amd_g2_mul_points_device if g2 else _lib().msm_amd_mul_points_device
        self._check(fn(self.h, scalar_layout, point_layout, base_mode, c_void_p(d_scalars), c_void_p(d_points), n,
                       point_layout_out, c_void_p(d_out)))

    def test_mul_stage(self, group, which, layout, data: bytes, table, n: int) -> bytes:
        """One stage of mul_points on the GPU (msm_amd_test_mul_stage): MUL_STAGE_FIXED walks the caller's table over n
        scalars and returns the raw XYZZ records, MUL_STAGE_NORMALISE turns n XYZZ records into affine ones,
        MUL_STAGE_NORMALISE_RECORDS returns the records as that stage leaves them."""
        out = ctypes.create_string_buffer(max(1, n * mul_stage_out_bytes(group, which, layout)))
        self._check(_lib().msm_amd_test_mul_stage(self.h, group, which, layout, data, table, n, out))
        return out.raw[:n * mul_stage_out_bytes(group, which, layout)]

    # ---- number-theoretic transform over Fr ------------------------------------------------------
    def ntt_domain(self, root, log_n) -> "NttDomain":
        """Twiddles of one (root, log_n) on this ctx's device (msm_amd_ntt_domain_build)."""
        h = c_void_p()
        self._check(_lib().msm_amd_ntt_domain_build(self.h, root, log_n, ctypes.byref(h)))
        return NttDomain(self, h)

    def ntt(self, dom, data: bytes, direction=NTT_FORWARD, scalar_layout=SCALAR_MONT_LE, shift=None, n_vec=1) -> bytes:
        """n_vec transforms of host records (msm_amd_ntt); shift: 32 bytes in scalar_layout, or None."""
        out = ctypes.create_string_buffer(max(1, len(data)))
        self._check(_lib().msm_amd_ntt(self.h, _ntt_handle(dom), direction, scalar_layout, shift, data, out, n_vec))
        return out.raw[:len(data)]

    def ntt_device(self, dom, d_in, d_out, direction=NTT_FORWARD, scalar_layout=SCALAR_MONT_LE, shift=None,
                   n_vec=1) -> float:
        """The same on device-resident records, d_out == d_in or disjoint (msm_amd_ntt_device); returns kernel_ms."""
        ms = c_float(0)
        self._check(_lib().msm_amd_ntt_device(self.h, _ntt_handle(dom), direction, scalar_layout, shift, c_void_p(d_in),
                                              c_void_p(d_out), n_vec, ctypes.byref(ms)))
        return ms.value

    def test_ntt_passes(self, dom, data: bytes, passes, direction=NTT_FORWARD, scalar_layout=SCALAR_MONT_LE, shift=None,
                        n_vec=1) -> bytes:
        """MsmConfig.ntt stopped after the first `passes` passes of its plan (msm_amd_test_ntt_passes): below the plan's
        count the pass buffer -- Montgomery residues at the positions of the network --, with it the result of ntt."""
        out = ctypes.create_string_buffer(max(1, len(data)))
        self._check(_lib().msm_amd_test_ntt_passes(self.h, _ntt_handle(dom), direction, scalar_layout, shift, data, out,
                                                   n_vec, passes))
        return out.raw[:len(data)]

    def test_ntt_twiddles(self, dom, first, count) -> bytes:
        """count records of a domain's table from entry first (msm_amd_test_ntt_twiddles): omega^j in MONT_LE"""
        out = ctypes.create_string_buffer(max(1, 32 * count))
        self._check(_lib().msm_amd_test_ntt_twiddles(self.h, _ntt_handle(dom), first, count, out))
        return out.raw[:32 * count]

    # ---- transform over G1 points ------------------------------------------------------------------
    def ntt_points(self, dom, points: bytes, direction=NTT_FORWARD, point_layout=POINT_H2C_AFFINE,
                   point_layout_out=POINT_H2C_AFFINE) -> bytes:
        """The transform of the domain's n host point records (msm_amd_ntt_points): n affine records of
        point_layout_out.  NTT_INVERSE on [tau^j] G gives the Lagrange SRS [L_i(tau)] G."""
        out, size = _ntt_points_out(_ntt_log_n(self, dom), points, point_layout, point_layout_out)
        self._check(_lib().msm_amd_ntt_points(self.h, _ntt_handle(dom), direction, point_layout, points, point_layout_out,
                                              out))
        return out.raw[:size]

    def ntt_points_device(self, dom, d_in, d_out, direction=NTT_FORWARD, point_layout=POINT_PREPARED,
                          point_layout_out=POINT_PREPARED) -> float:
        """The same between device buffers, d_out == d_in or disjoint; input and output may also be POINT_PREPARED
        records, which the MSM, table, check and compress calls take as they are; returns kernel_ms."""
        ms = c_float(0)
        self._check(_lib().msm_amd_ntt_points_device(self.h, _ntt_handle(dom), direction, point_layout, c_void_p(d_in),
                                                     point_layout_out, c_void_p(d_out), ctypes.byref(ms)))
        return ms.value

    def test_ntt_points_levels(self, dom, points: bytes, levels, direction=NTT_FORWARD, point_layout=POINT_H2C_AFFINE,
                               point_layout_out=POINT_H2C_AFFINE) -> bytes:
        """MsmConfig.ntt_points stopped after `levels` levels (msm_amd_test_ntt_points_levels): the work array as affine
        records in network order, no final scaling."""
        out, size = _ntt_points_out(_ntt_log_n(self, dom), points, point_layout, point_layout_out)
        self._check(_lib().msm_amd_test_ntt_points_levels(self.h, _ntt_handle(dom), direction, point_layout, points, levels,
                                                          point_layout_out, out))
        return out.raw[:size]

    # ---- vectors over Fr ---------------------------------------------------------------------------
    def fr_map(self, op, a: bytes, b: bytes = None, c: bytes = None, k: bytes = None, scalar_layout=SCALAR_MONT_LE) -> bytes:
        """out[i] = op(k, a[i], b[i], c[i]) on host records (msm_amd_fr_map); k: 32 bytes in scalar_layout"""
        n = len(a) // 32 if a is not None else 0
        out = ctypes.create_string_buffer(max(1, 32 * n))
        self._check(_lib().msm_amd_fr_map(self.h, op, scalar_layout, k, a, b, c, n, out))
        return out.raw[:32 * n]

    def fr_map_device(self, op, d_a, d_b, d_c, n: int, d_out, k: bytes = None, scalar_layout=SCALAR_MONT_LE) -> float:
        """The same on device-resident records, d_out an operand itself or disjoint (msm_amd_fr_map_device); returns
        kernel_ms."""
        ms = c_float(0)
        self._check(_lib().msm_amd_fr_map_device(self.h, op, scalar_layout, k, c_void_p(d_a), c_void_p(d_b), c_void_p(d_c), n,
                                                 c_void_p(d_out), ctypes.byref(ms)))
        return ms.value

    def fr_batch_inverse(self, data: bytes, scalar_layout=SCALAR_MONT_LE):
        """(records of the inverses -- 0 for 0 --, the number of zeros) of host records (msm_amd_fr_batch_inverse)"""
        n, zeros = len(data) // 32, c_uint64(0)
        out = ctypes.create_string_buffer(max(1, len(data)))
        self._check(_lib().msm_amd_fr_batch_inverse(self.h, scalar_layout, data, n, out, ctypes.byref(zeros)))
        return out.raw[:32 * n], zeros.value

    def fr_batch_inverse_device(self, d_in, n: int, d_out, scalar_layout=SCALAR_MONT_LE):
        """The same on device-resident records (msm_amd_fr_batch_inverse_device); returns (n_zero, kernel_ms)."""
        zeros, ms = c_uint64(0), c_float(0)
        self._check(_lib().msm_amd_fr_batch_inverse_device(self.h, scalar_layout, c_void_p(d_in), n, c_void_p(d_out),
                                                           ctypes.byref(zeros), ctypes.byref(ms)))
        return zeros.value, ms.value

    def fr_prefix_product(self, data: bytes, mode=FR_PREFIX_INCLUSIVE, scalar_layout=SCALAR_MONT_LE, n_vec=1) -> bytes:
        """Running products of n_vec vectors of host records, restarting at every vector (msm_amd_fr_prefix_product)"""
        n = len(data) // 32 // n_vec if n_vec else 0
        out = ctypes.create_string_buffer(max(1, len(data)))
        self._check(_lib().msm_amd_fr_prefix_product(self.h, scalar_layout, mode, data, n, n_vec, out))
        return out.raw[:32 * n * n_vec]

    def fr_prefix_product_device(self, d_in, n: int, d_out, mode=FR_PREFIX_INCLUSIVE, scalar_layout=SCALAR_MONT_LE,
                                 n_vec=1) -> float:
        """The same on device-resident records (msm_amd_fr_prefix_product_device); returns kernel_ms."""
        ms = c_float(0)
        self._check(_lib().msm_amd_fr_prefix_product_device(self.h, scalar_layout, mode, c_void_p(d_in), n, n_vec,
                                                            c_void_p(d_out), ctypes.byref(ms)))
        return ms.value

    def fr_prefix_sum(self, data: bytes, mode=FR_PREFIX_INCLUSIVE, scalar_layout=SCALAR_MONT_LE, n_vec=1) -> bytes:
        """Running sums of n_vec vectors of host records, restarting at every vector (msm_amd_fr_prefix_sum)"""
        n = len(data) // 32 // n_vec if n_vec else 0
        out = ctypes.create_string_buffer(max(1, len(data)))
        self._check(_lib().msm_amd_fr_prefix_sum(self.h, scalar_layout, mode, data, n, n_vec, out))
        return out.raw[:32 * n * n_vec]

    def fr_prefix_sum_device(self, d_in, n: int, d_out, mode=FR_PREFIX_INCLUSIVE, scalar_layout=SCALAR_MONT_LE,
                             n_vec=1) -> float:
        """The same on device-resident records (msm_amd_fr_prefix_sum_device); returns kernel_ms."""
        ms = c_float(0)
        self._check(_lib().msm_amd_fr_prefix_sum_device(self.h, scalar_layout, mode, c_void_p(d_in), n, n_vec,
                                                        c_void_p(d_out), ctypes.byref(ms)))
        return ms.value

    def fr_shift(self, a: bytes, k: bytes, scalar_layout=SCALAR_MONT_LE) -> bytes:
        """out[i] = a[i] + k on host records (msm_amd_fr_shift); k: 32 bytes in scalar_layout"""
        n = len(a) // 32 if a is not None else 0
        out = ctypes.create_string_buffer(max(1, 32 * n))
        self._check(_lib().msm_amd_fr_shift(self.h, scalar_layout, k, a, n, out))
        return out.raw[:32 * n]

    def fr_shift_device(self, d_a, n: int, d_out, k: bytes, scalar_layout=SCALAR_MONT_LE) -> float:
        """The same on device-resident records, d_out == d_a or disjoint (msm_amd_fr_shift_device); returns kernel_ms."""
        ms = c_float(0)
        self._check(_lib().msm_amd_fr_shift_device(self.h, scalar_layout, k, c_void_p(d_a), n, c_void_p(d_out),
                                                   ctypes.byref(ms)))
        return ms.value

    # ---- lookup tables over Fr: multiplicities and row indices --------------------------------------
    def fr_lookup_build(self, table: bytes, scalar_layout=SCALAR_MONT_LE, n_rows=None) -> "FrLookup":
        """The index of a table of host records on this ctx's device (msm_amd_fr_lookup_build)"""
        h = c_void_p()
        n_rows = len(table) // 32 if n_rows is None else n_rows
        self._check(_lib().msm_amd_fr_lookup_build(self.h, scalar_layout, table, n_rows, ctypes.byref(h)))
        return FrLookup(self, h)

    def fr_lookup_build_device(self, d_table, n_rows: int, scalar_layout=SCALAR_MONT_LE) -> "FrLookup":
        """The same from device-resident rows (msm_amd_fr_lookup_build_device); kernel_ms is left in .build_ms"""
        h, ms = c_void_p(), c_float(0)
        self._check(_lib().msm_amd_fr_lookup_build_device(self.h, scalar_layout, c_void_p(d_table), n_rows, ctypes.byref(h),
                                                          ctypes.byref(ms)))
        t = FrLookup(self, h)
        t.build_ms = ms.value
        return t

    def fr_lookup_info(self, table) -> dict:
        return _fr_lookup_info(self, _fr_lookup_handle(table))

    def fr_lookup_free(self, table):
        self._check(_lib().msm_amd_fr_lookup_free(self.h, _fr_lookup_handle(table)))

    def fr_lookup_multiplicities(self, table, data: bytes, on_missing=LOOKUP_STRICT, scalar_layout=SCALAR_MONT_LE, n_vec=1,
                                 want_idx=True, n_rows=None, m_out=None):
        """(m, idx or None, report) of n_vec columns of host records looked up in a table (msm_amd_fr_lookup_multiplicities):
        m as n_rows records, idx as a list of row indices (LOOKUP_NOT_FOUND for a miss), report as a dict.  A miss under
        LOOKUP_STRICT raises MsmError with .report and .idx set.  m_out: a ctypes buffer to write into (then m is None)."""
        n = (len(data) // 32 // n_vec if n_vec else 0) if data is not None else 1   # None: the null pointer of an argument test
        if n_rows is None:
            n_rows = self.fr_lookup_info(table)["n_rows"]
        m = ctypes.create_string_buffer(max(1, 32 * n_rows)) if m_out is None else m_out
        idx = (c_uint32 * max(1, n * n_vec))() if want_idx else None
        rep = (c_uint64 * 4)()
        st = _lib().msm_amd_fr_lookup_multiplicities(self.h, _fr_lookup_handle(table), scalar_layout, on_missing, data, n,
                                                     n_vec, m, idx, rep)
        return _lookup_result(self, st, m if m_out is None else None, n_rows, idx, n * n_vec, rep)

    def fr_lookup_multiplicities_device(self, table, d_in, n: int, d_m_out, d_idx_out=None, on_missing=LOOKUP_STRICT,
                                        scalar_layout=SCALAR_MONT_LE, n_vec=1):
        """The same on device-resident records (msm_amd_fr_lookup_multiplicities_device); returns (report, kernel_ms)."""
        rep, ms = (c_uint64 * 4)(), c_float(0)
        st = _lib().msm_amd_fr_lookup_multiplicities_device(self.h, _fr_lookup_handle(table), scalar_layout, on_missing,
                                                            c_void_p(d_in), n, n_vec, c_void_p(d_m_out), c_void_p(d_idx_out),
                                                            rep, ctypes.byref(ms))
        return _lookup_result(self, st, None, 0, None, 0, rep)[2], ms.value

    def fr_lookup_permute(self, table, data: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1, want_a=True, want_s=True,
                          a_out=None, s_out=None):
        """(A', S', report) of n_vec columns of host records against a table (msm_amd_fr_lookup_permute): halo2's permuted
        columns in row order, each n_vec n records or None if not asked for.  A value that is in no row raises MsmError with
        .report set.  a_out / s_out: ctypes buffers to write into (then that result is None)."""
        n = len(data) // 32 // n_vec if n_vec else 0
        a, s = _permute_buffers(n * n_vec, want_a, want_s, a_out, s_out)
        rep = (c_uint64 * 4)()
        st = _lib().msm_amd_fr_lookup_permute(self.h, _fr_lookup_handle(table), scalar_layout, data, n, n_vec, a, s, rep)
        return _permute_result(self, st, a if a_out is None else None, s if s_out is None else None, n * n_vec, rep)

    def fr_lookup_build_sorted(self, table, scalar_layout=SCALAR_MONT_LE, n_rows=None, mem=MEM_HOST, perm_out=None,
                               want_perm=True):
        """The handle over the table sorted by value (msm_amd_fr_lookup_build_sorted): row k is sorted position k.
        MEM_HOST: table is bytes; returns (FrLookup, perm list or None).  MEM_DEVICE: table and perm_out (optional) are device
        addresses and n_rows is required; returns (FrLookup, None).  kernel_ms is left in .build_ms."""
        h, ms = c_void_p(), c_float(0)
        if mem != MEM_HOST:
            self._check(_lib().msm_amd_fr_lookup_build_sorted(self.h, mem, scalar_layout, c_void_p(table), n_rows or 0,
                                                              c_void_p(perm_out), ctypes.byref(h), ctypes.byref(ms)))
            perm = None
        else:
            n_rows = len(table) // 32 if n_rows is None else n_rows
            perm = (c_uint32 * max(1, n_rows))() if want_perm else None
            self._check(_lib().msm_amd_fr_lookup_build_sorted(self.h, mem, scalar_layout, table, n_rows, perm, ctypes.byref(h),
                                                              ctypes.byref(ms)))
            perm = list(perm[:n_rows]) if want_perm else None
        t = FrLookup(self, h)
        t.build_ms = ms.value
        return t, perm

    def fr_lookup_sorted(self, table) -> bool:
        """whether a handle came from fr_lookup_build_sorted (msm_amd_fr_lookup_sorted)"""
        flag = c_int(-1)
        self._check(_lib().msm_amd_fr_lookup_sorted(self.h, _fr_lookup_handle(table), ctypes.byref(flag)))
        return bool(flag.value)

    def test_fr_lookup_image(self, table) -> int:
        """the device address of a handle's image (msm_amd_test_fr_lookup_image): for overlap tests only"""
        p = c_void_p()
        self._check(_lib().msm_amd_test_fr_lookup_image(self.h, _fr_lookup_handle(table), ctypes.byref(p)))
        return p.value

    def fr_lookup_permute_as(self, table, data, arrangement=PERMUTE_HALO2, scalar_layout=SCALAR_MONT_LE, n_vec=1,
                             mem=MEM_HOST, n=None, want_a=True, want_s=True, a_out=None, s_out=None):
        """A', S' in a chosen arrangement (msm_amd_fr_lookup_permute_as).  MEM_HOST: as fr_lookup_permute, returns
        (A', S', report).  MEM_DEVICE: data, a_out, s_out are device addresses (None: not asked for), n is required; returns
        (None, None, report) and leaves kernel_ms in .last_kernel_ms.  A miss raises MsmError with .report set."""
        rep, ms = (c_uint64 * 4)(), c_float(0)
        if mem != MEM_HOST:
            st = _lib().msm_amd_fr_lookup_permute_as(self.h, _fr_lookup_handle(table), mem, scalar_layout, arrangement,
                                                     c_void_p(data), n or 0, n_vec, c_void_p(a_out), c_void_p(s_out), rep,
                                                     ctypes.byref(ms))
            self.last_kernel_ms = ms.value
            return _permute_result(self, st, None, None, 0, rep)
        if n is None:
            n = len(data) // 32 // n_vec if n_vec else 0
        a, s = _permute_buffers(n * n_vec, want_a, want_s, a_out, s_out)
        st = _lib().msm_amd_fr_lookup_permute_as(self.h, _fr_lookup_handle(table), mem, scalar_layout, arrangement, data, n,
                                                 n_vec, a, s, rep, ctypes.byref(ms))
        self.last_kernel_ms = ms.value
        return _permute_result(self, st, a if a_out is None else None, s if s_out is None else None, n * n_vec, rep)

    # ---- sorting Fr records by canonical value ---------------------------------------------------------
    def fr_sort(self, data, scalar_layout=SCALAR_MONT_LE, n_vec=1, mem=MEM_HOST, n=None, out=None, perm_out=None,
                want_out=True, want_perm=True):
        """n_vec columns of n records, each sorted ascending by canonical value, stably (msm_amd_fr_sort).
        MEM_HOST: data is bytes or a ctypes buffer; returns (records or None, perm as a list or None, kernel_ms); out /
        perm_out: ctypes buffers to write into (then that result is None; out may be data itself).
        MEM_DEVICE: data, out and perm_out are device addresses (None: not asked for) and n is required; returns
        (None, None, kernel_ms)."""
        ms = c_float(0)
        if mem != MEM_HOST:
            self._check(_lib().msm_amd_fr_sort(self.h, mem, scalar_layout, c_void_p(data), n or 0, n_vec, c_void_p(out),
                                               c_void_p(perm_out), ctypes.byref(ms)))
            return None, None, ms.value
        if n is None:
            n = len(data) // 32 // n_vec if n_vec else 0
        o = out if out is not None else ctypes.create_string_buffer(max(1, 32 * n * n_vec)) if want_out else None
        p = perm_out if perm_out is not None else (c_uint32 * max(1, n * n_vec))() if want_perm else None
        self._check(_lib().msm_amd_fr_sort(self.h, mem, scalar_layout, data, n, n_vec, o, p, ctypes.byref(ms)))
        return (o.raw[:32 * n * n_vec] if o is not None and out is None else None,
                list(p[:n * n_vec]) if p is not None and perm_out is None else None, ms.value)

    # ---- polynomials over Fr: n_vec polynomials of n coefficients back to back, lowest degree first -------
    def fr_poly_eval(self, coeffs: bytes, z: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1) -> bytes:
        """The n_vec records p_v(z) of host coefficients (msm_amd_fr_poly_eval); z: 32 bytes in scalar_layout"""
        n = len(coeffs) // 32 // n_vec if n_vec else 0
        y = ctypes.create_string_buffer(max(1, 32 * n_vec))
        self._check(_lib().msm_amd_fr_poly_eval(self.h, scalar_layout, z, coeffs, n, n_vec, y))
        return y.raw[:32 * n_vec] if n else b""

    def fr_poly_eval_device(self, d_coeffs, n: int, z: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1):
        """The same on device-resident coefficients (msm_amd_fr_poly_eval_device); returns (records, kernel_ms)."""
        ms = c_float(0)
        y = ctypes.create_string_buffer(max(1, 32 * n_vec))
        self._check(_lib().msm_amd_fr_poly_eval_device(self.h, scalar_layout, z, c_void_p(d_coeffs), n, n_vec, y,
                                                       ctypes.byref(ms)))
        return (y.raw[:32 * n_vec] if n else b""), ms.value

    def fr_poly_div_linear(self, data: bytes, z: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1):
        """(the quotients of p_v by X - z, padded with a zero record to n; the remainders p_v(z)) of host coefficients
        (msm_amd_fr_poly_div_linear)"""
        n = len(data) // 32 // n_vec if n_vec else 0
        out = ctypes.create_string_buffer(max(1, len(data)))
        rem = ctypes.create_string_buffer(max(1, 32 * n_vec))
        self._check(_lib().msm_amd_fr_poly_div_linear(self.h, scalar_layout, z, data, n, n_vec, out, rem))
        return out.raw[:32 * n * n_vec], (rem.raw[:32 * n_vec] if n else b"")

    def fr_poly_div_linear_device(self, d_in, n: int, d_out, z: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1, rem=True):
        """The same on device-resident coefficients, d_out == d_in or disjoint (msm_amd_fr_poly_div_linear_device);
        returns (remainders -- None with rem=False: rem_out is null --, kernel_ms)."""
        ms = c_float(0)
        r = ctypes.create_string_buffer(max(1, 32 * n_vec)) if rem else None
        self._check(_lib().msm_amd_fr_poly_div_linear_device(self.h, scalar_layout, z, c_void_p(d_in), n, n_vec,
                                                             c_void_p(d_out), r, ctypes.byref(ms)))
        return ((r.raw[:32 * n_vec] if n else b"") if rem else None), ms.value

    def fr_poly_eval_points(self, coeffs, z: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1, mem=MEM_HOST, n=None):
        """p_v(z_j) at the k = len(z) // 32 points of z in one pass (msm_amd_fr_poly_eval_points): returns (the n_vec k
        records y[v k + j], kernel_ms).  MEM_HOST: coeffs is bytes; MEM_DEVICE: a device address, and n is required."""
        k = len(z) // 32
        if mem == MEM_HOST and n is None:
            n = len(coeffs) // 32 // n_vec if n_vec else 0
        ms = c_float(0)
        y = ctypes.create_string_buffer(max(1, 32 * n_vec * k))
        src = coeffs if mem == MEM_HOST else c_void_p(coeffs)
        self._check(_lib().msm_amd_fr_poly_eval_points(self.h, mem, scalar_layout, z, k, src, n or 0, n_vec, y,
                                                       ctypes.byref(ms)))
        return (y.raw[:32 * n_vec * k] if n else b""), ms.value

    def fr_poly_div_points(self, data, z: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1, mem=MEM_HOST, n=None, out=None,
                           vals=True):
        """The quotients of p_v by prod_j (X - z_j) over the k = len(z) // 32 distinct points of z, n records each, and the
        values p_v(z_j) (msm_amd_fr_poly_div_points).  MEM_HOST: data is bytes, returns (quotients, values or None,
        kernel_ms).  MEM_DEVICE: data and out are device addresses (out == data or disjoint), n is required, returns
        (None, values or None, kernel_ms).  vals=False: vals_out is null."""
        k = len(z) // 32
        ms = c_float(0)
        val = ctypes.create_string_buffer(max(1, 32 * n_vec * k)) if vals else None
        if mem != MEM_HOST:
            self._check(_lib().msm_amd_fr_poly_div_points(self.h, mem, scalar_layout, z, k, c_void_p(data), n or 0, n_vec,
                                                          c_void_p(out), val, ctypes.byref(ms)))
            return None, ((val.raw[:32 * n_vec * k] if n else b"") if vals else None), ms.value
        if n is None:
            n = len(data) // 32 // n_vec if n_vec else 0
        o = ctypes.create_string_buffer(max(1, 32 * n * n_vec))
        self._check(_lib().msm_amd_fr_poly_div_points(self.h, mem, scalar_layout, z, k, data, n, n_vec, o, val,
                                                      ctypes.byref(ms)))
        return o.raw[:32 * n * n_vec], ((val.raw[:32 * n_vec * k] if n else b"") if vals else None), ms.value

    def fr_lincomb(self, data: bytes, k: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1) -> bytes:
        """out[i] = sum_v k^v a[v n + i] of host records (msm_amd_fr_lincomb)"""
        n = len(data) // 32 // n_vec if n_vec else 0
        out = ctypes.create_string_buffer(max(1, 32 * n))
        self._check(_lib().msm_amd_fr_lincomb(self.h, scalar_layout, k, data, n, n_vec, out))
        return out.raw[:32 * n]

    def fr_lincomb_device(self, d_a, n: int, d_out, k: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1) -> float:
        """The same on device-resident records, d_out the first vector or disjoint from all (msm_amd_fr_lincomb_device);
        returns kernel_ms."""
        ms = c_float(0)
        self._check(_lib().msm_amd_fr_lincomb_device(self.h, scalar_layout, k, c_void_p(d_a), n, n_vec, c_void_p(d_out),
                                                     ctypes.byref(ms)))
        return ms.value

    # ---- sparse matrix times vector over Fr ---------------------------------------------------------
    def fr_matrix_build(self, n_rows, n_cols, row_ptr, col_idx, values: bytes, scalar_layout=SCALAR_MONT_LE) -> "FrMatrix":
        """A CSR matrix of host data on this ctx's device (msm_amd_fr_matrix_build): row_ptr of n_rows + 1 offsets and
        col_idx of nnz columns (sequences of int, or the packed u64 / u32 bytes), values of nnz records; col_idx and
        values may be None with nnz == 0."""
        h = c_void_p()
        self._check(_lib().msm_amd_fr_matrix_build(self.h, scalar_layout, n_rows, n_cols, _csr_u64(row_ptr),
                                                   _csr_u32(col_idx), values, ctypes.byref(h)))
        return FrMatrix(self, h)

    def fr_matrix_info(self, mat) -> dict:
        return _fr_matrix_info(self, _fr_matrix_handle(mat))

    def fr_matrix_free(self, mat):
        self._check(_lib().msm_amd_fr_matrix_free(self.h, _fr_matrix_handle(mat)))

    def fr_matvec(self, mat, x: bytes, scalar_layout=SCALAR_MONT_LE, n_rows=None) -> bytes:
        """y = M x of host records (msm_amd_fr_matvec); n_rows: the rows of the matrix if the caller knows them"""
        if n_rows is None:
            n_rows = self.fr_matrix_info(mat)["n_rows"]
        y = ctypes.create_string_buffer(max(1, 32 * n_rows))
        self._check(_lib().msm_amd_fr_matvec(self.h, _fr_matrix_handle(mat), scalar_layout, x, y))
        return y.raw[:32 * n_rows]

    def fr_matvec_device(self, mat, d_x, d_y, scalar_layout=SCALAR_MONT_LE) -> float:
        """The same on device-resident records, d_y disjoint from d_x (msm_amd_fr_matvec_device); returns kernel_ms."""
        ms = c_float(0)
        self._check(_lib().msm_amd_fr_matvec_device(self.h, _fr_matrix_handle(mat), scalar_layout, c_void_p(d_x),
                                                    c_void_p(d_y), ctypes.byref(ms)))
        return ms.value

    # ---- Poseidon over Fr: permutations, hashes and Merkle trees -------------------------------------
    def poseidon_params_build(self, t, r_f, r_p, ark: bytes, mds: bytes, scalar_layout=SCALAR_MONT_LE) -> "PoseidonParams":
        """The constants of one Poseidon instance on this ctx's device (msm_amd_poseidon_params_build): (r_f + r_p) t
        records of round constants and t t records of the matrix, the caller's own or those of poseidon_constants()."""
        h = c_void_p()
        self._check(_lib().msm_amd_poseidon_params_build(self.h, t, r_f, r_p, scalar_layout, ark, mds, ctypes.byref(h)))
        return PoseidonParams(self, h)

    def poseidon_params(self, t, r_f=8, r_p=None) -> "PoseidonParams":
        """The handle of the generated constants (circomlib's at the default rounds)"""
        r_p = POSEIDON_R_P[t] if r_p is None else r_p
        return self.poseidon_params_build(t, r_f, r_p, *poseidon_constants(t, r_f, r_p))

    def poseidon_permute(self, params, data: bytes, n: int, scalar_layout=SCALAR_MONT_LE) -> bytes:
        """n states of t host records -> n states (msm_amd_poseidon_permute)"""
        t = _poseidon_t(self, params)
        out = ctypes.create_string_buffer(max(1, 32 * n * t))
        self._check(_lib().msm_amd_poseidon_permute(self.h, _poseidon_handle(params), scalar_layout, data, n, out))
        return out.raw[:32 * n * t]

    def poseidon_permute_device(self, params, d_in, n: int, d_out, scalar_layout=SCALAR_MONT_LE) -> float:
        """The same on device-resident states, d_out == d_in or disjoint (msm_amd_poseidon_permute_device); returns
        kernel_ms."""
        ms = c_float(0)
        self._check(_lib().msm_amd_poseidon_permute_device(self.h, _poseidon_handle(params), scalar_layout, c_void_p(d_in), n,
                                                           c_void_p(d_out), ctypes.byref(ms)))
        return ms.value

    def poseidon_hash(self, params, data: bytes, n: int, scalar_layout=SCALAR_MONT_LE, tag: bytes = None) -> bytes:
        """n groups of t - 1 host records -> n digests (msm_amd_poseidon_hash); tag: one record, None for 0"""
        out = ctypes.create_string_buffer(max(1, 32 * n))
        self._check(_lib().msm_amd_poseidon_hash(self.h, _poseidon_handle(params), scalar_layout, tag, data, n, out))
        return out.raw[:32 * n]

    def poseidon_hash_device(self, params, d_in, n: int, d_out, scalar_layout=SCALAR_MONT_LE, tag: bytes = None) -> float:
        """The same on device-resident records (msm_amd_poseidon_hash_device); returns kernel_ms."""
        ms = c_float(0)
        self._check(_lib().msm_amd_poseidon_hash_device(self.h, _poseidon_handle(params), scalar_layout, tag, c_void_p(d_in), n,
                                                        c_void_p(d_out), ctypes.byref(ms)))
        return ms.value

    def poseidon_merkle_build(self, params, leaves: bytes, n_leaves: int, scalar_layout=SCALAR_MONT_LE, tag: bytes = None):
        """The inner nodes of the tree over host leaves, the root last, and the root (msm_amd_poseidon_merkle_build)"""
        nodes = merkle_nodes(_poseidon_t(self, params), n_leaves)
        tree, root = ctypes.create_string_buffer(max(1, 32 * nodes)), ctypes.create_string_buffer(32)
        self._check(_lib().msm_amd_poseidon_merkle_build(self.h, _poseidon_handle(params), scalar_layout, tag, leaves, n_leaves,
                                                         tree, root))
        return tree.raw[:32 * nodes], root.raw

    def poseidon_merkle_build_device(self, params, d_leaves, n_leaves: int, d_tree, scalar_layout=SCALAR_MONT_LE,
                                     tag: bytes = None, want_root=True):
        """The same on device-resident leaves into device memory (msm_amd_poseidon_merkle_build_device); returns
        (root or None, kernel_ms)."""
        ms, root = c_float(0), ctypes.create_string_buffer(32) if want_root else None
        self._check(_lib().msm_amd_poseidon_merkle_build_device(self.h, _poseidon_handle(params), scalar_layout, tag,
                                                                c_void_p(d_leaves), n_leaves, c_void_p(d_tree), root,
                                                                ctypes.byref(ms)))
        return (root.raw if want_root else None), ms.value

    def poseidon_merkle_paths(self, params, leaves: bytes, n_leaves: int, tree: bytes, idx, scalar_layout=SCALAR_MONT_LE) -> bytes:
        """d (a - 1) sibling records per leaf index of idx, host memory throughout (msm_amd_poseidon_merkle_paths)"""
        size = 32 * len(idx) * merkle_path_records(_poseidon_t(self, params), n_leaves)
        out = ctypes.create_string_buffer(max(1, size))
        self._check(_lib().msm_amd_poseidon_merkle_paths(self.h, _poseidon_handle(params), scalar_layout, leaves, n_leaves, tree,
                                                         _csr_u64(idx), len(idx), out))
        return out.raw[:size]

    def poseidon_merkle_paths_device(self, params, d_leaves, n_leaves: int, d_tree, idx, d_out,
                                     scalar_layout=SCALAR_MONT_LE) -> float:
        """The same from device-resident leaves and tree into device memory (msm_amd_poseidon_merkle_paths_device);
        returns kernel_ms."""
        ms = c_float(0)
        self._check(_lib().msm_amd_poseidon_merkle_paths_device(self.h, _poseidon_handle(params), scalar_layout,
                                                                c_void_p(d_leaves), n_leaves, c_void_p(d_tree), _csr_u64(idx),
                                                                len(idx), c_void_p(d_out), ctypes.byref(ms)))
        return ms.value

    # ---- multilinear tables over Fr and sumcheck rounds: n_vec tables of n = 2^m records, `stride` records apart ----
    def fr_mle_bind(self, data: bytes, r: bytes, n: int, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, n_vec=1, stride=None,
                    out: bytes = None) -> bytes:
        """len(r) / 32 steps of `order` on host tables (msm_amd_fr_mle_bind): the output span of (n_vec - 1) stride + n / 2
        records, or all of `out` if given: the call writes over a copy of it, so that what it leaves alone shows."""
        stride = n if stride is None else stride
        span = 32 * ((n_vec - 1) * stride + n // 2) if n_vec else 0
        size = len(out) if out is not None else span
        buf = ctypes.create_string_buffer(out if out is not None else b"\xFF" * span, size + 1)
        self._check(_lib().msm_amd_fr_mle_bind(self.h, scalar_layout, order, r, len(r) // 32 if r else 0, data, n, n_vec,
                                               stride, buf))
        return buf.raw[:size]

    def fr_mle_bind_device(self, d_in, n: int, d_out, r: bytes, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, n_vec=1,
                           stride=None, n_bind=None) -> float:
        """The same on device-resident tables, d_out == d_in with MLE_HIGH or disjoint (msm_amd_fr_mle_bind_device);
        returns kernel_ms."""
        ms = c_float(0)
        n_bind = (len(r) // 32 if r else 0) if n_bind is None else n_bind
        self._check(_lib().msm_amd_fr_mle_bind_device(self.h, scalar_layout, order, r, n_bind, c_void_p(d_in), n, n_vec,
                                                      n if stride is None else stride, c_void_p(d_out), ctypes.byref(ms)))
        return ms.value

    def fr_mle_eval(self, data: bytes, point: bytes, n: int, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, n_vec=1,
                    stride=None) -> bytes:
        """The n_vec records f_v(point) of host tables (msm_amd_fr_mle_eval); point: log2 n records in scalar_layout"""
        y = ctypes.create_string_buffer(max(1, 32 * n_vec))
        self._check(_lib().msm_amd_fr_mle_eval(self.h, scalar_layout, order, point, data, n, n_vec,
                                               n if stride is None else stride, y))
        return y.raw[:32 * n_vec]

    def fr_mle_eval_device(self, d_in, n: int, point: bytes, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, n_vec=1,
                           stride=None):
        """The same on device-resident tables (msm_amd_fr_mle_eval_device); returns (records, kernel_ms)."""
        ms = c_float(0)
        y = ctypes.create_string_buffer(max(1, 32 * n_vec))
        self._check(_lib().msm_amd_fr_mle_eval_device(self.h, scalar_layout, order, point, c_void_p(d_in), n, n_vec,
                                                      n if stride is None else stride, y, ctypes.byref(ms)))
        return y.raw[:32 * n_vec], ms.value

    def fr_eq_table(self, point: bytes, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, m=None) -> bytes:
        """The 2^m records eq(point, .) in host memory (msm_amd_fr_eq_table)"""
        m = (len(point) // 32 if point else 0) if m is None else m
        out = ctypes.create_string_buffer(max(1, 32 << m if 0 < m < 32 else 1))
        self._check(_lib().msm_amd_fr_eq_table(self.h, scalar_layout, order, point, m, out))
        return out.raw[:32 << m]

    def fr_eq_table_device(self, d_out, point: bytes, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, m=None) -> float:
        """The same into device memory of 2^m records (msm_amd_fr_eq_table_device); returns kernel_ms."""
        ms = c_float(0)
        m = (len(point) // 32 if point else 0) if m is None else m
        self._check(_lib().msm_amd_fr_eq_table_device(self.h, scalar_layout, order, point, m, c_void_p(d_out),
                                                      ctypes.byref(ms)))
        return ms.value

    def fr_sumcheck_round(self, data: bytes, n: int, form=SUMCHECK_PRODUCT, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE,
                          n_vec=1, stride=None) -> bytes:
        """The d + 1 records g(0) .. g(d) of one round over host tables (msm_amd_fr_sumcheck_round)"""
        g = ctypes.create_string_buffer(32 * 5)
        self._check(_lib().msm_amd_fr_sumcheck_round(self.h, scalar_layout, order, form, data, n, n_vec,
                                                     n if stride is None else stride, g))
        return g.raw[:32 * sumcheck_values(form, n_vec)]

    def fr_sumcheck_round_device(self, d_in, n: int, form=SUMCHECK_PRODUCT, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE,
                                 n_vec=1, stride=None):
        """The same on device-resident tables (msm_amd_fr_sumcheck_round_device); returns (records, kernel_ms)."""
        ms = c_float(0)
        g = ctypes.create_string_buffer(32 * 5)
        self._check(_lib().msm_amd_fr_sumcheck_round_device(self.h, scalar_layout, order, form, c_void_p(d_in), n, n_vec,
                                                            n if stride is None else stride, g, ctypes.byref(ms)))
        return g.raw[:32 * sumcheck_values(form, n_vec)], ms.value

    def fr_sumcheck_round_terms(self, data: bytes, n: int, terms, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, n_vec=1,
                                stride=None) -> bytes:
        """The d + 1 records g(0) .. g(d) of one round of a SumcheckTerms list over host tables
        (msm_amd_fr_sumcheck_round_terms with MEM_HOST)"""
        g = ctypes.create_string_buffer(32 * 8)
        self._check(_lib().msm_amd_fr_sumcheck_round_terms(self.h, MEM_HOST, scalar_layout, order, _terms_ptr(terms), data, n, n_vec,
                                                           n if stride is None else stride, g, None))
        return g.raw[:32 * sumcheck_terms_values(terms, n_vec)]

    def fr_sumcheck_round_terms_device(self, d_in, n: int, terms, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, n_vec=1,
                                       stride=None):
        """The same on device-resident tables (msm_amd_fr_sumcheck_round_terms with MEM_DEVICE); returns (records, kernel_ms)."""
        ms = c_float(0)
        g = ctypes.create_string_buffer(32 * 8)
        self._check(_lib().msm_amd_fr_sumcheck_round_terms(self.h, MEM_DEVICE, scalar_layout, order, _terms_ptr(terms), c_void_p(d_in),
                                                                  n, n_vec, n if stride is None else stride, g,
                                                                  ctypes.byref(ms)))
        return g.raw[:32 * sumcheck_terms_values(terms, n_vec)], ms.value

    def fr_sumcheck_step_terms(self, data: bytes, r: bytes, n: int, terms, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, n_vec=1,
                               stride=None, out: bytes = None):
        """Bind r, then the next round's values, over host tables (msm_amd_fr_sumcheck_step_terms): (the output span of
        (n_vec - 1) stride + n / 2 records, or all of `out` if given, written over a copy of it; the d + 1 records)"""
        stride = n if stride is None else stride
        span = 32 * ((n_vec - 1) * stride + n // 2) if n_vec else 0
        size = len(out) if out is not None else span
        buf = ctypes.create_string_buffer(out if out is not None else b"\xFF" * span, size + 1)
        g = ctypes.create_string_buffer(32 * 8)
        self._check(_lib().msm_amd_fr_sumcheck_step_terms(self.h, MEM_HOST, scalar_layout, order, _terms_ptr(terms), r, data, n, n_vec,
                                                          stride, buf, g, None))
        return buf.raw[:size], g.raw[:32 * sumcheck_terms_values(terms, n_vec)]

    def fr_sumcheck_step_terms_device(self, d_in, n: int, d_out, r: bytes, terms, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE,
                                      n_vec=1, stride=None):
        """The same on device-resident tables, d_out == d_in with MLE_HIGH or disjoint
        (msm_amd_fr_sumcheck_step_terms with MEM_DEVICE); returns (records, kernel_ms)."""
        ms = c_float(0)
        g = ctypes.create_string_buffer(32 * 8)
        self._check(_lib().msm_amd_fr_sumcheck_step_terms(self.h, MEM_DEVICE, scalar_layout, order, _terms_ptr(terms), r,
                                                                 c_void_p(d_in), n, n_vec, n if stride is None else stride,
                                                                 c_void_p(d_out), g, ctypes.byref(ms)))
        return g.raw[:32 * sumcheck_terms_values(terms, n_vec)], ms.value

    def fr_gate_eval(self, columns, terms, n=None, n_vec=1, stride=None, rot_step=1, flags=0, k_acc: bytes = None,
                     scale: bytes = None, out=None, scalar_layout=SCALAR_MONT_LE, mem=MEM_HOST):
        """out[i] = sum_k c_k prod_j col[(i + rot rot_step) mod n] of a GateTerms list (msm_amd_fr_gate_eval); with
        GATE_ACCUMULATE out[i] = k_acc out[i] + that, and with `scale` (period = len(scale) // 32 records) times
        scale[i mod period].  MEM_HOST: columns is bytes and `out` the old n records (required with GATE_ACCUMULATE, else a
        poison the call must not read); returns (the n records, kernel_ms).  MEM_DEVICE: columns and out are device
        addresses and n is required; returns (None, kernel_ms)."""
        ms = c_float(0)
        period = len(scale) // 32 if scale is not None else 0
        if mem != MEM_HOST:
            self._check(_lib().msm_amd_fr_gate_eval(self.h, mem, scalar_layout, flags, _terms_ptr(terms), c_void_p(columns), n or 0,
                                                    n_vec, (n or 0) if stride is None else stride, rot_step, k_acc, scale, period,
                                                    c_void_p(out), ctypes.byref(ms)))
            return None, ms.value
        if n is None:
            n = len(columns) // 32 // n_vec if n_vec else 0
        buf = ctypes.create_string_buffer(out if out is not None else b"\xFF" * (32 * n), 32 * n + 1)
        self._check(_lib().msm_amd_fr_gate_eval(self.h, mem, scalar_layout, flags, _terms_ptr(terms), columns, n, n_vec,
                                                n if stride is None else stride, rot_step, k_acc, scale, period, buf,
                                                ctypes.byref(ms)))
        return buf.raw[:32 * n], ms.value

    # ---- pairings -------------------------------------------------------------------------------
    def pairing_product(self, g1_points: bytes, g2_points: bytes, n_groups: int, group_size: int, flags=0,
                        gt_layout=GT_MONT_LE, point_layout=POINT_H2C_AFFINE, g2_point_layout=G2_POINT_H2C_AFFINE,
                        want_is_one=True):
        """Group g = the product of e(P_i, Q_i) over its group_size pairs, on the GPU from host memory
        (msm_amd_pairing_product); returns (n_groups GT records, is_one bytes or None)."""
        out = ctypes.create_string_buffer(max(1, n_groups * GT_BYTES))
        flag = ctypes.create_string_buffer(max(1, n_groups)) if want_is_one and not flags & PAIRING_MILLER_ONLY else None
        self._check(_lib().msm_amd_pairing_product(self.h, point_layout, g2_point_layout, g1_points, g2_points, n_groups,
                                                   group_size, flags, gt_layout, out, flag))
        return out.raw[:n_groups * GT_BYTES], (flag.raw[:n_groups] if flag is not None else None)

    def pairing_product_device(self, d_g1, d_g2, n_groups: int, group_size: int, d_out, d_is_one=None, flags=0,
                               gt_layout=GT_MONT_LE, point_layout=POINT_H2C_AFFINE,
                               g2_point_layout=G2_POINT_H2C_AFFINE) -> float:
        """The same between device buffers (points may be *_PREPARED records); returns kernel_ms."""
        ms = c_float(0)
        self._check(_lib().msm_amd_pairing_product_device(self.h, point_layout, g2_point_layout, c_void_p(d_g1),
                                                          c_void_p(d_g2), n_groups, group_size, flags, gt_layout,
                                                          c_void_p(d_out), c_void_p(d_is_one), ctypes.byref(ms)))
        return ms.value

    def final_exponentiation(self, records: bytes, n: int, gt_layout=GT_MONT_LE):
        """msm_amd_final_exponentiation on host memory; returns (records, is_one bytes)."""
        out = ctypes.create_string_buffer(max(1, n * GT_BYTES))
        flag = ctypes.create_string_buffer(max(1, n))
        self._check(_lib().msm_amd_final_exponentiation(self.h, gt_layout, records, n, out, flag))
        return out.raw[:n * GT_BYTES], flag.raw[:n]

    def final_exponentiation_device(self, d_in, n: int, d_out, d_is_one=None, gt_layout=GT_MONT_LE) -> float:
        ms = c_float(0)
        self._check(_lib().msm_amd_final_exponentiation_device(self.h, gt_layout, c_void_p(d_in), n, c_void_p(d_out),
                                                               c_void_p(d_is_one), ctypes.byref(ms)))
        return ms.value

    def test_fq12_op(self, op, a, b):
        """One raw-limb Fq12 op (MSM_AMD_FQ12_OP_*) on the device: a, b lists of up to FQ12_WORDS u32; returns FQ12_WORDS."""
        out = (c_uint32 * FQ12_WORDS)()
        self._check(_lib().msm_amd_test_fq12_op(self.h, op, _fq12_raw(a), _fq12_raw(b), out))
        return list(out)

    def test_fq12_ops(self, op, a, b, count):
        """count raw-limb Fq12 ops in one launch: a, b flat u32 lists of count * FQ12_WORDS; returns count * FQ12_WORDS."""
        out = (c_uint32 * max(1, count * FQ12_WORDS))()
        self._check(_lib().msm_amd_test_fq12_ops(self.h, op, _fq12_raw(a, count), _fq12_raw(b, count), out, count))
        return list(out)[:count * FQ12_WORDS]

    def test_op_g2(self, op, a, b, count):
        """Raw-limb G2 op (MSM_AMD_G2_RAW_*) on the device: a, b flat u32 lists of count * G2_RAW_IN_WORDS; returns
        count * G2_RAW_OUT_WORDS u32."""
        out = (c_uint32 * (count * G2_RAW_OUT_WORDS))()
        self._check(_lib().msm_amd_test_op_g2(self.h, op, _g2_raw_in(a, count), _g2_raw_in(b, count), out, count))
        return list(out)


def msm_batch_multi(configs, scalars_list, points_list, ns, scalar_layout=SCALAR_MONT_LE,
                    point_layout=POINT_H2C_AFFINE, device=False):
    """The instance loop sharded over several configs (gpu_profiler.rs:101-106): instance j -> configs[j mod G], one
    host thread per config inside the library.  device=True: lists of device pointers (instance j on config j mod G's
    GPU)."""
    k, g = len(ns), len(configs)
    cc = (c_void_p * g)(*[c.h for c in configs])
    if device:
        sp = (c_void_p * k)(*scalars_list)
        pp = (c_void_p * k)(*points_list)
    else:
        sp = (c_void_p * k)(*[ctypes.cast(ctypes.c_char_p(s), c_void_p) for s in scalars_list])
        pp = (c_void_p * k)(*[ctypes.cast(ctypes.c_char_p(p), c_void_p) for p in points_list])
    nn = (c_size_t * k)(*ns)
    out = ctypes.create_string_buffer(96 * k)
    fn = _lib().msm_amd_msm_batch_multi_device if device else _lib().msm_amd_msm_batch_multi
    st = fn(cc, g, scalar_layout, point_layout, k, sp, pp, nn, out)
    if st != OK:
        detail = "; ".join(_lib().msm_amd_last_error(c.h).decode() for c in configs)
        raise MsmError(st, detail)
    return [out.raw[96 * i:96 * i + 96] for i in range(k)]


def submit_batch_multi_device(configs, d_scalars, d_points, ns, scalar_layout=SCALAR_MONT_LE,
                              point_layout=POINT_H2C_AFFINE):
    """Pipelined form of msm_batch_multi(..., device=True): enqueue every config's share, return a handle for
    wait_batch_multi (msm_amd_submit_batch_multi_device)."""
    k, g = len(ns), len(configs)
    cc = (c_void_p * g)(*[c.h for c in configs])
    sp = (c_void_p * k)(*d_scalars)
    pp = (c_void_p * k)(*d_points)
    nn = (c_size_t * k)(*ns)
    out = ctypes.create_string_buffer(96 * k)
    ticket = c_void_p()
    st = _lib().msm_amd_submit_batch_multi_device(cc, g, scalar_layout, point_layout, k, sp, pp, nn, out,
                                                  ctypes.byref(ticket))
    if st != OK:
        raise MsmError(st, "; ".join(_lib().msm_amd_last_error(c.h).decode() for c in configs))
    return (ticket, out, k, configs)


def wait_batch_multi(handle):
    ticket, out, k, configs = handle
    st = _lib().msm_amd_wait_batch_multi(ticket)
    if st != OK:
        raise MsmError(st, "; ".join(_lib().msm_amd_last_error(c.h).decode() for c in configs))
    return [out.raw[96 * i:96 * i + 96] for i in range(k)]


def msm_range_multi(configs, scalars: bytes, points: bytes, n: int, scalar_layout=SCALAR_MONT_LE,
                    point_layout=POINT_H2C_AFFINE) -> bytes:
    """ONE instance split by point range over several configs (msm_amd_msm_range_multi): config g uploads and runs the
    points of msm_amd_shard_range(n, G, g), the partial results are added."""
    g = len(configs)
    cc = (c_void_p * g)(*[c.h for c in configs])
    out = ctypes.create_string_buffer(96)
    st = _lib().msm_amd_msm_range_multi(cc, g, scalar_layout, point_layout, scalars, points, n, out)
    if st != OK:
        raise MsmError(st, "; ".join(_lib().msm_amd_last_error(c.h).decode() for c in configs))
    return out.raw


def shard_range(n: int, n_ctx: int, k: int):
    b, e = c_size_t(0), c_size_t(0)
    _lib().msm_amd_shard_range(n, n_ctx, k, ctypes.byref(b), ctypes.byref(e))
    return b.value, e.value


def shard_owner(instance: int, n_ctx: int) -> int:
    return _lib().msm_amd_shard_owner(instance, n_ctx)


def shard_count(n_inst: int, n_ctx: int, k: int) -> int:
    return _lib().msm_amd_shard_count(n_inst, n_ctx, k)


class RcclGather:
    """RCCL all-gather of per-rank result blocks from C++ (msm_amd_gather_*): one communicator per listed device."""

    def __init__(self, devices):
        self.g = c_void_p()
        arr = (c_int * len(devices))(*devices)
        st = _lib().msm_amd_gather_init(arr, len(devices), ctypes.byref(self.g))
        if st != OK:
            raise MsmError(st, "msm_amd_gather_init")
        self.n = len(devices)

    def all_gather(self, blocks):
        per = len(blocks[0])
        send = (c_void_p * self.n)(*[ctypes.cast(ctypes.c_char_p(b), c_void_p) for b in blocks])
        outs = [ctypes.create_string_buffer(per * self.n) for _ in range(self.n)]
        recv = (c_void_p * self.n)(*[ctypes.cast(o, c_void_p) for o in outs])
        st = _lib().msm_amd_gather_all(self.g, send, per, recv)
        if st != OK:
            raise MsmError(st, _lib().msm_amd_gather_last_error(self.g).decode())
        return [o.raw for o in outs]

    def close(self):
        if self.g:
            _lib().msm_amd_gather_destroy(self.g)
        self.g = None


def host_msm(scalars: bytes, points: bytes, n: int, threads=0, scalar_layout=SCALAR_MONT_LE,
             point_layout=POINT_H2C_AFFINE) -> bytes:
    """The product's CPU MSM (where the reference calls halo2curves::msm::msm_best: gpu_profiler.rs:157-159,
    msm.rs:412) -- host code of the library, no GPU and no ctx needed."""
    out = ctypes.create_string_buffer(96)
    st = _lib().msm_amd_host_msm(scalar_layout, point_layout, scalars, points, n, threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw


def _width_result(call):
    bits = c_uint32(0)
    stats = (c_uint64 * 4)()
    call(ctypes.byref(bits), stats)
    return bits.value, {"zeros": stats[0], "negatives": stats[1], "widest": stats[2]}


def _host_status(st):
    if st != OK:
        raise MsmError(st)


def host_scalar_width(scalars: bytes, n: int, sign=WIDTH_UNSIGNED, scalar_layout=SCALAR_MONT_LE, threads=0):
    """Host twin of MsmConfig.scalar_width."""
    return _width_result(lambda b, st: _host_status(
        _lib().msm_amd_host_scalar_width(scalar_layout, scalars, n, sign, threads, b, st)))


def host_msm_bounded(scalars: bytes, points: bytes, n: int, bits: int, sign=WIDTH_UNSIGNED, threads=0,
                     scalar_layout=SCALAR_MONT_LE, point_layout=POINT_H2C_AFFINE, out=None) -> bytes:
    out = ctypes.create_string_buffer(96) if out is None else out
    _host_status(_lib().msm_amd_host_msm_bounded(scalar_layout, point_layout, scalars, points, n, bits, sign, threads, out))
    return out.raw[:96]


def host_msm_g2_bounded(scalars: bytes, points: bytes, n: int, bits: int, sign=WIDTH_UNSIGNED, threads=0,
                        scalar_layout=SCALAR_MONT_LE, point_layout=G2_POINT_H2C_AFFINE, out=None) -> bytes:
    out = ctypes.create_string_buffer(192) if out is None else out
    _host_status(_lib().msm_amd_host_msm_g2_bounded(scalar_layout, point_layout, scalars, points, n, bits, sign, threads, out))
    return out.raw[:192]


def auto_window_size_bounded(n: int, bits: int, lone=False) -> int:
    return _lib().msm_amd_auto_window_size_bounded(n, bits, 1 if lone else 0)


def generate_instance_host(seed, n, scalars_mont=True, threads=0):
    """(points, scalars) of the deterministic synthetic instance, generated on the host by the library."""
    pts = ctypes.create_string_buffer(64 * n)
    sc = ctypes.create_string_buffer(32 * n)
    st = _lib().msm_amd_generate_instance_host(seed, n, 1 if scalars_mont else 0, pts, sc, threads)
    if st != OK:
        raise MsmError(st)
    return pts.raw, sc.raw


def test_op_host(op, a, b, count):
    """Same single-op bodies as MsmConfig.test_op, executed on the host CPU by the library (no GPU)."""
    per = 24 if op_is_point(op) else 8
    out = (c_uint32 * (count * per))()
    st = _lib().msm_amd_test_op_host(op, _u32buf(a), _u32buf(b), out, count)
    if st != OK:
        raise MsmError(st)
    return list(out)


def _raw_in(seq, count):
    if len(seq) != count * RAW_IN_WORDS:
        raise ValueError(f"a raw-limb operand holds {RAW_IN_WORDS} words per element")
    return _u32buf(seq)


def test_op_raw_host(op, a, b, count):
    """Same raw-limb op bodies as MsmConfig.test_op_raw, executed on the host CPU by the library (no GPU)."""
    out = (c_uint32 * (count * RAW_OUT_WORDS))()
    st = _lib().msm_amd_test_op_raw_host(op, _raw_in(a, count), _raw_in(b, count), out, count)
    if st != OK:
        raise MsmError(st)
    return list(out)


def g2_point_bytes(layout) -> int:
    return _lib().msm_amd_g2_point_bytes(layout)


def host_msm_g2(scalars: bytes, points: bytes, n: int, threads=0, scalar_layout=SCALAR_MONT_LE,
                point_layout=G2_POINT_H2C_AFFINE) -> bytes:
    """The product's CPU G2 MSM (no GPU): 192-byte normalised Jacobian, the form msm_g2 returns."""
    out = ctypes.create_string_buffer(192)
    st = _lib().msm_amd_host_msm_g2(scalar_layout, point_layout, scalars, points, n, threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw


def g2_table_host(points: bytes, n: int, window_size: int, num_windows: int, threads=0,
                  point_layout=G2_POINT_H2C_AFFINE) -> bytes:
    """Host twin of the G2 table build (no GPU): num_windows * n G2_POINT_H2C_AFFINE records, entry (w, i) at
    128 * (w * n + i)."""
    out = ctypes.create_string_buffer(128 * n * num_windows)
    st = _lib().msm_amd_test_g2_table_host(point_layout, points, n, window_size, num_windows, threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw


def g2_progression(start: bytes, step: bytes, n: int, threads=0) -> bytes:
    """n G2 points start + i * step (halo2curves G2Affine records, 128 B each), generated on the host by the library."""
    out = ctypes.create_string_buffer(128 * n)
    st = _lib().msm_amd_test_g2_progression(start, step, n, threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw


def _host_check(fn, points, n, checks, threads, point_layout, want_reasons):
    rep = CheckReport()
    reasons = ctypes.create_string_buffer(max(n, 1)) if want_reasons else None
    st = fn(point_layout, points, n, checks, threads, reasons, ctypes.byref(rep))
    if st != OK:
        raise MsmError(st)
    return rep.as_dict(), (reasons.raw[:n] if want_reasons else None)


def host_check_points(points: bytes, n: int, checks=CHECK_CURVE, threads=0, point_layout=POINT_H2C_AFFINE, reasons=True):
    """Host twin of MsmConfig.check_points (no GPU): (report dict, n reason bytes or None)."""
    return _host_check(_lib().msm_amd_host_check_points, points, n, checks, threads, point_layout, reasons)


def host_g2_check_points(points: bytes, n: int, checks=CHECK_CURVE | CHECK_SUBGROUP, threads=0,
                         point_layout=G2_POINT_H2C_AFFINE, reasons=True):
    """Host twin of MsmConfig.g2_check_points (no GPU)."""
    return _host_check(_lib().msm_amd_host_g2_check_points, points, n, checks, threads, point_layout, reasons)


def compressed_bytes(fmt, group) -> int:
    return _lib().msm_amd_compressed_bytes(fmt, group)


def decompressed_bytes(point_layout, g2=False) -> int:
    """record size of an output layout of the decompression (prepared records included), 0 = not one"""
    if g2:
        return G2_PREPARED_BYTES if point_layout == G2_POINT_PREPARED else G2_POINT_BYTES.get(point_layout, 0)
    return 64 if point_layout == POINT_PREPARED else {POINT_H2C_AFFINE: 64, POINT_ARK_AFFINE: 72}.get(point_layout, 0)


def host_decompress_points(data: bytes, n: int, fmt=COMPRESSED_ARK, point_layout=POINT_H2C_AFFINE, g2=False, threads=0,
                           reasons=True):
    """Host twin of MsmConfig.decompress_points (no GPU): (points bytes, report dict, n reason bytes or None)."""
    fn = _lib().msm_amd_host_g2_decompress_points if g2 else _lib().msm_amd_host_decompress_points
    size = decompressed_bytes(point_layout, g2)
    out = ctypes.create_string_buffer(max(1, n * size))
    rs = ctypes.create_string_buffer(max(n, 1)) if reasons else None
    rep = DecompressReport()
    st = fn(fmt, data, n, point_layout, threads, out, rs, ctypes.byref(rep))
    if st != OK:
        raise MsmError(st)
    return out.raw[:n * size], rep.as_dict(), (rs.raw[:n] if reasons else None)


def host_compress_points(points: bytes, n: int, fmt=COMPRESSED_ARK, point_layout=POINT_H2C_AFFINE, g2=False, threads=0):
    """Host twin of MsmConfig.compress_points (no GPU): (records bytes, n_bad)."""
    fn = _lib().msm_amd_host_g2_compress_points if g2 else _lib().msm_amd_host_compress_points
    size = 64 if g2 else 32
    out = ctypes.create_string_buffer(max(1, n * size))
    bad = c_uint64(0)
    st = fn(point_layout, points, n, fmt, threads, out, ctypes.byref(bad))
    if st != OK:
        raise MsmError(st)
    return out.raw[:n * size], bad.value


def _fq12_raw(words, count=1):
    """count records of FQ12_WORDS u32; one record may be shorter (padded with zeros), a batch must be exact"""
    if count != 1 and len(words) != count * FQ12_WORDS:
        raise ValueError("expected %d words, got %d" % (count * FQ12_WORDS, len(words)))
    return (c_uint32 * max(1, count * FQ12_WORDS))(*words)


def test_fq12_op_host(op, a, b):
    """The same op bodies as MsmConfig.test_fq12_op, on the host CPU (no GPU)."""
    out = (c_uint32 * FQ12_WORDS)()
    st = _lib().msm_amd_test_fq12_op_host(op, _fq12_raw(a), _fq12_raw(b), out)
    if st != OK:
        raise MsmError(st)
    return list(out)


def test_fq12_ops_host(op, a, b, count):
    """The same op bodies as MsmConfig.test_fq12_ops, on the host CPU (no GPU)."""
    out = (c_uint32 * max(1, count * FQ12_WORDS))()
    st = _lib().msm_amd_test_fq12_ops_host(op, _fq12_raw(a, count), _fq12_raw(b, count), out, count)
    if st != OK:
        raise MsmError(st)
    return list(out)[:count * FQ12_WORDS]


def host_pairing_product(g1_points: bytes, g2_points: bytes, n_groups: int, group_size: int, flags=0, gt_layout=GT_MONT_LE,
                         point_layout=POINT_H2C_AFFINE, g2_point_layout=G2_POINT_H2C_AFFINE, threads=0, want_is_one=True):
    """Host twin of MsmConfig.pairing_product (no GPU); returns (records, is_one bytes or None)."""
    out = ctypes.create_string_buffer(max(1, n_groups * GT_BYTES))
    flag = ctypes.create_string_buffer(max(1, n_groups)) if want_is_one and not flags & PAIRING_MILLER_ONLY else None
    st = _lib().msm_amd_host_pairing_product(point_layout, g2_point_layout, g1_points, g2_points, n_groups, group_size,
                                             flags, gt_layout, out, flag, threads)
    if st != OK:
        raise MsmError(st)
    return out.raw[:n_groups * GT_BYTES], (flag.raw[:n_groups] if flag is not None else None)


def host_final_exponentiation(records: bytes, n: int, gt_layout=GT_MONT_LE, threads=0):
    out = ctypes.create_string_buffer(max(1, n * GT_BYTES))
    flag = ctypes.create_string_buffer(max(1, n))
    st = _lib().msm_amd_host_final_exponentiation(gt_layout, records, n, out, flag, threads)
    if st != OK:
        raise MsmError(st)
    return out.raw[:n * GT_BYTES], flag.raw[:n]


def pairing_plan(n_groups: int, group_size: int, pairs_per_lane=0, device_final_from=None) -> dict:
    """msm_amd_test_pairing_plan: the plan of a pairing product as a dict (device_final_from None: the library's default)."""
    out = (c_uint32 * 4)()
    if device_final_from is None:
        device_final_from = 0xFFFFFFFFFFFFFFFF
    st = _lib().msm_amd_test_pairing_plan(n_groups, group_size, pairs_per_lane, device_final_from, out)
    if st != OK:
        raise MsmError(st)
    return dict(zip(("pairs_per_lane", "lanes_per_group", "fold_levels", "final_on_device"), out))


def host_mul_points(scalars: bytes, points: bytes, n: int, base_mode=MUL_BASE_EACH, scalar_layout=SCALAR_MONT_LE,
                    point_layout=POINT_H2C_AFFINE, point_layout_out=POINT_H2C_AFFINE, g2=False, threads=0) -> bytes:
    """Host twin of MsmConfig.mul_points (no GPU)."""
    fn = _lib().msm_amd_host_g2_mul_points if g2 else _lib().msm_amd_host_mul_points
    size = decompressed_bytes(point_layout_out, g2)
    out = ctypes.create_string_buffer(max(1, n * size))
    st = fn(scalar_layout, point_layout, base_mode, scalars, points, n, point_layout_out, threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw[:n * size]


class NttDomain:
    """A transform domain of one MsmConfig (msm_amd_ntt_domain_*)."""

    def __init__(self, cfg, handle):
        self.cfg, self.h = cfg, handle

    def info(self) -> dict:
        root, log_n, nbytes, omega = c_int(0), c_uint32(0), c_size_t(0), ctypes.create_string_buffer(32)
        self.cfg._check(_lib().msm_amd_ntt_domain_info(self.cfg.h, self.h, ctypes.byref(root), ctypes.byref(log_n),
                                                       ctypes.byref(nbytes), omega))
        return {"root": root.value, "log_n": log_n.value, "device_bytes": nbytes.value, "omega": omega.raw}

    def free(self):
        self.cfg._check(_lib().msm_amd_ntt_domain_free(self.cfg.h, self.h))


def _ntt_handle(dom):
    return dom.h if isinstance(dom, NttDomain) else dom


def _ntt_log_n(cfg, dom) -> int:
    """log_n of a domain handle of cfg (an unknown handle raises the MsmError of msm_amd_ntt_domain_info)"""
    log_n = c_uint32(0)
    cfg._check(_lib().msm_amd_ntt_domain_info(cfg.h, _ntt_handle(dom), None, ctypes.byref(log_n), None, None))
    return log_n.value


def _ntt_points_out(log_n, points, point_layout, point_layout_out):
    """(output buffer, its size) of a point transform from host records; a known input layout must come with n records"""
    n = 1 << log_n
    if points is not None and point_layout in POINT_BYTES and len(points) != n * POINT_BYTES[point_layout]:
        raise ValueError(f"ntt_points: {len(points)} bytes are not {n} records of point layout {point_layout}")
    size = n * {POINT_H2C_AFFINE: 64, POINT_ARK_AFFINE: 72}.get(point_layout_out, 0)
    return ctypes.create_string_buffer(max(1, size)), size


def host_ntt(data: bytes, root, log_n, direction=NTT_FORWARD, scalar_layout=SCALAR_MONT_LE, shift=None, n_vec=1,
             threads=0) -> bytes:
    """Host twin of MsmConfig.ntt (no GPU)."""
    out = ctypes.create_string_buffer(max(1, len(data)))
    st = _lib().msm_amd_host_ntt(root, log_n, direction, scalar_layout, shift, data, out, n_vec, threads)
    if st != OK:
        raise MsmError(st)
    return out.raw[:len(data)]


def test_host_ntt_levels(data: bytes, root, log_n, levels, direction=NTT_FORWARD, scalar_layout=SCALAR_MONT_LE, shift=None,
                         n_vec=1, threads=0) -> bytes:
    """host_ntt stopped after `levels` levels (msm_amd_test_host_ntt_levels): the work array as it stands, Montgomery
    residues, no permutation, no scaling."""
    out = ctypes.create_string_buffer(max(1, len(data)))
    st = _lib().msm_amd_test_host_ntt_levels(root, log_n, direction, scalar_layout, shift, data, out, n_vec, levels, threads)
    if st != OK:
        raise MsmError(st)
    return out.raw[:len(data)]


def host_ntt_points(points: bytes, root, log_n, direction=NTT_FORWARD, point_layout=POINT_H2C_AFFINE,
                    point_layout_out=POINT_H2C_AFFINE, threads=0) -> bytes:
    """Host twin of MsmConfig.ntt_points (no GPU)."""
    if not 0 <= log_n <= 28:
        raise MsmError(INPUT_ERROR)
    out, size = _ntt_points_out(log_n, points, point_layout, point_layout_out)
    st = _lib().msm_amd_host_ntt_points(root, log_n, direction, point_layout, points, point_layout_out, out, threads)
    if st != OK:
        raise MsmError(st)
    return out.raw[:size]


def test_host_ntt_points_levels(points: bytes, root, log_n, levels, direction=NTT_FORWARD, point_layout=POINT_H2C_AFFINE,
                                point_layout_out=POINT_H2C_AFFINE, threads=0) -> bytes:
    """host_ntt_points stopped after `levels` levels (msm_amd_test_host_ntt_points_levels): the work array as affine
    records in network order, no final scaling."""
    if not 0 <= log_n <= 28:
        raise MsmError(INPUT_ERROR)
    out, size = _ntt_points_out(log_n, points, point_layout, point_layout_out)
    st = _lib().msm_amd_test_host_ntt_points_levels(root, log_n, direction, point_layout, points, levels, point_layout_out,
                                                    out, threads)
    if st != OK:
        raise MsmError(st)
    return out.raw[:size]


def test_ntt_plan(log_n, tile_log=10) -> list:
    """The passes of a transform (msm_amd_test_ntt_plan): one dict of level0, levels, sigma, low per pass."""
    out = (c_uint32 * (1 + 4 * 28))()
    st = _lib().msm_amd_test_ntt_plan(log_n, tile_log, out)
    if st != OK:
        raise MsmError(st)
    return [dict(zip(("level0", "levels", "sigma", "low"), out[1 + 4 * k:5 + 4 * k])) for k in range(out[0])]


def test_ntt_slots(log_n, tile_log, pass_index, wg) -> list:
    """The flat element index of every slot of workgroup wg in one pass (msm_amd_test_ntt_slots: ntt_slot_index)."""
    out = (c_uint64 * (1 << min(max(tile_log, 0), 10)))()
    st = _lib().msm_amd_test_ntt_slots(log_n, tile_log, pass_index, wg, out)
    if st != OK:
        raise MsmError(st)
    return list(out)


class FrMatrix:
    """A sparse matrix over Fr of one MsmConfig (msm_amd_fr_matrix_*)."""

    def __init__(self, cfg, handle):
        self.cfg, self.h = cfg, handle

    def info(self) -> dict:
        return _fr_matrix_info(self.cfg, self.h)

    def free(self):
        self.cfg._check(_lib().msm_amd_fr_matrix_free(self.cfg.h, self.h))


def _fr_matrix_handle(mat):
    return mat.h if isinstance(mat, (FrMatrix, NttDomain)) else mat


def _fr_matrix_info(cfg, handle) -> dict:
    out = [c_size_t(0) for _ in range(5)]
    cfg._check(_lib().msm_amd_fr_matrix_info(cfg.h, handle, *[ctypes.byref(v) for v in out]))
    return dict(zip(("n_rows", "n_cols", "nnz", "n_distinct", "device_bytes"), (v.value for v in out)))


def _csr_u64(seq):
    """row offsets for the C side: packed bytes as they are, a sequence as a u64 array, None as null"""
    if seq is None or isinstance(seq, (bytes, bytearray)):
        return seq if seq is None else bytes(seq)
    return (c_uint64 * len(seq))(*seq)


def _csr_u32(seq):
    if seq is None or isinstance(seq, (bytes, bytearray)):
        return seq if seq is None else bytes(seq)
    return (c_uint32 * max(1, len(seq)))(*seq)


def host_fr_matvec(n_rows, n_cols, row_ptr, col_idx, values: bytes, x: bytes, scalar_layout=SCALAR_MONT_LE, threads=0,
                   y=None) -> bytes:
    """Host twin of MsmConfig.fr_matrix_build + fr_matvec (no GPU); y: a ctypes buffer to write into (argument tests)"""
    out = ctypes.create_string_buffer(max(1, 32 * n_rows)) if y is None else y
    st = _lib().msm_amd_host_fr_matvec(scalar_layout, n_rows, n_cols, _csr_u64(row_ptr), _csr_u32(col_idx), values, x,
                                       threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw[:32 * n_rows] if y is None else None


def test_fr_matrix_plan(row_ptr, long_rows=32, seg_log=8, segs_cap=0) -> dict:
    """The plan of a matrix with these row offsets (msm_amd_test_fr_matrix_plan): the counts by name, and `segs`, the
    first segs_cap segment records as (row, first, count, slot) with slot None for a row of one segment."""
    n_rows = (len(row_ptr) // 8 if isinstance(row_ptr, (bytes, bytearray)) else len(row_ptr)) - 1
    counts = (c_uint64 * 8)()
    segs = (c_uint32 * (4 * max(1, segs_cap)))()
    st = _lib().msm_amd_test_fr_matrix_plan(n_rows, _csr_u64(row_ptr), long_rows, seg_log, counts, segs, segs_cap)
    if st != OK:
        raise MsmError(st)
    plan = dict(zip(("lane_rows", "wave_rows", "segments", "split_rows", "partials", "launches", "waves"), counts))
    take = min(segs_cap, plan["segments"])
    plan["segs"] = [(segs[4 * k], segs[4 * k + 1], segs[4 * k + 2], None if segs[4 * k + 3] == 0xFFFFFFFF else segs[4 * k + 3])
                    for k in range(take)]
    return plan


def host_fr_map(op, a: bytes, b: bytes = None, c: bytes = None, k: bytes = None, scalar_layout=SCALAR_MONT_LE,
                threads=0) -> bytes:
    """Host twin of MsmConfig.fr_map (no GPU)."""
    n = len(a) // 32 if a is not None else 0
    out = ctypes.create_string_buffer(max(1, 32 * n))
    st = _lib().msm_amd_host_fr_map(op, scalar_layout, k, a, b, c, n, threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw[:32 * n]


def host_fr_batch_inverse(data: bytes, scalar_layout=SCALAR_MONT_LE, threads=0):
    """Host twin of MsmConfig.fr_batch_inverse (no GPU): (records, n_zero)."""
    n, zeros = len(data) // 32, c_uint64(0)
    out = ctypes.create_string_buffer(max(1, len(data)))
    st = _lib().msm_amd_host_fr_batch_inverse(scalar_layout, data, n, threads, out, ctypes.byref(zeros))
    if st != OK:
        raise MsmError(st)
    return out.raw[:32 * n], zeros.value


def host_fr_prefix_product(data: bytes, mode=FR_PREFIX_INCLUSIVE, scalar_layout=SCALAR_MONT_LE, n_vec=1, threads=0) -> bytes:
    """Host twin of MsmConfig.fr_prefix_product (no GPU)."""
    n = len(data) // 32 // n_vec if n_vec else 0
    out = ctypes.create_string_buffer(max(1, len(data)))
    st = _lib().msm_amd_host_fr_prefix_product(scalar_layout, mode, data, n, n_vec, threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw[:32 * n * n_vec]


def host_fr_prefix_sum(data: bytes, mode=FR_PREFIX_INCLUSIVE, scalar_layout=SCALAR_MONT_LE, n_vec=1, threads=0) -> bytes:
    """Host twin of MsmConfig.fr_prefix_sum (no GPU)."""
    n = len(data) // 32 // n_vec if n_vec else 0
    out = ctypes.create_string_buffer(max(1, len(data)))
    st = _lib().msm_amd_host_fr_prefix_sum(scalar_layout, mode, data, n, n_vec, threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw[:32 * n * n_vec]


def host_fr_shift(a: bytes, k: bytes, scalar_layout=SCALAR_MONT_LE, threads=0) -> bytes:
    """Host twin of MsmConfig.fr_shift (no GPU)."""
    n = len(a) // 32 if a is not None else 0
    out = ctypes.create_string_buffer(max(1, 32 * n))
    st = _lib().msm_amd_host_fr_shift(scalar_layout, k, a, n, threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw[:32 * n]


class FrLookup:
    """A lookup table over Fr of one MsmConfig (msm_amd_fr_lookup_*)."""

    def __init__(self, cfg, handle):
        self.cfg, self.h, self.build_ms = cfg, handle, None

    def info(self) -> dict:
        return _fr_lookup_info(self.cfg, self.h)

    def free(self):
        self.cfg._check(_lib().msm_amd_fr_lookup_free(self.cfg.h, self.h))


def _fr_lookup_handle(table):
    return table.h if isinstance(table, (FrLookup, FrMatrix, NttDomain)) else table


def _fr_lookup_info(cfg, handle) -> dict:
    out = [c_size_t(0) for _ in range(5)]
    cfg._check(_lib().msm_amd_fr_lookup_info(cfg.h, handle, *[ctypes.byref(v) for v in out]))
    return dict(zip(("n_rows", "n_distinct", "capacity", "device_bytes", "longest_probe"), (v.value for v in out)))


LOOKUP_REPORT_FIELDS = ("n_missing", "first_missing", "rows_hit", "max_multiplicity")


def _lookup_result(cfg, st, m, n_rows, idx, total, rep):
    """(m bytes or None, idx list or None, report dict) of a multiplicities call; a failed call raises MsmError, with
    .report and .idx set when the failure is a miss under LOOKUP_STRICT"""
    report = dict(zip(LOOKUP_REPORT_FIELDS, rep))
    idx_list = list(idx[:total]) if idx is not None else None
    if st != OK:
        err = MsmError(st, _lib().msm_amd_last_error(cfg.h).decode() if cfg is not None else "")
        err.report, err.idx = report, idx_list
        raise err
    return (m.raw[:32 * n_rows] if m is not None else None), idx_list, report


def host_fr_lookup_multiplicities(table: bytes, data: bytes, on_missing=LOOKUP_STRICT, scalar_layout=SCALAR_MONT_LE, n_vec=1,
                                  threads=0, want_idx=True, m_out=None):
    """Host twin of MsmConfig.fr_lookup_build + fr_lookup_multiplicities (no GPU): (m, idx or None, report); m_out: a ctypes
    buffer to write into (then m is None)."""
    n_rows = len(table) // 32
    n = len(data) // 32 // n_vec if n_vec else 0
    m = ctypes.create_string_buffer(max(1, 32 * n_rows)) if m_out is None else m_out
    idx = (c_uint32 * max(1, n * n_vec))() if want_idx else None
    rep = (c_uint64 * 4)()
    st = _lib().msm_amd_host_fr_lookup_multiplicities(scalar_layout, on_missing, table, n_rows, data, n, n_vec, threads, m, idx,
                                                      rep)
    return _lookup_result(None, st, m if m_out is None else None, n_rows, idx, n * n_vec, rep)


def test_fr_lookup_plan(n_rows, hash_bits=32) -> dict:
    """The index of a table of n_rows (msm_amd_test_fr_lookup_plan)"""
    out = (c_uint64 * 4)()
    st = _lib().msm_amd_test_fr_lookup_plan(n_rows, hash_bits, out)
    if st != OK:
        raise MsmError(st)
    return dict(zip(("capacity", "bytes", "home_bits", "slots_off"), out))


def _permute_buffers(total, want_a, want_s, a_out, s_out):
    a = a_out if a_out is not None else ctypes.create_string_buffer(max(1, 32 * total)) if want_a else None
    s = s_out if s_out is not None else ctypes.create_string_buffer(max(1, 32 * total)) if want_s else None
    return a, s


def _permute_result(cfg, st, a, s, total, rep):
    """(A' bytes or None, S' bytes or None, report dict) of a permute call; a failed call raises MsmError with .report set"""
    report = dict(zip(LOOKUP_REPORT_FIELDS, rep))
    if st != OK:
        err = MsmError(st, _lib().msm_amd_last_error(cfg.h).decode() if cfg is not None else "")
        err.report = report
        raise err
    return (a.raw[:32 * total] if a is not None else None), (s.raw[:32 * total] if s is not None else None), report


def host_fr_lookup_permute(table: bytes, data: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1, threads=0, want_a=True,
                           want_s=True, a_out=None, s_out=None):
    """Host twin of MsmConfig.fr_lookup_build + fr_lookup_permute (no GPU): (A', S', report)"""
    n_rows = len(table) // 32
    n = len(data) // 32 // n_vec if n_vec else 0
    a, s = _permute_buffers(n * n_vec, want_a, want_s, a_out, s_out)
    rep = (c_uint64 * 4)()
    st = _lib().msm_amd_host_fr_lookup_permute(scalar_layout, table, n_rows, data, n, n_vec, threads, a, s, rep)
    return _permute_result(None, st, a if a_out is None else None, s if s_out is None else None, n * n_vec, rep)


def host_fr_lookup_permute_as(table: bytes, data: bytes, arrangement=PERMUTE_HALO2, scalar_layout=SCALAR_MONT_LE, n_vec=1,
                              threads=0, want_a=True, want_s=True, a_out=None, s_out=None):
    """Host twin of MsmConfig.fr_lookup_build_sorted + fr_lookup_permute_as (no GPU): (A', S', report)"""
    n_rows = len(table) // 32
    n = len(data) // 32 // n_vec if n_vec else 0
    a, s = _permute_buffers(n * n_vec, want_a, want_s, a_out, s_out)
    rep = (c_uint64 * 4)()
    st = _lib().msm_amd_host_fr_lookup_permute_as(scalar_layout, arrangement, table, n_rows, data, n, n_vec, threads, a, s, rep)
    return _permute_result(None, st, a if a_out is None else None, s if s_out is None else None, n * n_vec, rep)


def test_fr_permute_plan(n_rows, n_vec=1, tile_log=11) -> dict:
    """The plan of a permute call (msm_amd_test_fr_permute_plan)"""
    out = (c_uint64 * 4)()
    st = _lib().msm_amd_test_fr_permute_plan(n_rows, n_vec, tile_log, out)
    if st != OK:
        raise MsmError(st)
    return dict(zip(("levels", "launches", "tiles", "bytes"), out))


def host_fr_sort(data, scalar_layout=SCALAR_MONT_LE, n_vec=1, threads=0, n=None, out=None, perm_out=None, want_out=True,
                 want_perm=True):
    """Host twin of MsmConfig.fr_sort (no GPU): (records or None, perm as a list or None)"""
    if n is None:
        n = len(data) // 32 // n_vec if n_vec else 0
    o = out if out is not None else ctypes.create_string_buffer(max(1, 32 * n * n_vec)) if want_out else None
    p = perm_out if perm_out is not None else (c_uint32 * max(1, n * n_vec))() if want_perm else None
    st = _lib().msm_amd_host_fr_sort(scalar_layout, data, n, n_vec, threads, o, p)
    if st != OK:
        raise MsmError(st)
    return (o.raw[:32 * n * n_vec] if o is not None and out is None else None,
            list(p[:n * n_vec]) if p is not None and perm_out is None else None)


def test_fr_sort_plan(n, n_vec=1, digit_mask=0) -> dict:
    """The plan of a sort whose keys differ in the bytes of digit_mask (msm_amd_test_fr_sort_plan)"""
    out = (c_uint64 * 4)()
    st = _lib().msm_amd_test_fr_sort_plan(n, n_vec, digit_mask, out)
    if st != OK:
        raise MsmError(st)
    return dict(zip(("passes", "launches", "tiles", "bytes"), out))


def host_fr_poly_eval(coeffs: bytes, z: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1, threads=0) -> bytes:
    """Host twin of MsmConfig.fr_poly_eval (no GPU)."""
    n = len(coeffs) // 32 // n_vec if n_vec else 0
    y = ctypes.create_string_buffer(max(1, 32 * n_vec))
    st = _lib().msm_amd_host_fr_poly_eval(scalar_layout, z, coeffs, n, n_vec, threads, y)
    if st != OK:
        raise MsmError(st)
    return y.raw[:32 * n_vec] if n else b""


def host_fr_poly_div_linear(data: bytes, z: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1, threads=0):
    """Host twin of MsmConfig.fr_poly_div_linear (no GPU): (quotients, remainders)."""
    n = len(data) // 32 // n_vec if n_vec else 0
    out = ctypes.create_string_buffer(max(1, len(data)))
    rem = ctypes.create_string_buffer(max(1, 32 * n_vec))
    st = _lib().msm_amd_host_fr_poly_div_linear(scalar_layout, z, data, n, n_vec, threads, out, rem)
    if st != OK:
        raise MsmError(st)
    return out.raw[:32 * n * n_vec], (rem.raw[:32 * n_vec] if n else b"")


def host_fr_poly_eval_points(coeffs: bytes, z: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1, threads=0) -> bytes:
    """Host twin of MsmConfig.fr_poly_eval_points (no GPU): the n_vec k records y[v k + j]."""
    k = len(z) // 32
    n = len(coeffs) // 32 // n_vec if n_vec else 0
    y = ctypes.create_string_buffer(max(1, 32 * n_vec * k))
    st = _lib().msm_amd_host_fr_poly_eval_points(scalar_layout, z, k, coeffs, n, n_vec, threads, y)
    if st != OK:
        raise MsmError(st)
    return y.raw[:32 * n_vec * k] if n else b""


def host_fr_poly_div_points(data: bytes, z: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1, threads=0):
    """Host twin of MsmConfig.fr_poly_div_points (no GPU), k chained divisions: (quotients, values)."""
    k = len(z) // 32
    n = len(data) // 32 // n_vec if n_vec else 0
    out = ctypes.create_string_buffer(max(1, len(data)))
    val = ctypes.create_string_buffer(max(1, 32 * n_vec * k))
    st = _lib().msm_amd_host_fr_poly_div_points(scalar_layout, z, k, data, n, n_vec, threads, out, val)
    if st != OK:
        raise MsmError(st)
    return out.raw[:32 * n * n_vec], (val.raw[:32 * n_vec * k] if n else b"")


def test_fr_poly_points_plan(n, n_vec=1, k=1, tile_log=9, divide=True) -> dict:
    """The plan of a multi-point evaluation or division (msm_amd_test_fr_poly_points_plan): launches (those of one point),
    waves over all launches, records and bytes of ctx-owned device memory, levels, bytes of the kernel arguments of a
    level-0 launch, waves of the level-0 launches."""
    out = (c_uint64 * 8)()
    st = _lib().msm_amd_test_fr_poly_points_plan(n, n_vec, k, tile_log, 1 if divide else 0, out)
    if st != OK:
        raise MsmError(st)
    return dict(zip(("launches", "waves", "records", "bytes", "levels", "arg_bytes", "level0_waves"), out))


def host_fr_lincomb(data: bytes, k: bytes, scalar_layout=SCALAR_MONT_LE, n_vec=1, threads=0) -> bytes:
    """Host twin of MsmConfig.fr_lincomb (no GPU)."""
    n = len(data) // 32 // n_vec if n_vec else 0
    out = ctypes.create_string_buffer(max(1, 32 * n))
    st = _lib().msm_amd_host_fr_lincomb(scalar_layout, k, data, n, n_vec, threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw[:32 * n]


class PoseidonParams:
    """The constants of one Poseidon instance of one MsmConfig (msm_amd_poseidon_params_*)."""

    def __init__(self, cfg, handle):
        self.cfg, self.h = cfg, handle

    def info(self) -> dict:
        t, r_f, r_p, nbytes = c_uint32(0), c_uint32(0), c_uint32(0), c_size_t(0)
        self.cfg._check(_lib().msm_amd_poseidon_params_info(self.cfg.h, self.h, ctypes.byref(t), ctypes.byref(r_f),
                                                            ctypes.byref(r_p), ctypes.byref(nbytes)))
        return {"t": t.value, "r_f": r_f.value, "r_p": r_p.value, "device_bytes": nbytes.value}

    def free(self):
        self.cfg._check(_lib().msm_amd_poseidon_params_free(self.cfg.h, self.h))


POSEIDON_R_P = {2: 56, 3: 57, 4: 56, 5: 60}   # circomlib's partial rounds at r_f = 8


def _poseidon_handle(params):
    return params.h if isinstance(params, PoseidonParams) else params


def _poseidon_t(cfg, params) -> int:
    """t of a handle, to size a host output; 0 for what is no handle: the call itself then reports it"""
    t = c_uint32(0)
    st = _lib().msm_amd_poseidon_params_info(cfg.h, _poseidon_handle(params), ctypes.byref(t), None, None, None)
    return t.value if st == OK else 0


def merkle_depth(t, n_leaves) -> int:
    """d with n_leaves = (t - 1)^d, d >= 1; 0 if there is none"""
    a, d = t - 1, 0
    if a < 2 or n_leaves < a:
        return 0
    while n_leaves > 1:
        if n_leaves % a:
            return 0
        n_leaves, d = n_leaves // a, d + 1
    return d


def merkle_nodes(t, n_leaves) -> int:
    """inner nodes of the tree msm_amd_poseidon_merkle_build* write (0 for a count that is no power of the arity)"""
    return (n_leaves - 1) // (t - 2) if merkle_depth(t, n_leaves) else 0


def merkle_path_records(t, n_leaves) -> int:
    """sibling records per leaf index of msm_amd_poseidon_merkle_paths*"""
    return merkle_depth(t, n_leaves) * (t - 2)


def poseidon_constants(t, r_f=8, r_p=None, scalar_layout=SCALAR_MONT_LE):
    """(ark, mds) of the reference generator (msm_amd_poseidon_constants): circomlib's at the default rounds"""
    r_p = POSEIDON_R_P.get(t, 0) if r_p is None else r_p
    ok = 2 <= t <= 5 and 0 <= r_f + r_p <= 128
    ark = ctypes.create_string_buffer(max(1, 32 * (r_f + r_p) * t if ok else 1))
    mds = ctypes.create_string_buffer(max(1, 32 * t * t if ok else 1))
    st = _lib().msm_amd_poseidon_constants(t, r_f, r_p, scalar_layout, ark, mds)
    if st != OK:
        raise MsmError(st)
    return ark.raw[:32 * (r_f + r_p) * t], mds.raw[:32 * t * t]


def host_poseidon_permute(t, r_f, r_p, ark: bytes, mds: bytes, data: bytes, n: int, scalar_layout=SCALAR_MONT_LE,
                          threads=0) -> bytes:
    """Host twin of MsmConfig.poseidon_permute (no GPU)."""
    out = ctypes.create_string_buffer(max(1, 32 * n * t))
    st = _lib().msm_amd_host_poseidon_permute(t, r_f, r_p, scalar_layout, ark, mds, data, n, threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw[:32 * n * t]


def host_poseidon_hash(t, r_f, r_p, ark: bytes, mds: bytes, data: bytes, n: int, scalar_layout=SCALAR_MONT_LE, tag: bytes = None,
                       threads=0) -> bytes:
    """Host twin of MsmConfig.poseidon_hash (no GPU)."""
    out = ctypes.create_string_buffer(max(1, 32 * n))
    st = _lib().msm_amd_host_poseidon_hash(t, r_f, r_p, scalar_layout, ark, mds, tag, data, n, threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw[:32 * n]


def host_poseidon_merkle_build(t, r_f, r_p, ark: bytes, mds: bytes, leaves: bytes, n_leaves: int, scalar_layout=SCALAR_MONT_LE,
                               tag: bytes = None, threads=0):
    """Host twin of MsmConfig.poseidon_merkle_build (no GPU): (tree, root)."""
    nodes = merkle_nodes(t, n_leaves) if t >= 3 else 0
    tree, root = ctypes.create_string_buffer(max(1, 32 * nodes)), ctypes.create_string_buffer(32)
    st = _lib().msm_amd_host_poseidon_merkle_build(t, r_f, r_p, scalar_layout, ark, mds, tag, leaves, n_leaves, threads, tree, root)
    if st != OK:
        raise MsmError(st)
    return tree.raw[:32 * nodes], root.raw


def host_poseidon_merkle_paths(t, leaves: bytes, n_leaves: int, tree: bytes, idx, scalar_layout=SCALAR_MONT_LE,
                               threads=0) -> bytes:
    """Host twin of MsmConfig.poseidon_merkle_paths (no GPU)."""
    size = 32 * len(idx) * (merkle_path_records(t, n_leaves) if t >= 3 else 0)
    out = ctypes.create_string_buffer(max(1, size))
    st = _lib().msm_amd_host_poseidon_merkle_paths(t, scalar_layout, leaves, n_leaves, tree, _csr_u64(idx), len(idx), threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw[:size]


def test_poseidon_plan(t, n_leaves, top_log=8) -> dict:
    """The launches of a tree build (msm_amd_test_poseidon_plan)"""
    out = (c_uint64 * 40)()
    st = _lib().msm_amd_test_poseidon_plan(t, n_leaves, top_log, out)
    if st != OK:
        raise MsmError(st)
    return {"launches": out[0], "depth": out[1], "nodes": out[2], "tail_levels": out[3], "tail_nodes": out[4],
            "per_launch": list(out[8:8 + out[0]])}


def sumcheck_values(form, n_vec) -> int:
    """d + 1 of a round: the records msm_amd_fr_sumcheck_round* return (0 when there is nothing to do)"""
    return 0 if n_vec == 0 else 4 if form == SUMCHECK_EQ_AB_C else n_vec + 1


def host_fr_mle_bind(data: bytes, r: bytes, n: int, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, n_vec=1, stride=None,
                     threads=0, out: bytes = None) -> bytes:
    """Host twin of MsmConfig.fr_mle_bind (no GPU)."""
    stride = n if stride is None else stride
    span = 32 * ((n_vec - 1) * stride + n // 2) if n_vec else 0
    size = len(out) if out is not None else span
    buf = ctypes.create_string_buffer(out if out is not None else b"\xFF" * span, size + 1)
    st = _lib().msm_amd_host_fr_mle_bind(scalar_layout, order, r, len(r) // 32 if r else 0, data, n, n_vec, stride, threads, buf)
    if st != OK:
        raise MsmError(st)
    return buf.raw[:size]


def host_fr_mle_eval(data: bytes, point: bytes, n: int, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, n_vec=1, stride=None,
                     threads=0) -> bytes:
    """Host twin of MsmConfig.fr_mle_eval (no GPU)."""
    y = ctypes.create_string_buffer(max(1, 32 * n_vec))
    st = _lib().msm_amd_host_fr_mle_eval(scalar_layout, order, point, data, n, n_vec, n if stride is None else stride,
                                         threads, y)
    if st != OK:
        raise MsmError(st)
    return y.raw[:32 * n_vec]


def host_fr_eq_table(point: bytes, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, threads=0, m=None) -> bytes:
    """Host twin of MsmConfig.fr_eq_table (no GPU)."""
    m = (len(point) // 32 if point else 0) if m is None else m
    out = ctypes.create_string_buffer(max(1, 32 << m if 0 < m < 32 else 1))
    st = _lib().msm_amd_host_fr_eq_table(scalar_layout, order, point, m, threads, out)
    if st != OK:
        raise MsmError(st)
    return out.raw[:32 << m]


def host_fr_sumcheck_round(data: bytes, n: int, form=SUMCHECK_PRODUCT, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, n_vec=1,
                           stride=None, threads=0) -> bytes:
    """Host twin of MsmConfig.fr_sumcheck_round (no GPU)."""
    g = ctypes.create_string_buffer(32 * 5)
    st = _lib().msm_amd_host_fr_sumcheck_round(scalar_layout, order, form, data, n, n_vec, n if stride is None else stride,
                                               threads, g)
    if st != OK:
        raise MsmError(st)
    return g.raw[:32 * sumcheck_values(form, n_vec)]


class _SumcheckTermsC(ctypes.Structure):
    _fields_ = [("n_terms", c_uint32), ("outer", c_uint32), ("coeff", c_void_p), ("term_len", POINTER(c_uint32)),
                ("factors", POINTER(c_uint32))]


class SumcheckTerms:
    """A term list F = [f_outer] sum_k c_k prod_j f_(factors[k][j]) for the *_terms calls (msm_amd_fr_sumcheck_terms):
    `terms` is a sequence of (coefficient record of 32 bytes in the call's layout, sequence of table indices)."""

    def __init__(self, terms, outer=None):
        terms = list(terms)
        self.coeff = ctypes.create_string_buffer(b"".join(c for c, _ in terms), max(1, 32 * len(terms)))
        self.term_len = (c_uint32 * max(1, len(terms)))(*[len(f) for _, f in terms])
        flat = [i for _, f in terms for i in f]
        self.factors = (c_uint32 * max(1, len(flat)))(*flat)
        self.c = _SumcheckTermsC(len(terms), SUMCHECK_NO_OUTER if outer is None else outer,
                                 ctypes.cast(self.coeff, c_void_p), self.term_len, self.factors)


def _terms_ptr(terms):
    return None if terms is None else ctypes.addressof(terms.c)


def sumcheck_terms_degree(terms, n_vec) -> int:
    """The degree d of a round over `terms` and n_vec tables (msm_amd_fr_sumcheck_terms_degree: the shared check of a list)"""
    d = c_uint32(0)
    st = _lib().msm_amd_fr_sumcheck_terms_degree(_terms_ptr(terms), n_vec, ctypes.byref(d))
    if st != OK:
        raise MsmError(st)
    return d.value


def sumcheck_terms_values(terms, n_vec) -> int:
    """d + 1 of a round over a term list: the records the *_terms calls return (0 when there is nothing to do)"""
    return 0 if n_vec == 0 else sumcheck_terms_degree(terms, n_vec) + 1


def host_fr_sumcheck_round_terms(data: bytes, n: int, terms, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, n_vec=1, stride=None,
                                 threads=0) -> bytes:
    """Host twin of MsmConfig.fr_sumcheck_round_terms (no GPU)."""
    g = ctypes.create_string_buffer(32 * 8)
    st = _lib().msm_amd_host_fr_sumcheck_round_terms(scalar_layout, order, _terms_ptr(terms), data, n, n_vec,
                                                     n if stride is None else stride, threads, g)
    if st != OK:
        raise MsmError(st)
    return g.raw[:32 * sumcheck_terms_values(terms, n_vec)]


def host_fr_sumcheck_step_terms(data: bytes, r: bytes, n: int, terms, order=MLE_LOW, scalar_layout=SCALAR_MONT_LE, n_vec=1,
                                stride=None, threads=0, out: bytes = None):
    """Host twin of MsmConfig.fr_sumcheck_step_terms (no GPU); out == "in place": the call runs on one buffer (MLE_HIGH)."""
    stride = n if stride is None else stride
    span = 32 * ((n_vec - 1) * stride + n // 2) if n_vec else 0
    g = ctypes.create_string_buffer(32 * 8)
    if out == "in place":
        buf = ctypes.create_string_buffer(data, len(data) + 1)
        size, src = len(data), buf
    else:
        size = len(out) if out is not None else span
        buf = ctypes.create_string_buffer(out if out is not None else b"\xFF" * span, size + 1)
        src = data
    st = _lib().msm_amd_host_fr_sumcheck_step_terms(scalar_layout, order, _terms_ptr(terms), r, src, n, n_vec, stride, threads,
                                                    buf, g)
    if st != OK:
        raise MsmError(st)
    return buf.raw[:size], g.raw[:32 * sumcheck_terms_values(terms, n_vec)]


def test_fr_sumcheck_terms_plan(terms, n, n_vec=1, chunk_log=8, step=False) -> dict:
    """The plan of a *_terms call (msm_amd_test_fr_sumcheck_terms_plan); step: msm_amd_fr_sumcheck_step_terms at n."""
    out = (c_uint64 * 8)()
    st = _lib().msm_amd_test_fr_sumcheck_terms_plan(_terms_ptr(terms), n, n_vec, chunk_log, int(step), out)
    if st != OK:
        raise MsmError(st)
    return dict(zip(("launches", "waves", "records", "bytes", "levels", "first_waves", "values"), out))


class _GateTermsC(ctypes.Structure):
    _fields_ = [("n_terms", c_uint32), ("coeff", c_void_p), ("term_len", POINTER(c_uint32)), ("factors", POINTER(c_uint32)),
                ("rotations", POINTER(ctypes.c_int32))]


class GateTerms:
    """A gate polynomial sum_k c_k prod_j col_(index)[i + rotation rot_step] for msm_amd_fr_gate_eval
    (msm_amd_fr_gate_terms): `terms` is a sequence of (coefficient record of 32 bytes in the call's layout, sequence of
    factors), a factor being a column index or a (column index, rotation) pair."""

    def __init__(self, terms):
        terms = [(c, [f if isinstance(f, tuple) else (f, 0) for f in fs]) for c, fs in terms]
        self.coeff = ctypes.create_string_buffer(b"".join(c for c, _ in terms), max(1, 32 * len(terms)))
        self.term_len = (c_uint32 * max(1, len(terms)))(*[len(f) for _, f in terms])
        flat = [f for _, fs in terms for f in fs]
        self.factors = (c_uint32 * max(1, len(flat)))(*[col for col, _ in flat])
        self.rotations = (ctypes.c_int32 * max(1, len(flat)))(*[rot for _, rot in flat])
        self.c = _GateTermsC(len(terms), ctypes.cast(self.coeff, c_void_p), self.term_len, self.factors, self.rotations)


def fr_gate_last_error() -> str:
    """Why the last fr_gate_check, host_fr_gate_eval or test_fr_gate_plan of this thread refused (msm_amd_fr_gate_last_error)"""
    return _lib().msm_amd_fr_gate_last_error().decode()


def fr_gate_check(terms, n_vec, n, rot_step=1):
    """The shared check of a GateTerms list (msm_amd_fr_gate_check): (degree, distinct offsets); MsmError with the reason."""
    d, k = c_uint32(0), c_uint32(0)
    st = _lib().msm_amd_fr_gate_check(_terms_ptr(terms), n_vec, n, rot_step, ctypes.byref(d), ctypes.byref(k))
    if st != OK:
        raise MsmError(st, fr_gate_last_error())
    return d.value, k.value


def host_fr_gate_eval(columns: bytes, terms, n=None, n_vec=1, stride=None, rot_step=1, flags=0, k_acc: bytes = None,
                      scale: bytes = None, out: bytes = None, scalar_layout=SCALAR_MONT_LE, threads=0) -> bytes:
    """Host twin of MsmConfig.fr_gate_eval with MEM_HOST (no GPU): the n records."""
    if n is None:
        n = len(columns) // 32 // n_vec if n_vec else 0
    buf = ctypes.create_string_buffer(out if out is not None else b"\xFF" * (32 * n), 32 * n + 1)
    st = _lib().msm_amd_host_fr_gate_eval(scalar_layout, flags, _terms_ptr(terms), columns, n, n_vec,
                                          n if stride is None else stride, rot_step, k_acc, scale,
                                          len(scale) // 32 if scale is not None else 0, threads, buf)
    if st != OK:
        raise MsmError(st, fr_gate_last_error())
    return buf.raw[:32 * n]


def test_fr_gate_plan(terms, n, n_vec=1, rot_step=1, flags=0, period=0, scalar_layout=SCALAR_MONT_LE) -> dict:
    """The plan of an fr_gate_eval call (msm_amd_test_fr_gate_plan); period 0: no scale."""
    out = (c_uint64 * 8)()
    st = _lib().msm_amd_test_fr_gate_plan(scalar_layout, flags, _terms_ptr(terms), n, n_vec, rot_step, period, out)
    if st != OK:
        raise MsmError(st, fr_gate_last_error())
    return dict(zip(("launches", "workgroups", "reads", "products", "offsets", "bytes", "degree"), out))


def test_fr_mle_plan(call, n, n_vec=1, order=MLE_LOW, form=SUMCHECK_PRODUCT, n_bind=1, chunk_log=8, tile_log=9) -> dict:
    """The plan of a multilinear call (msm_amd_test_fr_mle_plan); call: MLE_CALL_*; for the eq table n is m."""
    out = (c_uint64 * 8)()
    st = _lib().msm_amd_test_fr_mle_plan(call, order, form, n, n_vec, n_bind, chunk_log, tile_log, out)
    if st != OK:
        raise MsmError(st)
    return dict(zip(("launches", "waves", "records", "bytes", "levels", "first_waves", "values"), out))


def test_fr_plan(n, n_vec=1, tile_log=9) -> dict:
    """The plan of a prefix-product scan (msm_amd_test_fr_plan): levels, launches, tiles of the first level over all
    vectors, records of ctx-owned device memory."""
    out = (c_uint64 * 4)()
    st = _lib().msm_amd_test_fr_plan(n, n_vec, tile_log, out)
    if st != OK:
        raise MsmError(st)
    return {"levels": out[0], "launches": out[1], "tiles": out[2], "records": out[3]}


def mul_plan(group=1) -> dict:
    """Constants of the scalar-multiplication paths (msm_amd_test_mul_plan): window c, windows W and entries of the
    fixed-base table, and K, the number of consecutive outputs that share one inversion."""
    out = (c_uint32 * 4)()
    st = _lib().msm_amd_test_mul_plan(group, out)
    if st != OK:
        raise MsmError(st)
    return {"c": out[0], "W": out[1], "entries": out[2], "K": out[3]}


MUL_STAGE_FIXED, MUL_STAGE_NORMALISE, MUL_STAGE_NORMALISE_RECORDS = 0, 1, 2       # MSM_AMD_MUL_STAGE_*
MUL_XYZZ_WORDS = {1: 36, 2: 72}                   # u32 per raw XYZZ record of the stage entries


def mul_stage_out_bytes(group, which, layout) -> int:
    """bytes per output record of a stage entry: a raw XYZZ record, or an affine record of the layout"""
    return decompressed_bytes(layout, group == 2) if which == MUL_STAGE_NORMALISE else 4 * MUL_XYZZ_WORDS.get(group, 0)


def test_mul_stage_host(group, which, layout, data: bytes, table, n: int) -> bytes:
    """MsmConfig.test_mul_stage on the host CPU (msm_amd_test_mul_stage_host: the same bodies, no GPU)."""
    size = mul_stage_out_bytes(group, which, layout)
    out = ctypes.create_string_buffer(max(1, n * size))
    st = _lib().msm_amd_test_mul_stage_host(group, which, layout, data, table, n, out)
    if st != OK:
        raise MsmError(st)
    return out.raw[:n * size]


def _g2_raw_in(seq, count):
    if len(seq) != count * G2_RAW_IN_WORDS:
        raise ValueError(f"a raw-limb G2 operand holds {G2_RAW_IN_WORDS} words per element")
    return _u32buf(seq)


def test_op_g2_host(op, a, b, count):
    """Same raw-limb G2 op bodies as MsmConfig.test_op_g2, executed on the host CPU by the library (no GPU)."""
    out = (c_uint32 * (count * G2_RAW_OUT_WORDS))()
    st = _lib().msm_amd_test_op_g2_host(op, _g2_raw_in(a, count), _g2_raw_in(b, count), out, count)
    if st != OK:
        raise MsmError(st)
    return list(out)


def sum_points(results) -> bytes:
    """Host sum of 96-byte results (the final addition of gpu_with_cpu, msm.rs:418-419)."""
    blob = b"".join(results)
    if len(blob) != 96 * len(results):
        raise ValueError("every result must be 96 bytes")
    out = ctypes.create_string_buffer(96)
    st = _lib().msm_amd_sum_points(blob, len(results), out)
    if st != OK:
        raise MsmError(st)
    return out.raw


def final_accumulation(res_be32, num_windows, window_size):
    """final_accumulation (final_accumulation.rs:5-40) -- host code in the library, no GPU needed."""
    out = (c_uint32 * 24)()
    st = _lib().msm_amd_final_accumulation(_u32buf(res_be32), num_windows, window_size, out)
    if st != OK:
        raise MsmError(st)
    return list(out)


# ---- names of the reference API (src/metal/msm.rs) ----------------------------------------------------
def setup_metal_state(device=-1) -> MsmConfig:
    """setup_metal_state (msm.rs:77-94)."""
    return MsmConfig(device)


def setup_metal_state_reusable() -> MsmConfig:
    """setup_metal_state_reusable (msm.rs:96-109): process-global cached config."""
    h = c_void_p()
    st = _lib().msm_amd_init_reusable(ctypes.byref(h))
    if st != OK:
        raise MsmError(st)
    return MsmConfig(_handle=h, _owned=False)


def get_global_metal_config() -> MsmConfig:
    """get_global_metal_config (msm.rs:114-119)."""
    h = c_void_p()
    st = _lib().msm_amd_get_global(ctypes.byref(h))
    if st != OK:
        raise MsmError(st, "MetalMsmConfig must be initialized before use.")
    return MsmConfig(_handle=h, _owned=False)


def gpu_msm_h2c(scalars: bytes, points: bytes, config: MsmConfig | None = None) -> bytes:
    """gpu_msm_h2c (msm.rs:352-364): bn256::Fr scalars (32 B each) x bn256::G1Affine points (64 B each)."""
    n = min(len(scalars) // 32, len(points) // 64)
    cfg = config or setup_metal_state_reusable()
    out = ctypes.create_string_buffer(96)
    cfg._check(_lib().msm_amd_gpu_msm_h2c(cfg.h, scalars, points, n, out))
    return out.raw


def gpu_msm_h2c_sync(scalars: bytes, points: bytes, after_sort, config: MsmConfig | None = None) -> bytes:
    """gpu_msm_h2c_sync (msm.rs:237-349): `after_sort()` is called once the GPU has finished sorting this MSM's
    bucket indices -- where the reference notifies its (Mutex<bool>, Condvar) pair (msm.rs:306-312)."""
    n = min(len(scalars) // 32, len(points) // 64)
    cfg = config or setup_metal_state_reusable()
    out = ctypes.create_string_buffer(96)
    cb = AFTER_SORT_FN((lambda _user: after_sort()) if after_sort is not None else 0)
    cfg._check(_lib().msm_amd_gpu_msm_h2c_sync(cfg.h, scalars, points, n, cb, None, out))
    return out.raw


def msm_best(scalars: bytes, points: bytes, config: MsmConfig | None = None) -> bytes:
    """msm_best (msm.rs:424-445): zero-scalar filtering + MSM."""
    n = min(len(scalars) // 32, len(points) // 64)
    cfg = config or setup_metal_state_reusable()
    out = ctypes.create_string_buffer(96)
    cfg._check(_lib().msm_amd_msm_best(cfg.h, scalars, points, n, out))
    return out.raw


def gpu_with_cpu(scalars: bytes, points: bytes, config: MsmConfig | None = None, split_at=None, cpu_threads=0) -> bytes:
    """gpu_with_cpu (msm.rs:366-421); split_at defaults to the reference's policy."""
    n = min(len(scalars) // 32, len(points) // 64)
    cfg = config or setup_metal_state_reusable()
    if split_at is None:
        split_at = _lib().msm_amd_reference_split(n)
    out = ctypes.create_string_buffer(96)
    cfg._check(_lib().msm_amd_gpu_with_cpu(cfg.h, scalars, points, n, split_at, cpu_threads, out))
    return out.raw


def metal_msm(points: bytes, scalars: bytes, config: MsmConfig) -> bytes:
    """metal_msm (msm.rs:220-234): ark G1Projective points (96 B each) x ark Fr scalars."""
    n = min(len(scalars) // 32, len(points) // 96)
    out = ctypes.create_string_buffer(96)
    config._check(_lib().msm_amd_metal_msm_ark(config.h, points, scalars, n, out))
    return out.raw
