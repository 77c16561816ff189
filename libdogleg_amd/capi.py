"""ctypes bindings to libdogleg_amd.so: the dogleg.h API (include/dogleg.h) and
the backend C-ABI (include/dlg_backend.h).  There is no CPU fallback: if the
HIP library is missing this module raises at load time, and every compute
entry point fails with DLG_ERR_NODEVICE when no GPU is present.
"""
import ctypes as C
import os
import numpy as np

from .ctypes_defs import (Parameters2, CholmodSparse, Trace, TraceBuffer, BatchResult, BatchLoss, BatchBounds, BatchFit, BatchModel, BatchCamera, MODEL_NSTATE, JacobianReport,
                          JacobianEntry,
                          NumericOptions, NUMERIC_FORWARD, NUMERIC_CENTRAL,
                          CB_SPARSE, CB_DENSE, CB_PRODUCTS, dptr, iptr)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DLG_TEST_LIB") or os.path.join(HERE, "libdogleg_amd.so")      # (DLG_TEST_LIB: tools only -- the test suite against a variant build, tools/variant_lib.sh)

DLG_OK = 0
DLG_DENSE, DLG_SPARSE, DLG_DENSE_PRODUCTS = 0, 1, 2
FLAG_PACKED, FLAG_UPPER = 1, 2
KIND_CAUCHY, KIND_GN, KIND_INTERP = 0, 1, 2
VEC_P, VEC_X, VEC_JTX, VEC_CAUCHY, VEC_GN, VEC_STEP, VEC_J, VEC_X_OWN, VEC_J_OWN = range(9)

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)

# every symbol include/dlg_backend.h and include/dogleg.h declare
BACKEND_SYMBOLS = [
    "dlg_last_error", "dlg_device_count", "dlg_backend_create", "dlg_backend_destroy",
    "dlg_backend_set_stream", "dlg_backend_get_stream", "dlg_backend_set_shard",
    "dlg_sparse_set_pattern", "dlg_sparse_stats", "dlg_sparse_schedule", "dlg_sparse_leaf_rows_stats", "dlg_point_set_p", "dlg_point_upload",
    "dlg_point_upload_products", "dlg_point_bind_device", "dlg_point_eval", "dlg_point_bind_held", "dlg_cauchy",
    "dlg_factorize", "dlg_solve_gn", "dlg_gauss_newton", "dlg_cauchy_gauss_newton", "dlg_make_step",
    "dlg_expected_improvement", "dlg_step", "dlg_take_step", "dlg_solve_with_factor",
    "dlg_point_download", "dlg_factor_download_dense", "dlg_point_device_ptr",
    "dlg_kernel_syrk_lower", "dlg_kernel_potrf_lower", "dlg_probe_mfma_f64", "dlg_probe_mfma_f64_clock", "dlg_probe_mfma_f64_waves",
    "dlg_probe_hbm_copy", "dlg_set_trace", "dlg_mem_alloc", "dlg_mem_free", "dlg_host_alloc",
    "dlg_host_free", "dlg_mem_upload",
    "dlg_mem_download", "dlg_mem_zero", "dlg_device_sync", "dlg_sparse_symbolic_probe",
    "dlg_backend_set_profiling", "dlg_backend_get_profile", "dlg_backend_get_profile_early",
    "dlg_backend_set_allreduce", "dlg_backend_set_partition", "dlg_partition_rows", "dlg_partition_stats",
    "dlg_sparse_partition_probe", "dlg_rccl_unique_id", "dlg_backend_init_rccl", "dlg_backend_set_rccl",
    "dlg_backend_comm_size", "dlg_backend_has_rccl", "dlg_backend_set_noop_comm", "dlg_solve_multi", "dlg_pseudoinverse_chunk", "dlg_backend_set_speculation", "dlg_backend_set_defer_tail", "dlg_step_tail",
    "dlg_step_tail_pending", "dlg_backend_ei_source", "dlg_backend_set_between", "dlg_backend_between_redone", "dlg_point_eval_early",
    "dlg_backend_share_rccl", "dlg_point_gather_device", "dlg_backend_reset", "dlg_backend_device",
    "dlg_sparse_pattern_matches", "dlg_sparse_drop_pattern", "dlg_sparse_region_probe", "dlg_run_steps", "dlg_backend_time_allreduce",
    "dlg_feature_leverage", "dlg_outlierness_factors", "dlg_leverage_query", "dlg_leverage_stats",
    "dlg_covariance_blocks", "dlg_marginal_variances", "dlg_covariance_stats", "dlg_covariance_plan_seconds",
    "dlg_covariance_plan_probe", "dlg_covariance_entries", "dlg_covariance_entries_stats", "dlg_covariance_entries_probe",
    "dlg_query_covariance", "dlg_query_covariance_stats", "dlg_query_covariance_plan_seconds", "dlg_query_covariance_plan_probe",
]
PROF_NAMES = ["K1_jtx", "K3K8_norm2Jv", "K4_kernel", "K4_total", "K5_factor", "K6_solve", "K7_step", "vec"]
DOGLEG_SYMBOLS = [
    "dogleg_getDefaultParameters", "dogleg_setMaxIterations",
    "dogleg_setTrustregionUpdateParameters", "dogleg_setDebug", "dogleg_setInitialTrustregion",
    "dogleg_setThresholds", "dogleg_optimize", "dogleg_optimize2", "dogleg_optimize_dense",
    "dogleg_optimize_dense2", "dogleg_optimize_dense_products", "dogleg_computeJtJfactorization",
    "dogleg_freeContext", "dogleg_testGradient", "dogleg_testGradient_dense",
    "dogleg_testGradient_dense_products",
    "dogleg_optimize_device2", "dogleg_amd_backend", "dogleg_amd_point_slot",
    "dogleg_amd_set_communicator", "dogleg_amd_set_allreduce", "dogleg_amd_clear_communicator",
    "dogleg_amd_rccl_unique_id", "dogleg_amd_rank", "dogleg_amd_release_cache",
    "dogleg_amd_id_file_publish", "dogleg_amd_id_file_wait", "dogleg_amd_last_solve_timing",
    "dogleg_getOutliernessFactors", "dogleg_markOutliers", "dogleg_reportOutliers",
    "dogleg_getOutliernessTrace_newFeature_sparse",
    "dogleg_amd_covariance_blocks", "dogleg_amd_marginal_variances", "dogleg_amd_covariance_entries",
    "dogleg_amd_query_covariance",
    "dogleg_amd_optimize_dense_batch", "dogleg_amd_batch_last_stats",
    "dogleg_amd_dense_batch_uncertainty", "dogleg_amd_batch_uncertainty_last_stats",
    "dogleg_amd_optimize_dense_products_batch", "dogleg_amd_dense_products_batch_uncertainty",
    "dogleg_amd_optimize_dense_batch_device", "dogleg_amd_optimize_dense_products_batch_device",
    "dogleg_amd_dense_batch_uncertainty_device", "dogleg_amd_dense_products_batch_uncertainty_device",
    "dlg_batch_device_span_ok",          # (csrc/dense_batch.h: the pointer check of the four above, exported for the tests)
    "dogleg_amd_optimize_dense_batch_robust", "dogleg_amd_optimize_dense_batch_robust_device",
    "dogleg_amd_optimize_dense_batch_bounded", "dogleg_amd_optimize_dense_batch_bounded_device",
    "dogleg_amd_optimize_dense_products_batch_bounded", "dogleg_amd_optimize_dense_products_batch_bounded_device",
    "dogleg_amd_dense_batch_query_covariance", "dogleg_amd_dense_products_batch_query_covariance",
    "dogleg_amd_dense_batch_query_covariance_device", "dogleg_amd_dense_products_batch_query_covariance_device",
    "dogleg_amd_dense_batch_uncertainty_fit", "dogleg_amd_dense_products_batch_uncertainty_fit",
    "dogleg_amd_dense_batch_uncertainty_fit_device", "dogleg_amd_dense_products_batch_uncertainty_fit_device",
    "dogleg_amd_dense_batch_query_covariance_fit", "dogleg_amd_dense_products_batch_query_covariance_fit",
    "dogleg_amd_dense_batch_query_covariance_fit_device", "dogleg_amd_dense_products_batch_query_covariance_fit_device",
    "dogleg_amd_jacobian_colouring", "dogleg_amd_check_jacobian_device", "dogleg_amd_check_jacobian_device_batch",
    "dogleg_amd_testGradient_device", "dogleg_amd_check_jacobian_last_stats",
    "dogleg_amd_optimize_device2_robust", "dogleg_amd_robust_last_stats",
    "dogleg_amd_optimize_device2_bounded", "dogleg_amd_bounded_last_stats",
    "dogleg_amd_batch_numeric_create", "dogleg_amd_batch_numeric_destroy", "dogleg_amd_batch_numeric_callback",
    "dogleg_amd_batch_numeric_stats", "dogleg_amd_batch_numeric_buffers", "dogleg_amd_numeric_step",
    "dogleg_amd_numeric_plan", "dogleg_amd_numeric_create", "dogleg_amd_numeric_destroy", "dogleg_amd_numeric_callback",
    "dogleg_amd_numeric_stats", "dogleg_amd_numeric_buffers",
    "dogleg_amd_batch_model_nstate", "dogleg_amd_batch_model_callback", "dogleg_amd_batch_model_callback_invocations",
    "dogleg_amd_optimize_dense_batch_model", "dogleg_amd_optimize_dense_batch_model_device",
    "dogleg_amd_optimize_dense_batch_model_mle", "dogleg_amd_optimize_dense_batch_model_mle_device",
    "dogleg_amd_batch_model_fisher_callback",
    "dogleg_amd_dense_batch_model_uncertainty", "dogleg_amd_dense_batch_model_uncertainty_device",
    "dogleg_amd_dense_batch_model_query_covariance", "dogleg_amd_dense_batch_model_query_covariance_device",
    "dogleg_amd_batch_camera_callback", "dogleg_amd_batch_camera_fisher_callback",
    "dogleg_amd_optimize_dense_batch_camera", "dogleg_amd_optimize_dense_batch_camera_device",
    "dogleg_amd_dense_batch_camera_uncertainty", "dogleg_amd_dense_batch_camera_uncertainty_device",
    "dogleg_amd_dense_batch_camera_query_covariance", "dogleg_amd_dense_batch_camera_query_covariance_device",
]

_lib = None


class DlgError(RuntimeError):
    pass


def lib():
    """Load libdogleg_amd.so (building it is __graft_entry__.build()'s job)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DlgError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; "
                       "g.build()'` (there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    D, I, V = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    L.dlg_last_error.restype = C.c_char_p
    L.dlg_device_count.restype = C.c_int
    L.dlg_backend_create.argtypes = [C.POINTER(V), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.dlg_backend_destroy.argtypes = [V]
    L.dlg_backend_destroy.restype = None
    L.dlg_backend_set_stream.argtypes = [V, V]
    L.dlg_backend_get_stream.argtypes = [V]
    L.dlg_backend_get_stream.restype = V
    L.dlg_backend_set_shard.argtypes = [V, C.c_int, C.c_int, V, V]
    L.dlg_backend_set_allreduce.argtypes = [V, V, V]
    L.dlg_backend_set_speculation.argtypes = [V, C.c_int]
    L.dlg_backend_set_defer_tail.argtypes = [V, C.c_int]
    L.dlg_step_tail.argtypes = [V, C.POINTER(C.c_double)]
    L.dlg_step_tail_pending.argtypes = [V]
    L.dlg_backend_ei_source.argtypes = [V, I, D]
    L.dlg_backend_set_partition.argtypes = [V, C.c_int, C.c_int]
    L.dlg_partition_rows.argtypes = [V, I, C.POINTER(I)]
    L.dlg_partition_stats.argtypes = [V, C.POINTER(C.c_long), C.c_int]
    L.dlg_sparse_partition_probe.argtypes = [C.c_int, C.c_int, I, I, C.c_int, C.c_int, C.POINTER(C.c_long), C.c_int, C.c_char_p]
    L.dlg_rccl_unique_id.argtypes = [V]
    L.dlg_backend_init_rccl.argtypes = [V, C.c_int, C.c_int, V]
    L.dlg_backend_set_rccl.argtypes = [V, V]
    L.dlg_backend_comm_size.argtypes = [V, I]
    L.dlg_backend_has_rccl.argtypes = [V]
    L.dlg_backend_set_noop_comm.argtypes = [V, C.c_int]
    L.dlg_backend_get_profile_early.argtypes = [V, D, C.POINTER(C.c_long), C.c_int]
    L.dlg_sparse_set_pattern.argtypes = [V, I, I]
    L.dlg_sparse_stats.argtypes = [V, C.POINTER(C.c_long), C.POINTER(C.c_long), I, I, D]
    L.dlg_sparse_schedule.argtypes = [V, I, I, I]
    L.dlg_sparse_leaf_rows_stats.argtypes = [V, C.POINTER(C.c_long), C.c_int]
    L.dlg_point_set_p.argtypes = [V, C.c_int, D]
    L.dlg_point_upload.argtypes = [V, C.c_int, D, D]
    L.dlg_point_upload_products.argtypes = [V, C.c_int, C.c_double, D, D]
    L.dlg_point_bind_device.argtypes = [V, C.c_int, V, V]
    L.dlg_point_eval.argtypes = [V, C.c_int, D, D]
    L.dlg_cauchy.argtypes = [V, C.c_int, D]
    L.dlg_factorize.argtypes = [V, C.c_int, C.c_double, I]
    L.dlg_solve_gn.argtypes = [V, C.c_int, D]
    L.dlg_gauss_newton.argtypes = [V, C.c_int, D, D]
    L.dlg_cauchy_gauss_newton.argtypes = [V, C.c_int, D, D, D]
    L.dlg_make_step.argtypes = [V, C.c_int, C.c_int, C.c_int, C.c_double, D, D, D, D]
    L.dlg_step.argtypes = [V, C.c_int, C.c_int, C.c_int, C.c_double, D, D, D, D, D]
    L.dlg_take_step.argtypes = [V, C.c_int, C.c_int, C.c_double, D, D, D]
    L.dlg_solve_with_factor.argtypes = [V, C.c_int, D, D, C.c_int]
    L.dlg_solve_multi.argtypes = [V, C.c_int, D, D, C.c_int]
    L.dlg_pseudoinverse_chunk.argtypes = [V, C.c_int, C.c_int, C.c_int, D]
    L.dlg_feature_leverage.argtypes = [V, C.c_int, C.c_int, C.c_int, C.c_int, D]
    L.dlg_outlierness_factors.argtypes = [V, C.c_int, C.c_int, C.c_int, C.c_double, D]
    L.dlg_leverage_query.argtypes = [V, C.c_int, D, C.c_int, C.c_int, C.c_int, D]
    L.dlg_leverage_stats.argtypes = [V, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long), I]
    L.dlg_covariance_blocks.argtypes = [V, C.c_int, C.c_int, I, I, I, I, D]
    L.dlg_marginal_variances.argtypes = [V, C.c_int, D]
    L.dlg_covariance_stats.argtypes = [V, C.POINTER(C.c_long), C.POINTER(C.c_long), I]
    L.dlg_covariance_plan_seconds.argtypes = [V]
    L.dlg_covariance_plan_seconds.restype = C.c_double
    L.dlg_covariance_plan_probe.argtypes = [C.c_int, C.c_int, I, I, C.c_int, I, I, I, I, I, C.POINTER(C.c_long), C.c_int]
    L.dlg_covariance_entries.argtypes = [V, C.c_int, C.c_long, I, I, D]
    L.dlg_covariance_entries_stats.argtypes = [V, D, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.dlg_covariance_entries_probe.argtypes = [C.c_int, C.c_int, I, I, C.c_long, I, I, I, C.POINTER(C.c_long), C.c_int]
    if hasattr(L, "dlg_query_covariance"):          # (a DLG_TEST_LIB built before query covariance has none of these)
        L.dlg_query_covariance.argtypes = [V, C.c_int, C.c_int, I, I, I, D, C.c_int, D]
        L.dlg_query_covariance_stats.argtypes = [V, C.POINTER(C.c_long), C.POINTER(C.c_long), I]
        L.dlg_query_covariance_plan_seconds.argtypes = [V]
        L.dlg_query_covariance_plan_seconds.restype = C.c_double
        L.dlg_query_covariance_plan_probe.argtypes = [C.c_int, C.c_int, I, I, C.c_int, I, I, I, I, C.POINTER(C.c_long),
                                                      C.c_int]
    L.dlg_expected_improvement.argtypes = [V, C.c_int, C.c_int, D]
    L.dlg_point_download.argtypes = [V, C.c_int, C.c_int, D, C.c_size_t]
    L.dlg_factor_download_dense.argtypes = [V, D, C.c_size_t]
    L.dlg_point_device_ptr.argtypes = [V, C.c_int, C.c_int]
    L.dlg_point_device_ptr.restype = V
    L.dlg_kernel_syrk_lower.argtypes = [V, V, C.c_int, V, C.c_int, C.c_int, C.c_int, C.c_double, V, C.c_size_t]
    L.dlg_kernel_potrf_lower.argtypes = [V, V, C.c_int, C.c_int, V]
    L.dlg_probe_mfma_f64.argtypes = [D]
    L.dlg_probe_hbm_copy.argtypes = [D]
    L.dlg_set_trace.argtypes = [V]
    L.dlg_set_trace.restype = None
    L.dlg_mem_alloc.argtypes = [C.c_size_t]
    L.dlg_mem_alloc.restype = V
    L.dlg_mem_free.argtypes = [V]
    L.dlg_mem_free.restype = None
    L.dlg_host_alloc.argtypes = [C.c_size_t]
    L.dlg_host_alloc.restype = V
    L.dlg_host_free.argtypes = [V]
    L.dlg_host_free.restype = None
    L.dlg_mem_upload.argtypes = [V, V, C.c_size_t]
    L.dlg_mem_download.argtypes = [V, V, C.c_size_t]
    L.dlg_mem_zero.argtypes = [V, C.c_size_t]
    L.dlg_backend_set_profiling.argtypes = [V, C.c_int]
    L.dlg_backend_get_profile.argtypes = [V, D, C.POINTER(C.c_long), C.c_int]
    L.dlg_sparse_symbolic_probe.argtypes = [C.c_int, C.c_int, I, I, C.c_int, C.c_int,
                                            C.POINTER(C.c_long), C.c_int, I]
    # dogleg.h
    PP = C.POINTER(Parameters2)
    L.dogleg_getDefaultParameters.argtypes = [PP]
    L.dogleg_getDefaultParameters.restype = None
    L.dogleg_optimize2.restype = C.c_double
    L.dogleg_optimize2.argtypes = [D, C.c_uint, C.c_uint, C.c_uint, V, V, PP, V]
    L.dogleg_optimize.restype = C.c_double
    L.dogleg_optimize.argtypes = [D, C.c_uint, C.c_uint, C.c_uint, V, V, V]
    L.dogleg_optimize_dense2.restype = C.c_double
    L.dogleg_optimize_dense2.argtypes = [D, C.c_uint, C.c_uint, V, V, PP, V]
    L.dogleg_optimize_dense.restype = C.c_double
    L.dogleg_optimize_dense.argtypes = [D, C.c_uint, C.c_uint, V, V, V]
    L.dogleg_optimize_dense_products.restype = C.c_double
    L.dogleg_optimize_dense_products.argtypes = [D, C.c_uint, V, V, PP, V]
    L.dogleg_freeContext.argtypes = [V]
    L.dogleg_freeContext.restype = None
    L.dogleg_optimize_device2.restype = C.c_double
    L.dogleg_optimize_device2.argtypes = [D, C.c_uint, C.c_uint, C.c_uint, I, I, V, V, PP, V]
    L.dogleg_amd_backend.restype = V
    L.dogleg_amd_backend.argtypes = [V]
    L.dogleg_amd_point_slot.restype = C.c_int
    L.dogleg_amd_point_slot.argtypes = [V, V]
    L.dogleg_amd_set_communicator.argtypes = [C.c_int, C.c_int, C.c_int, V]
    L.dogleg_amd_set_allreduce.argtypes = [C.c_int, C.c_int, C.c_int, V, V]
    L.dogleg_amd_clear_communicator.restype = None
    L.dogleg_amd_rccl_unique_id.argtypes = [V]
    L.dogleg_amd_rank.argtypes = [V, I]
    L.dogleg_amd_id_file_publish.argtypes = [C.c_char_p, V, C.c_char_p]
    L.dogleg_amd_id_file_wait.argtypes = [C.c_char_p, V, C.c_char_p, C.c_int]
    L.dlg_backend_share_rccl.argtypes = [V, V]
    L.dlg_sparse_region_probe.argtypes = [C.c_int, C.c_int, I, I, C.c_int, C.POINTER(C.c_long), C.c_int]
    L.dlg_run_steps.argtypes = [V, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(V), C.POINTER(V), C.c_int, C.c_double, C.c_double, D, I]
    L.dlg_backend_reset.argtypes = [V]
    L.dlg_backend_device.argtypes = [V]
    L.dlg_sparse_pattern_matches.argtypes = [V, I, I]
    L.dlg_sparse_drop_pattern.argtypes = [V]
    L.dogleg_amd_release_cache.restype = None
    if hasattr(L, "dogleg_amd_optimize_dense_batch"):          # (a DLG_TEST_LIB built before the batch solver has neither)
        L.dogleg_amd_optimize_dense_batch.argtypes = [D, C.c_uint, C.c_uint, C.c_uint, V, V, PP, C.POINTER(BatchResult)]
        L.dogleg_amd_batch_last_stats.argtypes = [D, C.c_int]
    if hasattr(L, "dogleg_amd_dense_batch_uncertainty"):
        L.dogleg_amd_dense_batch_uncertainty.argtypes = [D, C.c_uint, C.c_uint, C.c_uint, V, V, D, D, D, D, D, C.c_int, I]
        L.dogleg_amd_batch_uncertainty_last_stats.argtypes = [D, C.c_int]
    if hasattr(L, "dogleg_amd_optimize_dense_products_batch"):
        L.dogleg_amd_optimize_dense_products_batch.argtypes = [D, C.c_uint, C.c_uint, V, V, PP, C.POINTER(BatchResult)]
        L.dogleg_amd_dense_products_batch_uncertainty.argtypes = [D, C.c_uint, C.c_uint, V, V, PP, D, D, D, I]
    if hasattr(L, "dogleg_amd_optimize_dense_batch_device"):
        L.dogleg_amd_optimize_dense_batch_device.argtypes = [V, C.c_uint, C.c_uint, C.c_uint, V, V, PP, V, V, V, V]
        L.dogleg_amd_optimize_dense_products_batch_device.argtypes = [V, C.c_uint, C.c_uint, V, V, PP, V, V, V, V]
        L.dogleg_amd_dense_batch_uncertainty_device.argtypes = [V, C.c_uint, C.c_uint, C.c_uint, V, V, V, V, V, V, V, C.c_int,
                                                                V, V, V]
        L.dogleg_amd_dense_products_batch_uncertainty_device.argtypes = [V, C.c_uint, C.c_uint, V, V, PP, V, V, V, V, V, V]
        L.dlg_batch_device_span_ok.argtypes = [V, C.c_size_t]
    if hasattr(L, "dogleg_amd_optimize_dense_batch_robust"):
        LP = C.POINTER(BatchLoss)
        L.dogleg_amd_optimize_dense_batch_robust.argtypes = [D, C.c_uint, C.c_uint, C.c_uint, V, V, PP, LP,
                                                             C.POINTER(BatchResult), D]
        L.dogleg_amd_optimize_dense_batch_robust_device.argtypes = [V, C.c_uint, C.c_uint, C.c_uint, V, V, PP, LP, V, V, V, V, V]
    if hasattr(L, "dogleg_amd_optimize_dense_batch_bounded"):
        LP, BP = C.POINTER(BatchLoss), C.POINTER(BatchBounds)
        L.dogleg_amd_optimize_dense_batch_bounded.argtypes = [D, C.c_uint, C.c_uint, C.c_uint, V, V, PP, LP, BP,
                                                              C.POINTER(BatchResult), D]
        L.dogleg_amd_optimize_dense_batch_bounded_device.argtypes = [V, C.c_uint, C.c_uint, C.c_uint, V, V, PP, LP, BP, V, V, V,
                                                                     V, V]
    if hasattr(L, "dogleg_amd_optimize_dense_products_batch_bounded"):
        BP = C.POINTER(BatchBounds)
        L.dogleg_amd_optimize_dense_products_batch_bounded.argtypes = [D, C.c_uint, C.c_uint, V, V, PP, BP, C.POINTER(BatchResult)]
        L.dogleg_amd_optimize_dense_products_batch_bounded_device.argtypes = [V, C.c_uint, C.c_uint, V, V, PP, BP, V, V, V, V]
    if hasattr(L, "dogleg_amd_optimize_dense_batch_model"):
        MP, BP = C.POINTER(BatchModel), C.POINTER(BatchBounds)
        L.dogleg_amd_batch_model_nstate.argtypes = [C.c_int]
        L.dogleg_amd_batch_model_callback.argtypes = [V, V, V, V, C.c_uint, V, V]
        L.dogleg_amd_batch_model_callback.restype = None
        L.dogleg_amd_batch_model_callback_invocations.restype = C.c_ulonglong
        L.dogleg_amd_optimize_dense_batch_model.argtypes = [D, C.c_uint, MP, PP, BP, C.POINTER(BatchResult)]
        L.dogleg_amd_optimize_dense_batch_model_device.argtypes = [V, C.c_uint, MP, PP, BP, V, V, V, V]
    if hasattr(L, "dogleg_amd_optimize_dense_batch_model_mle"):
        MP, BP = C.POINTER(BatchModel), C.POINTER(BatchBounds)
        L.dogleg_amd_optimize_dense_batch_model_mle.argtypes = [D, C.c_uint, MP, C.c_int, PP, BP, C.POINTER(BatchResult)]
        L.dogleg_amd_optimize_dense_batch_model_mle_device.argtypes = [V, C.c_uint, MP, C.c_int, PP, BP, V, V, V, V]
        L.dogleg_amd_batch_model_fisher_callback.argtypes = [V, V, V, V, C.c_uint, V, V]
        L.dogleg_amd_batch_model_fisher_callback.restype = None
    if hasattr(L, "dogleg_amd_dense_batch_model_uncertainty"):
        MP, U = C.POINTER(BatchModel), C.c_uint
        L.dogleg_amd_dense_batch_model_uncertainty.argtypes = [D, U, MP, C.c_int, D, D, D, D, D, C.c_int, I, V]
        L.dogleg_amd_dense_batch_model_uncertainty_device.argtypes = [V, U, MP, C.c_int, V, V, V, V, V, C.c_int, V, V, V, V]
        L.dogleg_amd_dense_batch_model_query_covariance.argtypes = [D, U, MP, C.c_int, D, D, U, U, C.c_int, D, I, V]
        L.dogleg_amd_dense_batch_model_query_covariance_device.argtypes = [V, U, MP, C.c_int, V, V, U, U, C.c_int, V, V, V, V, V]
    if hasattr(L, "dogleg_amd_optimize_dense_batch_camera"):
        CP, PP, BP, U = C.POINTER(BatchCamera), C.POINTER(Parameters2), C.POINTER(BatchBounds), C.c_uint
        L.dogleg_amd_optimize_dense_batch_camera.argtypes = [D, U, CP, C.c_int, PP, BP, C.POINTER(BatchResult)]
        L.dogleg_amd_optimize_dense_batch_camera_device.argtypes = [V, U, CP, C.c_int, PP, BP, V, V, V, V]
        L.dogleg_amd_dense_batch_camera_uncertainty.argtypes = [D, U, CP, C.c_int, D, D, D, D, D, C.c_int, I, V]
        L.dogleg_amd_dense_batch_camera_uncertainty_device.argtypes = [V, U, CP, C.c_int, V, V, V, V, V, C.c_int, V, V, V, V]
        L.dogleg_amd_dense_batch_camera_query_covariance.argtypes = [D, U, CP, C.c_int, D, D, U, U, C.c_int, D, I, V]
        L.dogleg_amd_dense_batch_camera_query_covariance_device.argtypes = [V, U, CP, C.c_int, V, V, U, U, C.c_int, V, V, V, V, V]
        for n in ("dogleg_amd_batch_camera_callback", "dogleg_amd_batch_camera_fisher_callback"):
            getattr(L, n).argtypes = [V, V, V, V, C.c_uint, V, V]
            getattr(L, n).restype = None
    if hasattr(L, "dogleg_amd_dense_batch_query_covariance"):
        U = C.c_uint
        L.dogleg_amd_dense_batch_query_covariance.argtypes = [D, U, U, U, V, V, D, D, U, U, C.c_int, D, I]
        L.dogleg_amd_dense_products_batch_query_covariance.argtypes = [D, U, U, V, V, PP, D, D, U, U, D, I]
        L.dogleg_amd_dense_batch_query_covariance_device.argtypes = [V, U, U, U, V, V, V, V, U, U, C.c_int, V, V, V, V]
        L.dogleg_amd_dense_products_batch_query_covariance_device.argtypes = [V, U, U, V, V, PP, V, V, U, U, V, V, V, V]
    if hasattr(L, "dogleg_amd_dense_batch_uncertainty_fit"):
        # the argument lists of the eight calls without _fit, then the fit record
        FP = C.POINTER(BatchFit)
        for name in DOGLEG_SYMBOLS:
            if "_fit" in name:
                twin = name.replace("_fit", "")
                getattr(L, name).argtypes = list(getattr(L, twin).argtypes) + [FP]
    if hasattr(L, "dogleg_amd_check_jacobian_device"):
        JR, JE = C.POINTER(JacobianReport), C.POINTER(JacobianEntry)
        L.dogleg_amd_jacobian_colouring.argtypes = [C.c_uint, C.c_uint, I, I, I]
        L.dogleg_amd_check_jacobian_device.argtypes = [D, C.c_uint, C.c_uint, C.c_uint, I, I, V, V, C.c_double, C.c_double,
                                                       C.c_double, C.c_int, JR, D, JE, C.c_int]
        L.dogleg_amd_check_jacobian_device_batch.argtypes = [D, C.c_uint, C.c_uint, C.c_uint, V, V, C.c_double, C.c_double,
                                                             C.c_double, JR, JE, C.c_int, C.POINTER(C.c_longlong)]
        L.dogleg_amd_testGradient_device.argtypes = [C.c_uint, D, C.c_uint, C.c_uint, C.c_uint, I, I, V, V]
        L.dogleg_amd_testGradient_device.restype = None
        L.dogleg_amd_check_jacobian_last_stats.argtypes = [D, C.c_int]
    if hasattr(L, "dogleg_amd_optimize_device2_robust"):
        L.dogleg_amd_optimize_device2_robust.restype = C.c_double
        L.dogleg_amd_optimize_device2_robust.argtypes = [D, C.c_uint, C.c_uint, C.c_uint, I, I, V, V, C.POINTER(BatchLoss), D, PP, V]
        L.dogleg_amd_robust_last_stats.argtypes = [D, C.c_int]
    if hasattr(L, "dogleg_amd_optimize_device2_bounded"):
        L.dogleg_amd_optimize_device2_bounded.restype = C.c_double
        L.dogleg_amd_optimize_device2_bounded.argtypes = [D, C.c_uint, C.c_uint, C.c_uint, I, I, V, V, C.POINTER(BatchLoss), D,
                                                          C.POINTER(BatchBounds), PP, V]
        L.dogleg_amd_bounded_last_stats.argtypes = [D, C.c_int]
        L.dlg_point_bind_held.argtypes = [V, C.c_int, V, C.c_double]
    if hasattr(L, "dogleg_amd_batch_numeric_create"):
        L.dogleg_amd_batch_numeric_create.restype = V
        L.dogleg_amd_batch_numeric_create.argtypes = [C.c_uint, C.c_uint, C.c_uint, V, V, C.POINTER(NumericOptions)]
        L.dogleg_amd_batch_numeric_destroy.argtypes = [V]
        L.dogleg_amd_batch_numeric_destroy.restype = None
        L.dogleg_amd_batch_numeric_callback.argtypes = [V, V, V, V, C.c_uint, V, V]
        L.dogleg_amd_batch_numeric_callback.restype = None
        L.dogleg_amd_batch_numeric_stats.argtypes = [V, D, C.c_int]
        L.dogleg_amd_batch_numeric_buffers.argtypes = [V, C.POINTER(V), C.POINTER(V), C.POINTER(V)]
        L.dogleg_amd_numeric_step.argtypes = [C.c_int] + [C.c_double] * 5 + [D, D, D]
        L.dogleg_amd_numeric_step.restype = None
    if hasattr(L, "dogleg_amd_numeric_create"):
        L.dogleg_amd_numeric_plan.argtypes = [C.c_uint, C.c_uint, C.c_uint, I, I, C.c_int, I, I, D]
        L.dogleg_amd_numeric_create.restype = V
        L.dogleg_amd_numeric_create.argtypes = [C.c_uint, C.c_uint, C.c_uint, I, I, V, V, C.POINTER(NumericOptions)]
        L.dogleg_amd_numeric_destroy.argtypes = [V]
        L.dogleg_amd_numeric_destroy.restype = None
        L.dogleg_amd_numeric_callback.argtypes = [V, V, V, V, V]
        L.dogleg_amd_numeric_callback.restype = None
        L.dogleg_amd_numeric_stats.argtypes = [V, D, C.c_int]
        L.dogleg_amd_numeric_buffers.argtypes = [V, C.POINTER(V), C.POINTER(V), C.POINTER(V)]
    L.dogleg_amd_last_solve_timing.argtypes = [D, I]
    L.dlg_point_gather_device.argtypes = [V, C.c_int, V, V, I]
    L.dogleg_setMaxIterations.argtypes = [C.c_int]
    L.dogleg_setDebug.argtypes = [C.c_int]
    L.dogleg_setInitialTrustregion.argtypes = [C.c_double]
    L.dogleg_setThresholds.argtypes = [C.c_double, C.c_double, C.c_double]
    L.dogleg_setTrustregionUpdateParameters.argtypes = [C.c_double] * 4
    _lib = L
    return L


def _ck(rc, what=""):
    if rc != DLG_OK:
        raise DlgError(f"{what} failed (code {rc}): {lib().dlg_last_error().decode()}")


def default_parameters():
    p = Parameters2()
    lib().dogleg_getDefaultParameters(C.byref(p))
    return p


def optimize(kind, p0, N, M, nnz, cb, cookie, params=None, capacity=256, trace=True):
    """dogleg_optimize2 / _dense2 / _dense_products with a per-trial trace (trace=False: without, as a user calls it).
    kind in {'sparse','dense','products'}; cb is a function address (c_void_p).
    Returns (norm2x, p_final, TraceBuffer)."""
    L = lib()
    p = np.array(p0, dtype=np.float64, copy=True)
    tr = TraceBuffer(N, capacity) if trace else None
    prm = C.byref(params) if params is not None else None
    L.dlg_set_trace(C.cast(tr.byref(), C.c_void_p) if trace else None)
    try:
        if kind == "sparse":
            r = L.dogleg_optimize2(dptr(p), N, M, nnz, cb, cookie, prm, None)
        elif kind == "dense":
            r = L.dogleg_optimize_dense2(dptr(p), N, M, cb, cookie, prm, None)
        else:
            r = L.dogleg_optimize_dense_products(dptr(p), N, cb, cookie, prm, None)
    finally:
        L.dlg_set_trace(None)
    return r, p, tr


def optimize_device(p0, N, M, nnz, Jp, Ji, cb, cookie, params=None, capacity=256, trace=True):
    """dogleg_optimize_device2 (device-side evaluation) with a per-trial trace.  nnz == 0: dense
    (Jp, Ji ignored).  cb: address of a dogleg_callback_device_t.  Returns (norm2x, p_final, TraceBuffer).
    trace=False: no per-trial record (every record downloads the step vector: a test feature that costs a
    synchronisation a trial) -- what a user's call does; the third value is None then."""
    L = lib()
    p = np.array(p0, dtype=np.float64, copy=True)
    tr = TraceBuffer(N, capacity) if trace else None
    prm = C.byref(params) if params is not None else None
    if nnz > 0:
        Jp = np.ascontiguousarray(Jp, dtype=np.int32)
        Ji = np.ascontiguousarray(Ji, dtype=np.int32)
    L.dlg_set_trace(C.cast(tr.byref(), C.c_void_p) if trace else None)
    try:
        r = L.dogleg_optimize_device2(dptr(p), N, M, nnz, iptr(Jp) if nnz > 0 else None,
                                      iptr(Ji) if nnz > 0 else None, cb, cookie, prm, None)
    finally:
        L.dlg_set_trace(None)
    return r, p, tr


def optimize_device_robust(p0, N, M, nnz, Jp, Ji, cb, cookie, loss, params=None, capacity=256, trace=True, want_weights=True,
                           ctx=None):
    """dogleg_amd_optimize_device2_robust: the arguments of optimize_device with loss a BatchLoss (None: NULL).  Returns what
    optimize_device returns and the weights: (F, p_final, TraceBuffer, weights (M // max(featureSize, 1),) prefilled with -1, or
    None if not asked for).  ctx: a ctypes.c_void_p that receives the returnContext (release it with dogleg_freeContext)."""
    L = lib()
    p = np.array(p0, dtype=np.float64, copy=True)
    tr = TraceBuffer(N, capacity) if trace else None
    fs = max(loss.featureSize, 1) if loss is not None else 1
    w = np.full(M // fs, -1.0) if want_weights else None
    if nnz > 0:
        Jp = np.ascontiguousarray(Jp, dtype=np.int32)
        Ji = np.ascontiguousarray(Ji, dtype=np.int32)
    L.dlg_set_trace(C.cast(tr.byref(), C.c_void_p) if trace else None)
    try:
        r = L.dogleg_amd_optimize_device2_robust(dptr(p), N, M, nnz, iptr(Jp) if nnz > 0 else None, iptr(Ji) if nnz > 0 else None,
                                                 cb, cookie, C.byref(loss) if loss is not None else None,
                                                 dptr(w) if w is not None else None,
                                                 C.byref(params) if params is not None else None,
                                                 C.byref(ctx) if ctx is not None else None)
    finally:
        L.dlg_set_trace(None)
    return r, p, tr, w


def optimize_device_bounded(p0, N, M, nnz, Jp, Ji, cb, cookie, lower=None, upper=None, loss=None, params=None, capacity=256,
                            trace=True, want_weights=None, want_held=True, ctx=None, null_bounds=False):
    """dogleg_amd_optimize_device2_bounded: the arguments of optimize_device_robust with lower / upper (N,) arrays or None
    (NULL: no bounds on that side); loss None: least squares.  Returns (norm2x or F, p_final, TraceBuffer, weights or None,
    held (N,) uint8 prefilled with 255 or None).  weights are asked for by default iff a loss is given (want_weights=True
    without one passes an array all the same: the call is refused).  null_bounds: pass NULL for the struct itself."""
    L = lib()
    p = np.array(p0, dtype=np.float64, copy=True)
    tr = TraceBuffer(N, capacity) if trace else None
    fs = max(loss.featureSize, 1) if loss is not None else 1
    if want_weights is None:
        want_weights = loss is not None
    w = np.full(M // fs, -1.0) if want_weights else None
    held = np.full(N, 255, dtype=np.uint8) if want_held else None
    lo = None if lower is None else np.ascontiguousarray(lower, dtype=np.float64)
    hi = None if upper is None else np.ascontiguousarray(upper, dtype=np.float64)
    assert all(a is None or a.shape == (N,) for a in (lo, hi))
    addr = lambda a: a.ctypes.data if a is not None else None
    bounds = BatchBounds(addr(lo), addr(hi), addr(held))
    if nnz > 0:
        Jp = np.ascontiguousarray(Jp, dtype=np.int32)
        Ji = np.ascontiguousarray(Ji, dtype=np.int32)
    L.dlg_set_trace(C.cast(tr.byref(), C.c_void_p) if trace else None)
    try:
        r = L.dogleg_amd_optimize_device2_bounded(dptr(p), N, M, nnz, iptr(Jp) if nnz > 0 else None, iptr(Ji) if nnz > 0 else None,
                                                  cb, cookie, C.byref(loss) if loss is not None else None,
                                                  dptr(w) if w is not None else None,
                                                  None if null_bounds else C.byref(bounds),
                                                  C.byref(params) if params is not None else None,
                                                  C.byref(ctx) if ctx is not None else None)
    finally:
        L.dlg_set_trace(None)
    return r, p, tr, w, held


BOUNDED_STATS = ("evaluations", "clipped", "fallbacks", "held_steps", "kernels_ms", "mask_ms")


def bounded_last_stats():
    """dogleg_amd_bounded_last_stats as a dict: evaluations, steps with a clamped component, fallbacks, steps taken with a held
    variable (the oracle's evaluations, clipped, fallbacks, held_steps), ms in the feature's kernels and, of those, in the mask
    passes (DOGLEG_AMD_TIMING=1)"""
    out = np.zeros(6)
    n = lib().dogleg_amd_bounded_last_stats(dptr(out), 6)
    return dict(zip(BOUNDED_STATS, out[:n]))


def robust_last_stats():
    """dogleg_amd_robust_last_stats as a dict: evaluations, launches per evaluation, ms in the prelude (DOGLEG_AMD_TIMING=1)"""
    out = np.zeros(3)
    n = lib().dogleg_amd_robust_last_stats(dptr(out), 3)
    return dict(zip(("evaluations", "launches_per_evaluation", "prelude_ms"), out[:n]))


def optimize_dense_batch(p0s, N, M, cb, cookie, params=None):
    """dogleg_amd_optimize_dense_batch: p0s (B, N) start points, cb the address of a dogleg_callback_device_batch_t.
    Returns (rc, p (B, N), results): results a numpy record array with the fields of dogleg_amd_batch_result_t
    (norm2_x, trustregion, lambda_, iterations, evaluations, status)."""
    L = lib()
    p = np.array(p0s, dtype=np.float64, copy=True).reshape(-1, N)
    B = p.shape[0]
    res = (BatchResult * max(B, 1))()
    rc = L.dogleg_amd_optimize_dense_batch(dptr(p), B, N, M, cb, cookie, C.byref(params) if params is not None else None, res)
    return rc, p, _batch_results(res, B)


def _batch_results(res, B):
    """a (BatchResult * n) array as a numpy record array of its first B entries"""
    dt = np.dtype(dict(names=[n for n, _ in BatchResult._fields_], formats=[np.dtype(t) for _, t in BatchResult._fields_],
                       offsets=[getattr(BatchResult, n).offset for n, _ in BatchResult._fields_],
                       itemsize=C.sizeof(BatchResult)))
    return np.frombuffer(res, dtype=dt)[:B].copy()


def optimize_dense_products_batch(p0s, N, cb, cookie, params=None):
    """dogleg_amd_optimize_dense_products_batch: p0s (B, N) start points, cb the address of a
    dogleg_callback_device_batch_products_t; the layout of JtJ is params.JtJ_packed / JtJ_upper.  Returns (rc, p (B, N),
    results) as optimize_dense_batch."""
    L = lib()
    p = np.array(p0s, dtype=np.float64, copy=True).reshape(-1, N)
    B = p.shape[0]
    res = (BatchResult * max(B, 1))()
    rc = L.dogleg_amd_optimize_dense_products_batch(dptr(p), B, N, cb, cookie, C.byref(params) if params is not None else None,
                                                    res)
    return rc, p, _batch_results(res, B)


def dense_products_batch_uncertainty(p, N, cb, cookie, params=None, lam=None, want=("cov", "var"), fit=None):
    """dogleg_amd_dense_products_batch_uncertainty at the points p (B, N).  lam: (B,) or None (NULL: start at 0); want: which
    of "cov", "var" to ask for.  Returns dict(rc, status, lam (None if lam was None), cov (B, N, N) / var (B, N) as asked)."""
    L = lib()
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, N)
    B = p.shape[0]
    out = dict(lam=None if lam is None else np.array(lam, dtype=np.float64, copy=True).reshape(B))
    out["status"] = np.full(B, -1, dtype=np.int32)
    if "cov" in want:
        out["cov"] = np.zeros((B, N, N))
    if "var" in want:
        out["var"] = np.zeros((B, N))
    opt = lambda k: dptr(out[k]) if out.get(k) is not None else None
    out["rc"] = _call_fit("dogleg_amd_dense_products_batch_uncertainty", fit, dptr(p), B, N, cb, cookie,
                                                              C.byref(params) if params is not None else None,
                                                              opt("lam"), opt("cov"), opt("var"), iptr(out["status"]))
    return out


def batch_last_stats():
    """{rounds, ms_callback, ms_library} of the calling thread's last batch call (the times: DOGLEG_AMD_BATCH_TIMING=1)"""
    out = (C.c_double * 3)()
    lib().dogleg_amd_batch_last_stats(out, 3)
    return dict(rounds=int(out[0]), ms_callback=out[1], ms_library=out[2])


def dense_batch_uncertainty(p, N, M, cb, cookie, lam=None, want=("cov", "var", "factors"), fs=1, scale=None, fit=None):
    """dogleg_amd_dense_batch_uncertainty at the points p (B, N).  lam: (B,) or None (NULL: start at 0); want: which of
    "cov", "var", "factors" to ask for; scale: (B,) or a number for all, None: computed (<= 0).  Returns dict(rc, status,
    lam (None if lam was None), and cov (B, N, N) / var (B, N) / factors (B, M // max(fs, 1)) + scale (B,) as asked).
    fit: None, or batch_fit(...) / NULL_FIT for dogleg_amd_dense_batch_uncertainty_fit; so in the seven wrappers below."""
    L = lib()
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, N)
    B = p.shape[0]
    out = dict(lam=None if lam is None else np.array(lam, dtype=np.float64, copy=True).reshape(B))
    out["status"] = np.full(B, -1, dtype=np.int32)
    if "cov" in want:
        out["cov"] = np.zeros((B, N, N))
    if "var" in want:
        out["var"] = np.zeros((B, N))
    if "factors" in want:
        out["factors"] = np.zeros((B, M // max(fs, 1)))
        out["scale"] = np.full(B, -1.0) if scale is None else np.array(np.broadcast_to(scale, (B,)), dtype=np.float64)
    opt = lambda k: dptr(out[k]) if out.get(k) is not None else None
    out["rc"] = _call_fit("dogleg_amd_dense_batch_uncertainty", fit, dptr(p), B, N, M, cb, cookie, opt("lam"), opt("cov"), opt("var"),
                                                     opt("factors"), opt("scale"), fs, iptr(out["status"]))
    return out


NULL_FIT = object()          # fit=NULL_FIT: the ..._fit entry point with fit == NULL


def batch_fit(loss=None, weights=None, held=None):
    """the fit argument of the eight uncertainty / query wrappers (dogleg_amd_batch_fit_t): loss a BatchLoss, weights (B, M //
    featureSize) doubles and held (B, N) bytes -- numpy arrays (taken by their host address), DeviceArrays or raw addresses --
    each or None (NULL).  fit=None calls the entry point without _fit."""
    return dict(loss=loss, weights=weights, held=held)


def _call_fit(name, fit, *args):
    """the entry point `name`, or with a fit its ..._fit form: the same arguments, then the record"""
    L = lib()
    if fit is None:
        return getattr(L, name)(*args)
    name = name[:-len("_device")] + "_fit_device" if name.endswith("_device") else name + "_fit"
    if fit is NULL_FIT:
        return getattr(L, name)(*args, None)
    keep = []

    def addr(a, dtype):
        if a is None:
            return None
        if isinstance(a, np.ndarray):
            keep.append(np.ascontiguousarray(a, dtype=dtype))
            return keep[-1].ctypes.data
        return _dev(a).value

    loss = fit["loss"]
    rec = BatchFit(C.pointer(loss) if loss is not None else None, addr(fit["weights"], np.float64), addr(fit["held"], np.uint8))
    return getattr(L, name)(*args, C.byref(rec))


def batch_uncertainty_last_stats():
    """{launches, syncs, copies, ms_callback, ms_library} of the calling thread's last dense_batch_uncertainty (the times:
    DOGLEG_AMD_BATCH_TIMING=1)"""
    out = (C.c_double * 5)()
    lib().dogleg_amd_batch_uncertainty_last_stats(out, 5)
    return dict(launches=int(out[0]), syncs=int(out[1]), copies=int(out[2]), ms_callback=out[3], ms_library=out[4])


def _dev(a):
    """the device address of a DeviceArray, a raw address, or None"""
    if a is None:
        return None
    return C.c_void_p(a.ptr if isinstance(a, DeviceArray) else int(a))


def batch_device_span_ok(ptr, nbytes):
    """dlg_batch_device_span_ok: whether the device-resident batch entry points accept [ptr, ptr + nbytes)"""
    return bool(lib().dlg_batch_device_span_ok(_dev(ptr), nbytes))


def optimize_dense_batch_device(p_dev, B, N, M, cb, cookie, params, results_dev, lambda_dev=None, active_dev=None, stream=None):
    """dogleg_amd_optimize_dense_batch_device.  p_dev (B, N) doubles in/out, results_dev B dogleg_amd_batch_result_t,
    lambda_dev B doubles or None, active_dev B bytes or None: DeviceArrays or raw device addresses; stream: a hipStream_t as
    an integer, or None.  Returns rc."""
    return lib().dogleg_amd_optimize_dense_batch_device(_dev(p_dev), B, N, M, cb, cookie,
                                                        C.byref(params) if params is not None else None, _dev(results_dev),
                                                        _dev(lambda_dev), _dev(active_dev), _dev(stream))


def optimize_dense_products_batch_device(p_dev, B, N, cb, cookie, params, results_dev, lambda_dev=None, active_dev=None,
                                         stream=None):
    """dogleg_amd_optimize_dense_products_batch_device, the arguments as optimize_dense_batch_device.  Returns rc."""
    return lib().dogleg_amd_optimize_dense_products_batch_device(_dev(p_dev), B, N, cb, cookie,
                                                                 C.byref(params) if params is not None else None,
                                                                 _dev(results_dev), _dev(lambda_dev), _dev(active_dev),
                                                                 _dev(stream))


def optimize_dense_batch_robust(p0s, N, M, cb, cookie, loss, params=None, want_weights=True):
    """dogleg_amd_optimize_dense_batch_robust: as optimize_dense_batch with loss a BatchLoss (None: NULL).  Returns (rc, p (B, N),
    results, weights (B, M // max(featureSize, 1)) prefilled with -1, or None if not asked for); results["norm2_x"] is the
    robust cost."""
    L = lib()
    p = np.array(p0s, dtype=np.float64, copy=True).reshape(-1, N)
    B = p.shape[0]
    res = (BatchResult * max(B, 1))()
    fs = max(loss.featureSize, 1) if loss is not None else 1
    w = np.full((B, M // fs), -1.0) if want_weights else None
    rc = L.dogleg_amd_optimize_dense_batch_robust(dptr(p), B, N, M, cb, cookie, C.byref(params) if params is not None else None,
                                                  C.byref(loss) if loss is not None else None, res,
                                                  dptr(w) if w is not None else None)
    return rc, p, _batch_results(res, B), w


def optimize_dense_batch_robust_device(p_dev, B, N, M, cb, cookie, params, loss, results_dev, lambda_dev=None, weights_dev=None,
                                       active_dev=None, stream=None):
    """dogleg_amd_optimize_dense_batch_robust_device, the arguments as optimize_dense_batch_device; loss a BatchLoss (host),
    weights_dev (B, M // featureSize) doubles or None.  Returns rc."""
    return lib().dogleg_amd_optimize_dense_batch_robust_device(_dev(p_dev), B, N, M, cb, cookie,
                                                               C.byref(params) if params is not None else None,
                                                               C.byref(loss) if loss is not None else None, _dev(results_dev),
                                                               _dev(lambda_dev), _dev(weights_dev), _dev(active_dev),
                                                               _dev(stream))


def optimize_dense_batch_bounded(p0s, N, M, cb, cookie, lower, upper, loss=None, params=None, want_weights=None,
                                 want_held=True):
    """dogleg_amd_optimize_dense_batch_bounded: as optimize_dense_batch with lower, upper (B, N) arrays or None (NULL) and loss a
    BatchLoss or None (least squares).  Returns (rc, p (B, N), results, held (B, N) uint8 prefilled with 255 or None, weights
    (B, M // max(featureSize, 1)) prefilled with -1 or None: asked for by default where a loss is given)."""
    L = lib()
    p = np.array(p0s, dtype=np.float64, copy=True).reshape(-1, N)
    B = p.shape[0]
    res = (BatchResult * max(B, 1))()
    lo = None if lower is None else np.ascontiguousarray(lower, dtype=np.float64).reshape(B, N)
    hi = None if upper is None else np.ascontiguousarray(upper, dtype=np.float64).reshape(B, N)
    held = np.full((B, N), 255, dtype=np.uint8) if want_held else None
    if want_weights is None:
        want_weights = loss is not None
    fs = max(loss.featureSize, 1) if loss is not None else 1
    w = np.full((B, M // fs), -1.0) if want_weights else None
    addr = lambda a: None if a is None else a.ctypes.data
    bounds = BatchBounds(addr(lo), addr(hi), addr(held))
    rc = L.dogleg_amd_optimize_dense_batch_bounded(dptr(p), B, N, M, cb, cookie, C.byref(params) if params is not None else None,
                                                   C.byref(loss) if loss is not None else None, C.byref(bounds), res,
                                                   dptr(w) if w is not None else None)
    return rc, p, _batch_results(res, B), held, w


def optimize_dense_batch_bounded_device(p_dev, B, N, M, cb, cookie, params, loss, lower_dev, upper_dev, held_dev, results_dev,
                                        lambda_dev=None, weights_dev=None, active_dev=None, stream=None):
    """dogleg_amd_optimize_dense_batch_bounded_device, the arguments as optimize_dense_batch_robust_device; lower_dev, upper_dev
    (B, N) doubles and held_dev (B, N) bytes: DeviceArrays, raw addresses or None.  Returns rc."""
    raw = lambda a: None if a is None else _dev(a).value
    bounds = BatchBounds(raw(lower_dev), raw(upper_dev), raw(held_dev))
    return lib().dogleg_amd_optimize_dense_batch_bounded_device(_dev(p_dev), B, N, M, cb, cookie,
                                                                C.byref(params) if params is not None else None,
                                                                C.byref(loss) if loss is not None else None, C.byref(bounds),
                                                                _dev(results_dev), _dev(lambda_dev), _dev(weights_dev),
                                                                _dev(active_dev), _dev(stream))


def optimize_dense_products_batch_bounded(p0s, N, cb, cookie, lower, upper, params=None, want_held=True):
    """dogleg_amd_optimize_dense_products_batch_bounded: as optimize_dense_products_batch with lower, upper (B, N) arrays or None
    (NULL).  Returns (rc, p (B, N), results, held (B, N) uint8 prefilled with 255 or None)."""
    L = lib()
    p = np.array(p0s, dtype=np.float64, copy=True).reshape(-1, N)
    B = p.shape[0]
    res = (BatchResult * max(B, 1))()
    lo = None if lower is None else np.ascontiguousarray(lower, dtype=np.float64).reshape(B, N)
    hi = None if upper is None else np.ascontiguousarray(upper, dtype=np.float64).reshape(B, N)
    held = np.full((B, N), 255, dtype=np.uint8) if want_held else None
    addr = lambda a: None if a is None else a.ctypes.data
    bounds = BatchBounds(addr(lo), addr(hi), addr(held))
    rc = L.dogleg_amd_optimize_dense_products_batch_bounded(dptr(p), B, N, cb, cookie,
                                                            C.byref(params) if params is not None else None, C.byref(bounds), res)
    return rc, p, _batch_results(res, B), held


def optimize_dense_products_batch_bounded_device(p_dev, B, N, cb, cookie, params, lower_dev, upper_dev, held_dev, results_dev,
                                                 lambda_dev=None, active_dev=None, stream=None):
    """dogleg_amd_optimize_dense_products_batch_bounded_device, the arguments as optimize_dense_products_batch_device; lower_dev,
    upper_dev (B, N) doubles and held_dev (B, N) bytes: DeviceArrays, raw addresses or None.  Returns rc."""
    raw = lambda a: None if a is None else _dev(a).value
    bounds = BatchBounds(raw(lower_dev), raw(upper_dev), raw(held_dev))
    return lib().dogleg_amd_optimize_dense_products_batch_bounded_device(_dev(p_dev), B, N, cb, cookie,
                                                                         C.byref(params) if params is not None else None,
                                                                         C.byref(bounds), _dev(results_dev), _dev(lambda_dev),
                                                                         _dev(active_dev), _dev(stream))


def batch_model(kind, y_dev, Nmeas, width=0, height=0, t_dev=None, t_per_problem=False, scale_dev=None):
    """a dogleg_amd_batch_model_t: y_dev (B, Nmeas), t_dev (Nmeas,) or, with t_per_problem, (B, Nmeas), scale_dev (B, Nmeas):
    DeviceArrays or raw device addresses, None: NULL.  The caller keeps the record (and the arrays) alive while it is used"""
    raw = lambda a: None if a is None else _dev(a).value
    return BatchModel(kind, Nmeas, width, height, raw(y_dev), raw(t_dev), raw(scale_dev), 1 if t_per_problem else 0)


def batch_model_callback(model):
    """(cb, cookie, Nstate, Nmeas) of dogleg_amd_batch_model_callback on the record `model`: what every batch entry point that takes
    a dogleg_callback_device_batch_t is called with"""
    cb = C.cast(lib().dogleg_amd_batch_model_callback, C.c_void_p)
    return cb, C.c_void_p(C.addressof(model)), MODEL_NSTATE[model.kind], model.Nmeas


def batch_model_callback_invocations():
    """dogleg_amd_batch_model_callback_invocations: calls of the adapter callback in this process"""
    return int(lib().dogleg_amd_batch_model_callback_invocations())


def optimize_dense_batch_model(p0s, model, lower=None, upper=None, params=None, bounded=None, want_held=True):
    """dogleg_amd_optimize_dense_batch_model: p0s (B, N) host start points, model a BatchModel (None: NULL) whose arrays lie in
    device memory; lower, upper (B, N) host arrays or None.  bounded: whether a bounds record is passed at all (default: when a
    bound is given).  Returns (rc, p (B, N), results, held (B, N) uint8 prefilled with 255, or None without a bounds record)."""
    L = lib()
    N = MODEL_NSTATE.get(model.kind, 1) if model is not None else 1
    p = np.array(p0s, dtype=np.float64, copy=True).reshape(-1, N)
    B = p.shape[0]
    res = (BatchResult * max(B, 1))()
    if bounded is None:
        bounded = lower is not None or upper is not None
    lo = None if lower is None else np.ascontiguousarray(lower, dtype=np.float64).reshape(B, N)
    hi = None if upper is None else np.ascontiguousarray(upper, dtype=np.float64).reshape(B, N)
    held = np.full((B, N), 255, dtype=np.uint8) if bounded and want_held else None
    addr = lambda a: None if a is None else a.ctypes.data
    bounds = BatchBounds(addr(lo), addr(hi), addr(held))
    rc = L.dogleg_amd_optimize_dense_batch_model(dptr(p), B, C.byref(model) if model is not None else None,
                                                 C.byref(params) if params is not None else None,
                                                 C.byref(bounds) if bounded else None, res)
    return rc, p, _batch_results(res, B), held


def optimize_dense_batch_model_device(p_dev, B, model, params, results_dev, lower_dev=None, upper_dev=None, held_dev=None,
                                      lambda_dev=None, active_dev=None, stream=None, bounded=None):
    """dogleg_amd_optimize_dense_batch_model_device: the arguments as optimize_dense_batch_bounded_device without callback and
    loss; bounded: whether a bounds record is passed at all (default: when one of its arrays is given).  Returns rc."""
    raw = lambda a: None if a is None else _dev(a).value
    if bounded is None:
        bounded = lower_dev is not None or upper_dev is not None or held_dev is not None
    bounds = BatchBounds(raw(lower_dev), raw(upper_dev), raw(held_dev))
    return lib().dogleg_amd_optimize_dense_batch_model_device(_dev(p_dev), B, C.byref(model) if model is not None else None,
                                                              C.byref(params) if params is not None else None,
                                                              C.byref(bounds) if bounded else None, _dev(results_dev),
                                                              _dev(lambda_dev), _dev(active_dev), _dev(stream))


def batch_model_fisher_callback(model):
    """(cb, cookie, Nstate, Nmeas) of dogleg_amd_batch_model_fisher_callback on the record `model`: the rows of the Poisson
    likelihood, for the uncertainty, query and _fit calls (the solve entry points refuse it)"""
    cb = C.cast(lib().dogleg_amd_batch_model_fisher_callback, C.c_void_p)
    return cb, C.c_void_p(C.addressof(model)), MODEL_NSTATE[model.kind], model.Nmeas


def optimize_dense_batch_model_mle(p0s, model, likelihood, lower=None, upper=None, params=None, bounded=None, want_held=True):
    """dogleg_amd_optimize_dense_batch_model_mle: optimize_dense_batch_model with a likelihood (LIKELIHOOD_GAUSS or
    LIKELIHOOD_POISSON of ctypes_defs); the same arguments otherwise and the same return value"""
    L = lib()
    N = MODEL_NSTATE.get(model.kind, 1) if model is not None else 1
    p = np.array(p0s, dtype=np.float64, copy=True).reshape(-1, N)
    B = p.shape[0]
    res = (BatchResult * max(B, 1))()
    if bounded is None:
        bounded = lower is not None or upper is not None
    lo = None if lower is None else np.ascontiguousarray(lower, dtype=np.float64).reshape(B, N)
    hi = None if upper is None else np.ascontiguousarray(upper, dtype=np.float64).reshape(B, N)
    held = np.full((B, N), 255, dtype=np.uint8) if bounded and want_held else None
    addr = lambda a: None if a is None else a.ctypes.data
    bounds = BatchBounds(addr(lo), addr(hi), addr(held))
    rc = L.dogleg_amd_optimize_dense_batch_model_mle(dptr(p), B, C.byref(model) if model is not None else None, likelihood,
                                                     C.byref(params) if params is not None else None,
                                                     C.byref(bounds) if bounded else None, res)
    return rc, p, _batch_results(res, B), held


def optimize_dense_batch_model_mle_device(p_dev, B, model, likelihood, params, results_dev, lower_dev=None, upper_dev=None,
                                          held_dev=None, lambda_dev=None, active_dev=None, stream=None, bounded=None):
    """dogleg_amd_optimize_dense_batch_model_mle_device: optimize_dense_batch_model_device with a likelihood.  Returns rc."""
    raw = lambda a: None if a is None else _dev(a).value
    if bounded is None:
        bounded = lower_dev is not None or upper_dev is not None or held_dev is not None
    bounds = BatchBounds(raw(lower_dev), raw(upper_dev), raw(held_dev))
    return lib().dogleg_amd_optimize_dense_batch_model_mle_device(_dev(p_dev), B, C.byref(model) if model is not None else None,
                                                                  likelihood, C.byref(params) if params is not None else None,
                                                                  C.byref(bounds) if bounded else None, _dev(results_dev),
                                                                  _dev(lambda_dev), _dev(active_dev), _dev(stream))


def _held_addr(held, keep):
    """the address of a held array: a numpy array by its host address (kept alive in `keep`), a DeviceArray or a raw address"""
    if held is None:
        return None
    if isinstance(held, np.ndarray):
        keep.append(np.ascontiguousarray(held, dtype=np.uint8))
        return keep[-1].ctypes.data
    return _dev(held)


def dense_batch_model_uncertainty(p, model, likelihood, lam=None, want=("cov", "var", "factors"), fs=1, scale=None, held=None):
    """dogleg_amd_dense_batch_model_uncertainty at the points p (B, N): dense_batch_uncertainty with a BatchModel (None: NULL)
    and a likelihood instead of N, M, cb and cookie; held: (B, N) uint8 or None instead of a fit.  The same dict."""
    L = lib()
    N = MODEL_NSTATE.get(model.kind, 1) if model is not None else 1
    M = model.Nmeas if model is not None else 1
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, N)
    B = p.shape[0]
    out = dict(lam=None if lam is None else np.array(lam, dtype=np.float64, copy=True).reshape(B))
    out["status"] = np.full(B, -1, dtype=np.int32)
    if "cov" in want:
        out["cov"] = np.zeros((B, N, N))
    if "var" in want:
        out["var"] = np.zeros((B, N))
    if "factors" in want:
        out["factors"] = np.zeros((B, M // max(fs, 1)))
        out["scale"] = np.full(B, -1.0) if scale is None else np.array(np.broadcast_to(scale, (B,)), dtype=np.float64)
    opt = lambda k: dptr(out[k]) if out.get(k) is not None else None
    keep = []
    out["rc"] = L.dogleg_amd_dense_batch_model_uncertainty(dptr(p), B, C.byref(model) if model is not None else None, likelihood,
                                                           opt("lam"), opt("cov"), opt("var"), opt("factors"), opt("scale"), fs,
                                                           iptr(out["status"]), _held_addr(held, keep))
    return out


def dense_batch_model_uncertainty_device(p_dev, B, model, likelihood, status_dev, lambda_dev=None, cov_dev=None, var_dev=None,
                                         factors_dev=None, scale_dev=None, fs=1, held_dev=None, active_dev=None, stream=None):
    """dogleg_amd_dense_batch_model_uncertainty_device: every array a DeviceArray or a raw device address (None: NULL).
    Returns rc."""
    return lib().dogleg_amd_dense_batch_model_uncertainty_device(_dev(p_dev), B, C.byref(model) if model is not None else None,
                                                                 likelihood, _dev(lambda_dev), _dev(cov_dev), _dev(var_dev),
                                                                 _dev(factors_dev), _dev(scale_dev), fs, _dev(status_dev),
                                                                 _dev(held_dev), _dev(active_dev), _dev(stream))


def dense_batch_model_query_covariance(p, model, likelihood, Jq, lam=None, nobs=-1, held=None):
    """dogleg_amd_dense_batch_model_query_covariance at the points p (B, N): dense_batch_query_covariance with a BatchModel and a
    likelihood instead of N, M, cb and cookie; held: (B, N) uint8 or None instead of a fit.  The same dict."""
    N = MODEL_NSTATE.get(model.kind, 1) if model is not None else np.shape(Jq)[-1]
    p, Jq, out = _query_arrays(p, N, Jq, lam)
    keep = []
    out["rc"] = lib().dogleg_amd_dense_batch_model_query_covariance(dptr(p), p.shape[0], C.byref(model) if model is not None else None,
                                                                    likelihood, dptr(out["lam"]) if lam is not None else None,
                                                                    dptr(Jq), Jq.shape[1], Jq.shape[2], nobs, dptr(out["out"]),
                                                                    iptr(out["status"]), _held_addr(held, keep))
    return out


def dense_batch_model_query_covariance_device(p_dev, B, model, likelihood, Jq_dev, Nq, Q, out_dev, status_dev, nobs=-1,
                                              lambda_dev=None, held_dev=None, active_dev=None, stream=None):
    """dogleg_amd_dense_batch_model_query_covariance_device: every array a DeviceArray or a raw device address (None: NULL).
    Returns rc."""
    return lib().dogleg_amd_dense_batch_model_query_covariance_device(_dev(p_dev), B, C.byref(model) if model is not None else None,
                                                                      likelihood, _dev(lambda_dev), _dev(Jq_dev), Nq, Q, nobs,
                                                                      _dev(out_dev), _dev(status_dev), _dev(held_dev),
                                                                      _dev(active_dev), _dev(stream))


def batch_camera(model, dtype, raw_dev, sensor=(0, 0), offset_dev=None, gain_inv_dev=None, readvar_dev=None, origin_dev=None):
    """a dogleg_amd_batch_camera_t: model a BatchModel with y NULL (batch_model(kind, None, ...)), dtype a DATA_* of ctypes_defs,
    raw_dev (B, Nmeas) readings of that type; sensor = (width, height), the three float maps (height, width) and origin_dev (B, 2)
    int32: DeviceArrays or raw device addresses, None: NULL.  The caller keeps the record (and the arrays) alive while it is used"""
    raw = lambda a: None if a is None else _dev(a).value
    return BatchCamera(model, dtype, raw(raw_dev), sensor[0], sensor[1], raw(offset_dev), raw(gain_inv_dev), raw(readvar_dev),
                       raw(origin_dev))


def batch_camera_callback(camera, fisher=False):
    """(cb, cookie, Nstate, Nmeas) of dogleg_amd_batch_camera_callback (fisher: of dogleg_amd_batch_camera_fisher_callback, which
    the solve entry points refuse) on the record `camera`"""
    L = lib()
    cb = C.cast(L.dogleg_amd_batch_camera_fisher_callback if fisher else L.dogleg_amd_batch_camera_callback, C.c_void_p)
    return cb, C.c_void_p(C.addressof(camera)), MODEL_NSTATE[camera.model.kind], camera.model.Nmeas


def _camera_shape(camera):
    if camera is None:
        return 1, 1, None
    return MODEL_NSTATE.get(camera.model.kind, 1), camera.model.Nmeas, C.byref(camera)


def optimize_dense_batch_camera(p0s, camera, likelihood, lower=None, upper=None, params=None, bounded=None, want_held=True):
    """dogleg_amd_optimize_dense_batch_camera: optimize_dense_batch_model_mle with a BatchCamera (None: NULL) instead of the model;
    the same arguments otherwise and the same return value"""
    N, _, cam = _camera_shape(camera)
    p = np.array(p0s, dtype=np.float64, copy=True).reshape(-1, N)
    B = p.shape[0]
    res = (BatchResult * max(B, 1))()
    if bounded is None:
        bounded = lower is not None or upper is not None
    lo = None if lower is None else np.ascontiguousarray(lower, dtype=np.float64).reshape(B, N)
    hi = None if upper is None else np.ascontiguousarray(upper, dtype=np.float64).reshape(B, N)
    held = np.full((B, N), 255, dtype=np.uint8) if bounded and want_held else None
    addr = lambda a: None if a is None else a.ctypes.data
    bounds = BatchBounds(addr(lo), addr(hi), addr(held))
    rc = lib().dogleg_amd_optimize_dense_batch_camera(dptr(p), B, cam, likelihood, C.byref(params) if params is not None else None,
                                                      C.byref(bounds) if bounded else None, res)
    return rc, p, _batch_results(res, B), held


def optimize_dense_batch_camera_device(p_dev, B, camera, likelihood, params, results_dev, lower_dev=None, upper_dev=None,
                                       held_dev=None, lambda_dev=None, active_dev=None, stream=None, bounded=None):
    """dogleg_amd_optimize_dense_batch_camera_device: optimize_dense_batch_model_mle_device with a BatchCamera.  Returns rc."""
    raw = lambda a: None if a is None else _dev(a).value
    if bounded is None:
        bounded = lower_dev is not None or upper_dev is not None or held_dev is not None
    bounds = BatchBounds(raw(lower_dev), raw(upper_dev), raw(held_dev))
    return lib().dogleg_amd_optimize_dense_batch_camera_device(_dev(p_dev), B, _camera_shape(camera)[2], likelihood,
                                                               C.byref(params) if params is not None else None,
                                                               C.byref(bounds) if bounded else None, _dev(results_dev),
                                                               _dev(lambda_dev), _dev(active_dev), _dev(stream))


def dense_batch_camera_uncertainty(p, camera, likelihood, lam=None, want=("cov", "var", "factors"), fs=1, scale=None, held=None):
    """dogleg_amd_dense_batch_camera_uncertainty at the points p (B, N): dense_batch_model_uncertainty with a BatchCamera (None:
    NULL) instead of the model.  The same dict."""
    N, M, cam = _camera_shape(camera)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, N)
    B = p.shape[0]
    out = dict(lam=None if lam is None else np.array(lam, dtype=np.float64, copy=True).reshape(B))
    out["status"] = np.full(B, -1, dtype=np.int32)
    if "cov" in want:
        out["cov"] = np.zeros((B, N, N))
    if "var" in want:
        out["var"] = np.zeros((B, N))
    if "factors" in want:
        out["factors"] = np.zeros((B, M // max(fs, 1)))
        out["scale"] = np.full(B, -1.0) if scale is None else np.array(np.broadcast_to(scale, (B,)), dtype=np.float64)
    opt = lambda k: dptr(out[k]) if out.get(k) is not None else None
    keep = []
    out["rc"] = lib().dogleg_amd_dense_batch_camera_uncertainty(dptr(p), B, cam, likelihood, opt("lam"), opt("cov"), opt("var"),
                                                                opt("factors"), opt("scale"), fs, iptr(out["status"]),
                                                                _held_addr(held, keep))
    return out


def dense_batch_camera_uncertainty_device(p_dev, B, camera, likelihood, status_dev, lambda_dev=None, cov_dev=None, var_dev=None,
                                          factors_dev=None, scale_dev=None, fs=1, held_dev=None, active_dev=None, stream=None):
    """dogleg_amd_dense_batch_camera_uncertainty_device: every array a DeviceArray or a raw device address (None: NULL).
    Returns rc."""
    return lib().dogleg_amd_dense_batch_camera_uncertainty_device(_dev(p_dev), B, _camera_shape(camera)[2], likelihood,
                                                                  _dev(lambda_dev), _dev(cov_dev), _dev(var_dev), _dev(factors_dev),
                                                                  _dev(scale_dev), fs, _dev(status_dev), _dev(held_dev),
                                                                  _dev(active_dev), _dev(stream))


def dense_batch_camera_query_covariance(p, camera, likelihood, Jq, lam=None, nobs=-1, held=None):
    """dogleg_amd_dense_batch_camera_query_covariance at the points p (B, N): dense_batch_model_query_covariance with a BatchCamera
    instead of the model.  The same dict."""
    N = MODEL_NSTATE.get(camera.model.kind, 1) if camera is not None else np.shape(Jq)[-1]
    p, Jq, out = _query_arrays(p, N, Jq, lam)
    keep = []
    out["rc"] = lib().dogleg_amd_dense_batch_camera_query_covariance(dptr(p), p.shape[0], _camera_shape(camera)[2], likelihood,
                                                                     dptr(out["lam"]) if lam is not None else None, dptr(Jq),
                                                                     Jq.shape[1], Jq.shape[2], nobs, dptr(out["out"]),
                                                                     iptr(out["status"]), _held_addr(held, keep))
    return out


def dense_batch_camera_query_covariance_device(p_dev, B, camera, likelihood, Jq_dev, Nq, Q, out_dev, status_dev, nobs=-1,
                                               lambda_dev=None, held_dev=None, active_dev=None, stream=None):
    """dogleg_amd_dense_batch_camera_query_covariance_device: every array a DeviceArray or a raw device address (None: NULL).
    Returns rc."""
    return lib().dogleg_amd_dense_batch_camera_query_covariance_device(_dev(p_dev), B, _camera_shape(camera)[2], likelihood,
                                                                       _dev(lambda_dev), _dev(Jq_dev), Nq, Q, nobs, _dev(out_dev),
                                                                       _dev(status_dev), _dev(held_dev), _dev(active_dev),
                                                                       _dev(stream))


def batch_results_from_device(results_dev, B):
    """the record array of _batch_results from B dogleg_amd_batch_result_t in a DeviceArray"""
    raw = results_dev.numpy().view(np.uint8)[:B * C.sizeof(BatchResult)]
    return _batch_results((BatchResult * B).from_buffer_copy(raw.tobytes()), B)


def dense_batch_uncertainty_device(p_dev, B, N, M, cb, cookie, status_dev, lambda_dev=None, cov_dev=None, var_dev=None,
                                   factors_dev=None, scale_dev=None, fs=1, active_dev=None, stream=None, fit=None):
    """dogleg_amd_dense_batch_uncertainty_device: every array a DeviceArray or a raw device address (None: NULL).  Returns rc."""
    return _call_fit("dogleg_amd_dense_batch_uncertainty_device", fit, _dev(p_dev), B, N, M, cb, cookie, _dev(lambda_dev), _dev(cov_dev),
                                                           _dev(var_dev), _dev(factors_dev), _dev(scale_dev), fs,
                                                           _dev(status_dev), _dev(active_dev), _dev(stream))


def dense_products_batch_uncertainty_device(p_dev, B, N, cb, cookie, params, status_dev, lambda_dev=None, cov_dev=None,
                                            var_dev=None, active_dev=None, stream=None, fit=None):
    """dogleg_amd_dense_products_batch_uncertainty_device, as dense_batch_uncertainty_device.  Returns rc."""
    return _call_fit("dogleg_amd_dense_products_batch_uncertainty_device", fit, _dev(p_dev), B, N, cb, cookie,
                                                                    C.byref(params) if params is not None else None,
                                                                    _dev(lambda_dev), _dev(cov_dev), _dev(var_dev),
                                                                    _dev(status_dev), _dev(active_dev), _dev(stream))


def _query_arrays(p, N, Jq, lam):
    """(p (B, N), Jq (B, Nq, Q, N), the dict of outputs) of the host-pointer batch query calls"""
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, N)
    B = p.shape[0]
    Jq = np.ascontiguousarray(Jq, dtype=np.float64)
    assert Jq.ndim == 4 and Jq.shape[0] == B and Jq.shape[3] == N, Jq.shape
    out = dict(lam=None if lam is None else np.array(lam, dtype=np.float64, copy=True).reshape(B),
               status=np.full(B, -1, dtype=np.int32), out=np.zeros((B, Jq.shape[1], Jq.shape[2], Jq.shape[2])))
    return p, Jq, out


def dense_batch_query_covariance(p, N, M, cb, cookie, Jq, lam=None, nobs=-1, fit=None):
    """dogleg_amd_dense_batch_query_covariance at the points p (B, N): Jq (B, Nq, Qrows, N); lam: (B,) or None (NULL: start at
    0); nobs < 0: Jq Sigma Jq^T, otherwise the observations-only form over the first nobs measurements.  Returns dict(rc,
    status, lam (None if lam was None), out (B, Nq, Qrows, Qrows))."""
    p, Jq, out = _query_arrays(p, N, Jq, lam)
    out["rc"] = _call_fit("dogleg_amd_dense_batch_query_covariance", fit, dptr(p), p.shape[0], N, M, cb, cookie,
                                                              dptr(out["lam"]) if lam is not None else None, dptr(Jq),
                                                              Jq.shape[1], Jq.shape[2], nobs, dptr(out["out"]), iptr(out["status"]))
    return out


def dense_products_batch_query_covariance(p, N, cb, cookie, Jq, params=None, lam=None, fit=None):
    """dogleg_amd_dense_products_batch_query_covariance, as dense_batch_query_covariance (the plain form only); the layout of
    JtJ is params.JtJ_packed / JtJ_upper."""
    p, Jq, out = _query_arrays(p, N, Jq, lam)
    out["rc"] = _call_fit("dogleg_amd_dense_products_batch_query_covariance", fit, dptr(p), p.shape[0], N, cb, cookie,
                                                                       C.byref(params) if params is not None else None,
                                                                       dptr(out["lam"]) if lam is not None else None, dptr(Jq),
                                                                       Jq.shape[1], Jq.shape[2], dptr(out["out"]),
                                                                       iptr(out["status"]))
    return out


def dense_batch_query_covariance_device(p_dev, B, N, M, cb, cookie, Jq_dev, Nq, Q, out_dev, status_dev, nobs=-1, lambda_dev=None,
                                        active_dev=None, stream=None, fit=None):
    """dogleg_amd_dense_batch_query_covariance_device: every array a DeviceArray or a raw device address (None: NULL).
    Returns rc."""
    return _call_fit("dogleg_amd_dense_batch_query_covariance_device", fit, _dev(p_dev), B, N, M, cb, cookie, _dev(lambda_dev), _dev(Jq_dev),
                                                                Nq, Q, nobs, _dev(out_dev), _dev(status_dev), _dev(active_dev),
                                                                _dev(stream))


def dense_products_batch_query_covariance_device(p_dev, B, N, cb, cookie, params, Jq_dev, Nq, Q, out_dev, status_dev,
                                                 lambda_dev=None, active_dev=None, stream=None, fit=None):
    """dogleg_amd_dense_products_batch_query_covariance_device, as dense_batch_query_covariance_device.  Returns rc."""
    return _call_fit("dogleg_amd_dense_products_batch_query_covariance_device", fit, _dev(p_dev), B, N, cb, cookie,
                                                                         C.byref(params) if params is not None else None,
                                                                         _dev(lambda_dev), _dev(Jq_dev), Nq, Q, _dev(out_dev),
                                                                         _dev(status_dev), _dev(active_dev), _dev(stream))


def jacobian_colouring(N, M, Jp, Ji):
    """dogleg_amd_jacobian_colouring (host only): (ncolours or -1, colour[N]) of the first-fit colouring of a Jt pattern"""
    Jp = np.ascontiguousarray(Jp, dtype=np.int32)
    Ji = np.ascontiguousarray(Ji, dtype=np.int32)
    colour = np.full(N, -1, dtype=np.int32)
    return lib().dogleg_amd_jacobian_colouring(N, M, iptr(Jp), iptr(Ji), iptr(colour)), colour


def check_jacobian_device(p0, N, M, nnz, Jp, Ji, cb, cookie, delta=0.0, rtol=0.0, atol=0.0, flags=0, max_bad=64,
                          want_var_error=True):
    """dogleg_amd_check_jacobian_device.  nnz == 0: dense (Jp, Ji ignored).  cb: address of a dogleg_callback_device_t.
    Returns dict(rc, report (the fields of dogleg_amd_jacobian_report_t), var_error (N,) or None, bad: list of
    (problem, var, meas, reported, observed))."""
    L = lib()
    p0 = np.ascontiguousarray(p0, dtype=np.float64)
    if nnz > 0:
        Jp = np.ascontiguousarray(Jp, dtype=np.int32)
        Ji = np.ascontiguousarray(Ji, dtype=np.int32)
    rep = JacobianReport()
    ve = np.zeros(N) if want_var_error else None
    bad = (JacobianEntry * max(max_bad, 1))()
    rc = L.dogleg_amd_check_jacobian_device(dptr(p0), N, M, nnz, iptr(Jp) if nnz > 0 else None, iptr(Ji) if nnz > 0 else None,
                                            cb, cookie, delta, rtol, atol, flags, C.byref(rep),
                                            dptr(ve) if want_var_error else None, bad, max_bad)
    return dict(rc=rc, report=rep.asdict(), var_error=ve, bad=[bad[k].astuple() for k in range(max(rc, 0))])


def check_jacobian_device_batch(p0s, N, M, cb, cookie, delta=0.0, rtol=0.0, atol=0.0, max_bad=64):
    """dogleg_amd_check_jacobian_device_batch at the points p0s (B, N).  cb: address of a dogleg_callback_device_batch_t.
    Returns dict(rc, reports: list of dicts, one per problem, bad: list of (problem, var, meas, reported, observed))."""
    L = lib()
    p = np.ascontiguousarray(p0s, dtype=np.float64).reshape(-1, N)
    B = p.shape[0]
    reps = (JacobianReport * max(B, 1))()
    bad = (JacobianEntry * max(max_bad, 1))()
    n = C.c_longlong(0)
    rc = L.dogleg_amd_check_jacobian_device_batch(dptr(p), B, N, M, cb, cookie, delta, rtol, atol, reps, bad, max_bad, C.byref(n))
    return dict(rc=rc, reports=[reps[b].asdict() for b in range(B)], bad=[bad[k].astuple() for k in range(n.value)])


def check_jacobian_last_stats():
    """{callbacks, launches, syncs, copies, ms_callback, ms_library} of the calling thread's last Jacobian check (the
    times: DOGLEG_AMD_CHECK_TIMING=1, single problem)"""
    out = (C.c_double * 6)()
    lib().dogleg_amd_check_jacobian_last_stats(out, 6)
    return dict(callbacks=int(out[0]), launches=int(out[1]), syncs=int(out[2]), copies=int(out[3]), ms_callback=out[4],
                ms_library=out[5])


SYM_STAT_NAMES = ["var_blocks", "supernodes", "levels", "nnz_JtJ_lower", "nnz_L", "panel_doubles",
                  "factor_flops", "max_panel", "asm_tasks", "update_items", "relpos", "out_blocks",
                  "contribs", "update_subtasks", "solve_scratch", "jtx_tasks", "asm_mfma_tasks",
                  "asm_kgroups", "asm_shapes", "sym_hash"]


def covariance_plan_probe(N, M, Jp, Ji, r0, nr, c0, nc):
    """host only: (chunk of each request, {chunks, pair visits, most distinct variables in a chunk}) of a request list"""
    L = lib()
    r0, nr, c0, nc = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.int32) for a in (r0, nr, c0, nc))
    ch = np.zeros(max(len(r0), 1), dtype=np.int32)
    st = (C.c_long * 3)()
    _ck(L.dlg_covariance_plan_probe(N, M, iptr(Jp), iptr(Ji), len(r0), iptr(r0), iptr(nr), iptr(c0), iptr(nc),
                                    iptr(ch), st, 3), "covariance_plan_probe")
    return ch[:len(r0)], dict(chunks=st[0], visits=st[1], maxvar=st[2])


def query_covariance_plan_probe(N, M, Jp, Ji, qrow, rowptr, var):
    """host only: (chunk of each query, {chunks, pair visits, most rows in a chunk}) of a query batch"""
    L = lib()
    Jp = np.ascontiguousarray(Jp, dtype=np.int32)
    Ji = np.ascontiguousarray(Ji, dtype=np.int32)
    qrow, rowptr, var = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.int32) for a in (qrow, rowptr, var))
    nq = len(qrow) - 1
    ch = np.zeros(max(nq, 1), dtype=np.int32)
    st = (C.c_long * 3)()
    _ck(L.dlg_query_covariance_plan_probe(N, M, iptr(Jp), iptr(Ji), nq, iptr(qrow), iptr(rowptr), iptr(var), iptr(ch),
                                          st, 3), "query_covariance_plan_probe")
    return ch[:nq], dict(chunks=st[0], visits=st[1], maxrows=st[2])


def covariance_entries_probe(N, M, Jp, Ji, row, col):
    """host only: (whether each entry (row[e], col[e]) is in the structure of the factor, {nnz: entries of that structure
    (lower triangle with the diagonal), front_doubles: the selected inverse's front scratch})"""
    L = lib()
    Jp = np.ascontiguousarray(Jp, dtype=np.int32)
    Ji = np.ascontiguousarray(Ji, dtype=np.int32)
    row, col = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.int32) for a in (row, col))
    ins = np.zeros(max(len(row), 1), dtype=np.int32)
    st = (C.c_long * 3)()
    _ck(L.dlg_covariance_entries_probe(N, M, iptr(Jp), iptr(Ji), len(row), iptr(row), iptr(col), iptr(ins), st, 3),
        "covariance_entries_probe")
    return ins[:len(row)].astype(bool), dict(nnz=st[0], front_doubles=st[1], wmax=st[2])


def symbolic_probe(N, M, Jp, Ji, row0=0, row1=None, want_perm=False):
    """Host-only symbolic analysis of a Jt pattern: dict of statistics (+ perm)."""
    L = lib()
    Jp = np.ascontiguousarray(Jp, dtype=np.int32)
    Ji = np.ascontiguousarray(Ji, dtype=np.int32)
    st = (C.c_long * len(SYM_STAT_NAMES))()
    perm = np.zeros(N, dtype=np.int32) if want_perm else None
    _ck(L.dlg_sparse_symbolic_probe(N, M, iptr(Jp), iptr(Ji), row0, M if row1 is None else row1,
                                    st, len(SYM_STAT_NAMES), iptr(perm) if want_perm else None),
        "symbolic probe")
    d = {k: (st[i] & (2**64 - 1) if k.endswith("_hash") else st[i]) for i, k in enumerate(SYM_STAT_NAMES)}
    return (d, perm) if want_perm else d


PART_STAT_NAMES = ["cut_level", "supernodes_above_cut", "supernodes_mine", "rows_mine", "reduced_doubles",
                   "panel_doubles", "nnz_mine", "sym_hash"]


def partition_probe(N, M, Jp, Ji, rank, nranks):
    """Host-only: the subtree partition of a Jt pattern as rank `rank` of `nranks` sees it.
    Returns (dict of statistics, bool array row_is_mine[M])."""
    L = lib()
    Jp = np.ascontiguousarray(Jp, dtype=np.int32)
    Ji = np.ascontiguousarray(Ji, dtype=np.int32)
    st = (C.c_long * len(PART_STAT_NAMES))()
    own = np.zeros(M, dtype=np.uint8)
    _ck(L.dlg_sparse_partition_probe(N, M, iptr(Jp), iptr(Ji), rank, nranks, st, len(PART_STAT_NAMES),
                                     own.ctypes.data_as(C.c_char_p)), "partition probe")
    return {k: (st[i] & (2**64 - 1) if k.endswith("_hash") else st[i]) for i, k in enumerate(PART_STAT_NAMES)}, own.astype(bool)


REGION_STAT_NAMES = ["level0", "supernodes", "workgroups", "lds_bytes", "sliced_workgroups", "hbm_update_matrices",
                     "schedule_hash", "level_params_hash"]


def region_probe(N, M, Jp, Ji, ncu=256):
    """Host-only: the one-launch region of the factorisation of a pattern on a chip with `ncu` CUs, checked
    (raises DlgError on a violated invariant).  Returns a dict of REGION_STAT_NAMES; the two hashes (64-bit FNV-1a
    over the fields of the schedule / of the per-level launch parameters) as unsigned integers."""
    L = lib()
    Jp = np.ascontiguousarray(Jp, dtype=np.int32)
    Ji = np.ascontiguousarray(Ji, dtype=np.int32)
    st = (C.c_long * len(REGION_STAT_NAMES))()
    _ck(L.dlg_sparse_region_probe(N, M, iptr(Jp), iptr(Ji), ncu, st, len(REGION_STAT_NAMES)), "region probe")
    return {k: (st[i] & (2**64 - 1) if k.endswith("_hash") else st[i]) for i, k in enumerate(REGION_STAT_NAMES)}


def rccl_unique_id():
    """128 bytes from ncclGetUniqueId (rank 0 creates it and hands it to the others)"""
    buf = (C.c_char * 128)()
    _ck(lib().dlg_rccl_unique_id(C.cast(buf, C.c_void_p)), "rccl_unique_id")
    return bytes(buf)


class DeviceArray:
    """A hipMalloc'ed buffer filled from / read back into numpy (harness helper)."""

    def __init__(self, arr=None, nbytes=None, dtype=np.float64):
        L = lib()
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            nbytes, dtype = arr.nbytes, arr.dtype
        self.nbytes, self.dtype = nbytes, np.dtype(dtype)
        self.ptr = L.dlg_mem_alloc(nbytes)
        if not self.ptr:
            raise DlgError(L.dlg_last_error().decode())
        if arr is not None:
            _ck(L.dlg_mem_upload(self.ptr, arr.ctypes.data, nbytes), "upload")
        else:
            _ck(L.dlg_mem_zero(self.ptr, nbytes), "memset")

    def numpy(self, shape=None):
        out = np.zeros(self.nbytes // self.dtype.itemsize, dtype=self.dtype)
        _ck(lib().dlg_mem_download(out.ctypes.data, self.ptr, self.nbytes), "download")
        return out.reshape(shape) if shape is not None else out

    def free(self):
        if self.ptr:
            lib().dlg_mem_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Backend:
    """Thin OO wrapper over the dlg_backend C-ABI (include/dlg_backend.h)."""

    def __init__(self, solve_type, N, M, nnz=0, flags=0, device=-1):
        self.L = lib()
        self.h = C.c_void_p()
        self.N, self.M, self.nnz, self.type = N, M, nnz, solve_type
        _ck(self.L.dlg_backend_create(C.byref(self.h), solve_type, N, M, nnz, flags, device),
            "dlg_backend_create")
        self._keep = []
        self._pnew_ptr = None
        self._pnew = None

    def close(self):
        if self.h:
            self.L.dlg_backend_destroy(self.h)
            self.h = C.c_void_p()
        if self._pnew_ptr:
            self.L.dlg_host_free(self._pnew_ptr)
            self._pnew_ptr, self._pnew = None, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_profiling(self, on=True, only=None, every=1):
        """only: names of the phases to time (PROF_NAMES), default all; every: time every n-th occurrence only"""
        v = (1 if on else 0) if only is None else sum(2 << PROF_NAMES.index(n) for n in only)
        if v and every > 1:
            v |= min(int(every), 255) << 16
        _ck(self.L.dlg_backend_set_profiling(self.h, v), "set_profiling")

    def profile(self):
        """{phase: (total_ms, launches)} since set_profiling(True)"""
        n = len(PROF_NAMES)
        ms = (C.c_double * n)()
        cnt = (C.c_long * n)()
        _ck(self.L.dlg_backend_get_profile(self.h, ms, cnt, n), "get_profile")
        return {PROF_NAMES[i]: (ms[i], cnt[i]) for i in range(n)}

    def profile_early(self):
        """{phase: (total_ms, launches)} of the launches that returned early behind a failed factorisation"""
        n = len(PROF_NAMES)
        ms = (C.c_double * n)()
        cnt = (C.c_long * n)()
        _ck(self.L.dlg_backend_get_profile_early(self.h, ms, cnt, n), "get_profile_early")
        return {PROF_NAMES[i]: (ms[i], cnt[i]) for i in range(n)}

    def set_stream(self, stream_ptr):
        _ck(self.L.dlg_backend_set_stream(self.h, C.c_void_p(stream_ptr)), "set_stream")

    def set_shard(self, row0, row1, fn=None):
        cb = ALLREDUCE_FN(fn) if fn is not None else None
        self._allreduce_cb = cb                 # must outlive the backend: the C side keeps the pointer
        _ck(self.L.dlg_backend_set_shard(self.h, row0, row1,
                                         C.cast(cb, C.c_void_p) if cb else None, None), "set_shard")

    def set_speculation(self, on=True):
        """assemble JtJ beside Jt*x at every eval (for callers that expect to factorise the point)"""
        _ck(self.L.dlg_backend_set_speculation(self.h, 1 if on else 0), "set_speculation")

    def set_defer_tail(self, on=True):
        """dlg_take_step returns before the expected improvement's pass over J (K8): step_tail() has the value"""
        _ck(self.L.dlg_backend_set_defer_tail(self.h, 1 if on else 0), "set_defer_tail")

    def step_tail(self):
        """the expected improvement of the last step taken with set_defer_tail (and its p_new complete)"""
        v = C.c_double()
        _ck(self.L.dlg_step_tail(self.h, C.byref(v)), "step_tail")
        return v.value

    def step_tail_pending(self):
        return bool(self.L.dlg_step_tail_pending(self.h))

    def ei_source(self):
        """(the last expected improvement came from the solved system -- no pass over J --, pivot ratio of the factor)"""
        f, r = C.c_int(), C.c_double()
        _ck(self.L.dlg_backend_ei_source(self.h, C.byref(f), C.byref(r)), "ei_source")
        return bool(f.value), r.value

    def set_allreduce(self, fn):
        """host-synchronous sum-all-reduce hook (fallback / logical ranks on one device)"""
        cb = ALLREDUCE_FN(fn) if fn is not None else None
        self._allreduce_cb = cb
        _ck(self.L.dlg_backend_set_allreduce(self.h, C.cast(cb, C.c_void_p) if cb else None, None), "set_allreduce")

    def set_partition(self, rank, nranks):
        """sparse: subtree partition over nranks ranks (before set_pattern)"""
        _ck(self.L.dlg_backend_set_partition(self.h, rank, nranks), "set_partition")

    def partition_rows(self):
        """the measurement rows this rank holds (ascending); x / J values are uploaded for these"""
        n = C.c_int()
        rows = C.POINTER(C.c_int)()
        _ck(self.L.dlg_partition_rows(self.h, C.byref(n), C.byref(rows)), "partition_rows")
        return np.ctypeslib.as_array(rows, shape=(n.value,)).copy() if n.value else np.zeros(0, dtype=np.int32)

    def partition_stats(self):
        st = (C.c_long * len(PART_STAT_NAMES))()
        _ck(self.L.dlg_partition_stats(self.h, st, len(PART_STAT_NAMES)), "partition_stats")
        return {k: st[i] for i, k in enumerate(PART_STAT_NAMES)}

    def init_rccl(self, rank, nranks, unique_id):
        """join an RCCL communicator: collectives run on the backend's stream, no host in between"""
        buf = C.create_string_buffer(unique_id, 128)
        _ck(self.L.dlg_backend_init_rccl(self.h, rank, nranks, C.cast(buf, C.c_void_p)), "init_rccl")

    def set_noop_comm(self, on=True):
        """measurement only: one rank of a partition with every sum over the ranks skipped"""
        _ck(self.L.dlg_backend_set_noop_comm(self.h, 1 if on else 0), "set_noop_comm")

    def comm_size(self):
        n = C.c_int()
        _ck(self.L.dlg_backend_comm_size(self.h, C.byref(n)), "comm_size")
        return n.value

    def set_pattern(self, Jp, Ji):
        Jp = np.ascontiguousarray(Jp, dtype=np.int32)
        Ji = np.ascontiguousarray(Ji, dtype=np.int32)
        _ck(self.L.dlg_sparse_set_pattern(self.h, iptr(Jp), iptr(Ji)), "set_pattern")

    def stats(self):
        a, b = C.c_long(), C.c_long()
        c, d = C.c_int(), C.c_int()
        e = C.c_double()
        _ck(self.L.dlg_sparse_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)),
            "stats")
        return dict(nnz_JtJ_lower=a.value, nnz_L=b.value, n_supernodes=c.value, n_levels=d.value,
                    factor_flops=e.value)

    def schedule(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _ck(self.L.dlg_sparse_schedule(self.h, C.byref(a), C.byref(b), C.byref(c)), "schedule")
        return dict(n_levels=a.value, persist_level0=b.value, persist_items=c.value)

    def leaf_rows_stats(self):
        """lean leaf launches, materialisations of the leaves' rows, whether the current factor's are raw, lean levels"""
        v = (C.c_long * 4)()
        _ck(self.L.dlg_sparse_leaf_rows_stats(self.h, v, 4), "leaf_rows_stats")
        return dict(lean_launches=v[0], materialized=v[1], raw=bool(v[2]), lean_levels=v[3])

    def set_p(self, slot, p):
        p = np.ascontiguousarray(p, dtype=np.float64)
        _ck(self.L.dlg_point_set_p(self.h, slot, dptr(p)), "set_p")

    def upload(self, slot, x, J):
        x = np.ascontiguousarray(x, dtype=np.float64)
        J = np.ascontiguousarray(J, dtype=np.float64)
        self._keep = [x, J]
        _ck(self.L.dlg_point_upload(self.h, slot, dptr(x), dptr(J)), "upload")

    def upload_products(self, slot, norm2x, Jtx, JtJ):
        Jtx = np.ascontiguousarray(Jtx, dtype=np.float64)
        JtJ = np.ascontiguousarray(JtJ, dtype=np.float64)
        self._keep = [Jtx, JtJ]
        _ck(self.L.dlg_point_upload_products(self.h, slot, norm2x, dptr(Jtx), dptr(JtJ)), "upload")

    def bind_device(self, slot, x_ptr, J_ptr):
        _ck(self.L.dlg_point_bind_device(self.h, slot, C.c_void_p(x_ptr), C.c_void_p(J_ptr)), "bind")

    def eval(self, slot):
        a, b = C.c_double(), C.c_double()
        _ck(self.L.dlg_point_eval(self.h, slot, C.byref(a), C.byref(b)), "eval")
        return a.value, b.value

    def cauchy(self, slot):
        a = C.c_double()
        _ck(self.L.dlg_cauchy(self.h, slot, C.byref(a)), "cauchy")
        return a.value

    def factorize(self, slot, lam=0.0):
        ok = C.c_int()
        _ck(self.L.dlg_factorize(self.h, slot, lam, C.byref(ok)), "factorize")
        return bool(ok.value)

    def solve_gn(self, slot):
        a = C.c_double()
        _ck(self.L.dlg_solve_gn(self.h, slot, C.byref(a)), "solve_gn")
        return a.value

    def gauss_newton(self, slot, lam=0.0):
        """factorise (raising lambda as the reference does) + solve: returns (lambda, |gn|^2)"""
        l, a = C.c_double(lam), C.c_double()
        _ck(self.L.dlg_gauss_newton(self.h, slot, C.byref(l), C.byref(a)), "gauss_newton")
        return l.value, a.value

    def cauchy_gauss_newton(self, slot, lam=0.0):
        """Cauchy step + gauss_newton behind one synchronisation: (lambda, |cauchy|^2, |gn|^2)"""
        l, c, a = C.c_double(lam), C.c_double(), C.c_double()
        _ck(self.L.dlg_cauchy_gauss_newton(self.h, slot, C.byref(l), C.byref(c), C.byref(a)), "cauchy_gauss_newton")
        return l.value, c.value, a.value

    def _pnew_buffer(self):
        if self._pnew is None:
            self._pnew_ptr = self.L.dlg_host_alloc(8 * self.N)
            if not self._pnew_ptr:
                raise DlgError(self.L.dlg_last_error().decode())
            self._pnew = np.ctypeslib.as_array(C.cast(self._pnew_ptr, C.POINTER(C.c_double)), shape=(self.N,))
        return self._pnew

    def _pnew_dest(self, want_p, p_out):
        """where p_new goes: p_out (a caller's float64 array of N, e.g. pageable memory), else this object's
        page-locked buffer, else (want_p false) nowhere"""
        if not want_p:
            return None
        if p_out is None:
            return self._pnew_buffer()
        assert p_out.dtype == np.float64 and p_out.shape == (self.N,) and p_out.flags["C_CONTIGUOUS"]
        return p_out

    def step(self, frm, to, kind, trustregion, want_p=True, tail=True, p_out=None):
        """make_step + expected_improvement behind one synchronisation:
        (|step|^2, k, max|step|, expected improvement, p_new); p_new as in make_step"""
        n2, k, am, ei = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        dst = self._pnew_dest(want_p, p_out)
        _ck(self.L.dlg_step(self.h, frm, to, kind, trustregion, C.byref(n2), C.byref(k), C.byref(am),
                            C.byref(ei), dptr(dst) if want_p else None), "step")
        e = ei.value
        if tail and self.step_tail_pending():
            e = self.step_tail()                # set_defer_tail: the value (and a page-locked p_new) complete here
        return n2.value, k.value, am.value, e, dst

    def take_step(self, frm, to, trustregion, lam=0.0, want_p=True, tail=True, p_out=None):
        """Cauchy + Gauss-Newton + the choice of step + step + expected improvement behind one
        synchronisation: (lambda, dict(n2c, n2g, kind, n2s, k, amax, ei), p_new)"""
        l = C.c_double(lam)
        out = (C.c_double * 7)()
        dst = self._pnew_dest(want_p, p_out)
        _ck(self.L.dlg_take_step(self.h, frm, to, trustregion, C.byref(l), out,
                                 dptr(dst) if want_p else None), "take_step")
        keys = ("n2c", "n2g", "kind", "n2s", "k", "amax", "ei")
        r = dict(zip(keys, [float(v) for v in out]))
        r["kind"] = int(r["kind"])
        if tail and self.step_tail_pending():
            r["ei"] = self.step_tail()          # set_defer_tail: the value (and a page-locked p_new) complete here
        return l.value, r, dst

    def run_steps(self, frm, to, nsteps, x_ptrs, J_ptrs, first_copy, trustregion, lam0=0.0):
        """nsteps x (bind the next resident copy, eval, take_step) in one C call (dlg_run_steps): returns
        (dict of the last step's scalars, kind of step)"""
        n = len(x_ptrs)
        xa = (C.c_void_p * n)(*x_ptrs)
        ja = (C.c_void_p * n)(*J_ptrs)
        out = (C.c_double * 9)()
        kind = C.c_int()
        _ck(self.L.dlg_run_steps(self.h, frm, to, nsteps, n, xa, ja, first_copy, trustregion, lam0, out, C.byref(kind)),
            "run_steps")
        keys = ("n2x", "n2c", "n2g", "k", "n2s", "ei", "gmax", "amax", "lam")
        return dict(zip(keys, [float(v) for v in out])), kind.value

    def solve_with_factor(self, slot, rhs):
        """(JtJ + lambda I) u = rhs with the factor held for `slot`; rhs: (N,) or (nrhs, N) rows"""
        r = np.ascontiguousarray(np.atleast_2d(rhs), dtype=np.float64)
        out = np.zeros_like(r)
        _ck(self.L.dlg_solve_with_factor(self.h, slot, dptr(r), dptr(out), r.shape[0]), "solve_with_factor")
        return out if np.ndim(rhs) == 2 else out[0]

    def solve_multi(self, slot, rhs):
        """blocked variant of solve_with_factor: rhs (nrhs, N) rows = right-hand sides; 16 per pass over the factor"""
        r = np.ascontiguousarray(np.atleast_2d(rhs), dtype=np.float64)
        out = np.zeros_like(r)
        _ck(self.L.dlg_solve_multi(self.h, slot, dptr(r), dptr(out), r.shape[0]), "solve_multi")
        return out

    def pseudoinverse_chunk(self, slot, row0, row1):
        """inv(JtJ + lambda I) Jt[:, row0:row1] as (row1 - row0, N): row i = the column of measurement row0 + i"""
        out = np.zeros((row1 - row0, self.N))
        _ck(self.L.dlg_pseudoinverse_chunk(self.h, slot, row0, row1, dptr(out)), "pseudoinverse_chunk")
        return out

    def feature_leverage(self, slot, feature_size, f0, nf):
        """leverage blocks A_f = J_f inv(JtJ + lambda I) J_f^T of features f0 .. f0 + nf - 1, packed upper:
        (nf,) for feature size 1, (nf, 3) = {a00, a01, a11} for size 2"""
        nt = 3 if feature_size == 2 else 1
        out = np.zeros(nf * nt)
        _ck(self.L.dlg_feature_leverage(self.h, slot, feature_size, f0, nf, dptr(out)), "feature_leverage")
        return out if nt == 1 else out.reshape(nf, 3)

    def outlierness_factors(self, slot, feature_size, nf, scale):
        out = np.zeros(nf)
        _ck(self.L.dlg_outlierness_factors(self.h, slot, feature_size, nf, scale, dptr(out)), "outlierness_factors")
        return out

    def leverage_query(self, slot, Jq, istate):
        """Jq (featureSize, nstate) on the states istate ..: Jq inv(JtJ + lambda I) Jq^T, packed upper"""
        Jq = np.ascontiguousarray(np.atleast_2d(Jq), dtype=np.float64)
        fs, ns = Jq.shape
        out = np.zeros(fs * (fs + 1) // 2)
        _ck(self.L.dlg_leverage_query(self.h, slot, dptr(Jq), istate, ns, fs, dptr(out)), "leverage_query")
        return out

    def leverage_stats(self, feature_size):
        """(chunks, supernode visits of all chunks, supernodes) of the last sparse leverage plan"""
        a, b, c = C.c_long(), C.c_long(), C.c_int()
        _ck(self.L.dlg_leverage_stats(self.h, feature_size, C.byref(a), C.byref(b), C.byref(c)), "leverage_stats")
        return a.value, b.value, c.value

    def covariance_blocks(self, slot, r0, nr, c0, nc):
        """blocks Sigma[r0:r0+nr, c0:c0+nc] of inv(JtJ + lambda I) (the held factor, unscaled), one array (nr[q], nc[q])
        per request"""
        r0, nr, c0, nc = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.int32) for a in (r0, nr, c0, nc))
        n = len(r0)
        out = np.zeros(max(int(np.sum(nr.astype(np.int64) * nc)), 1))
        _ck(self.L.dlg_covariance_blocks(self.h, slot, n, iptr(r0), iptr(nr), iptr(c0), iptr(nc), dptr(out)),
            "covariance_blocks")
        blocks, o = [], 0
        for q in range(n):
            k = int(nr[q]) * int(nc[q])
            blocks.append(out[o:o + k].reshape(int(nr[q]), int(nc[q])))
            o += k
        return blocks

    def marginal_variances(self, slot):
        """diag(inv(JtJ + lambda I)) with the held factor, unscaled"""
        out = np.zeros(self.N)
        _ck(self.L.dlg_marginal_variances(self.h, slot, dptr(out)), "marginal_variances")
        return out

    def covariance_stats(self):
        """(chunks, supernode visits of all chunks, supernodes) of the last covariance plan run"""
        a, b, c = C.c_long(), C.c_long(), C.c_int()
        _ck(self.L.dlg_covariance_stats(self.h, C.byref(a), C.byref(b), C.byref(c)), "covariance_stats")
        return a.value, b.value, c.value

    def covariance_plan_seconds(self):
        return self.L.dlg_covariance_plan_seconds(self.h)

    def covariance_entries(self, slot, row, col):
        """Sigma[row[e], col[e]] of inv(JtJ + lambda I) (the held factor, unscaled) at entries of the structure of the
        factor, one value per entry"""
        row, col = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.int32) for a in (row, col))
        assert len(row) == len(col)
        out = np.zeros(max(len(row), 1))
        _ck(self.L.dlg_covariance_entries(self.h, slot, len(row), iptr(row), iptr(col), dptr(out)), "covariance_entries")
        return out[:len(row)]

    def query_covariance(self, slot, qrow, rowptr, var, val, nobs=-1):
        """Jq Sigma Jq^T (nobs < 0) or Jq Sigma J[0:nobs]^T J[0:nobs] Sigma Jq^T per query of the CSR batch (query k: rows
        qrow[k] .. qrow[k+1] - 1), with the held factor, unscaled: one (fs, fs) array per query"""
        qrow, rowptr, var = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.int32) for a in (qrow, rowptr, var))
        val = np.ascontiguousarray(np.atleast_1d(val), dtype=np.float64)
        nq = len(qrow) - 1
        fs = np.diff(qrow.astype(np.int64))
        out = np.zeros(max(int(np.sum(fs * fs)), 1))
        _ck(self.L.dlg_query_covariance(self.h, slot, nq, iptr(qrow), iptr(rowptr), iptr(var), dptr(val), nobs, dptr(out)),
            "query_covariance")
        blocks, o = [], 0
        for k in range(nq):
            n = int(fs[k])
            blocks.append(out[o:o + n * n].reshape(n, n))
            o += n * n
        return blocks

    def query_covariance_stats(self):
        """(chunks, supernode visits of all chunks, supernodes) of the last query covariance plan run"""
        a, b, c = C.c_long(), C.c_long(), C.c_int()
        _ck(self.L.dlg_query_covariance_stats(self.h, C.byref(a), C.byref(b), C.byref(c)), "query_covariance_stats")
        return a.value, b.value, c.value

    def query_covariance_plan_seconds(self):
        return self.L.dlg_query_covariance_plan_seconds(self.h)

    def covariance_entries_stats(self):
        """(plan seconds of the last call, values held for Sigma, doubles of the front scratch)"""
        t, a, f = C.c_double(), C.c_long(), C.c_long()
        _ck(self.L.dlg_covariance_entries_stats(self.h, C.byref(t), C.byref(a), C.byref(f)), "covariance_entries_stats")
        return t.value, a.value, f.value

    def make_step(self, frm, to, kind, trustregion, want_p=True, p_out=None):
        """p_new comes back in a page-locked buffer owned by this object (as the driver's operating
        points are): it is overwritten by the next call -- copy it to keep it.  p_out: a caller's array instead."""
        n2, k, am = C.c_double(), C.c_double(), C.c_double()
        dst = self._pnew_dest(want_p, p_out)
        _ck(self.L.dlg_make_step(self.h, frm, to, kind, trustregion, C.byref(n2), C.byref(k),
                                 C.byref(am), dptr(dst) if want_p else None), "make_step")
        return n2.value, k.value, am.value, dst

    def expected_improvement(self, frm, to):
        a = C.c_double()
        _ck(self.L.dlg_expected_improvement(self.h, frm, to, C.byref(a)), "expected_improvement")
        return a.value

    def download(self, slot, which, n=None):
        if n is None:
            n = self.M if which == VEC_X else self.N
        out = np.zeros(n)
        _ck(self.L.dlg_point_download(self.h, slot, which, dptr(out), n), "download")
        return out

    def factor_dense(self, n):
        out = np.zeros(n)
        _ck(self.L.dlg_factor_download_dense(self.h, dptr(out), n), "factor download")
        return out


def numeric_step(scheme, p, lo, hi, delta_rel, delta_abs):
    """dogleg_amd_numeric_step: (plus point, minus point, divisor) of one variable"""
    tp, tm, d = C.c_double(), C.c_double(), C.c_double()
    lib().dogleg_amd_numeric_step(scheme, p, lo, hi, delta_rel, delta_abs, C.byref(tp), C.byref(tm), C.byref(d))
    return tp.value, tm.value, d.value


def numeric_options(scheme=NUMERIC_FORWARD, delta_rel=0.0, delta_abs=0.0, lower=None, upper=None, bounds_on_device=False):
    """(a NumericOptions, what it points at): lower / upper numpy arrays (B, N), or with bounds_on_device DeviceArrays / raw
    device addresses, or None"""
    keep = []

    def addr(a):
        if a is None:
            return None
        if bounds_on_device:
            return a.ptr if isinstance(a, DeviceArray) else int(a)
        a = np.ascontiguousarray(a, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data

    return NumericOptions(scheme, delta_rel, delta_abs, addr(lower), addr(upper), 1 if bounds_on_device else 0), keep


class BatchNumeric:
    """dogleg_amd_batch_numeric_create: the numeric-Jacobian adapter over a values-only batch callback (values_cb: the address
    of a dogleg_callback_device_batch_values_t).  .cb / .cookie go to any J-form batch entry point.  Creation that the library
    refuses raises DlgError with its message."""

    def __init__(self, B, N, M, values_cb, values_cookie, scheme=None, delta_rel=0.0, delta_abs=0.0, lower=None, upper=None,
                 bounds_on_device=False):
        L = lib()
        self.B, self.N, self.M = B, N, M
        opt = None
        if scheme is not None:
            opt, self._keep = numeric_options(scheme, delta_rel, delta_abs, lower, upper, bounds_on_device)
        self.scheme = NUMERIC_FORWARD if scheme is None else scheme
        self.K = (2 * N + 1) if self.scheme == NUMERIC_CENTRAL else N + 1
        self.h = L.dogleg_amd_batch_numeric_create(B, N, M, values_cb, values_cookie, C.byref(opt) if opt is not None else None)
        if not self.h:
            raise DlgError((L.dlg_last_error() or b"").decode())
        self.cb = C.cast(L.dogleg_amd_batch_numeric_callback, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def invoke(self, p_dev, x_dev, J_dev, live_dev, B=None, stream=None):
        """the adapter itself, as a batch entry point would call it (asynchronous: dlg_device_sync or a download follows)"""
        lib().dogleg_amd_batch_numeric_callback(_dev(p_dev), _dev(x_dev), _dev(J_dev), _dev(live_dev), self.B if B is None else B,
                                                _dev(stream), self.h)

    def stats(self):
        """{invocations, f_calls, copies, launches, ms_f, ms_library} since the handle was made"""
        out = (C.c_double * 6)()
        lib().dogleg_amd_batch_numeric_stats(self.h, out, 6)
        return dict(zip(("invocations", "f_calls", "copies", "launches", "ms_f", "ms_library"), (float(v) for v in out)))

    def buffers(self, B=None):
        """(p_copies (K, B, N), x_copies (K, B, M), divisor (B, N)) downloaded, as the last invocation (of B problems) left them"""
        B = self.B if B is None else B
        a, b, d = C.c_void_p(), C.c_void_p(), C.c_void_p()
        K = lib().dogleg_amd_batch_numeric_buffers(self.h, C.byref(a), C.byref(b), C.byref(d))
        assert K == self.K
        out = []
        for ptr, shape in ((a, (K, B, self.N)), (b, (K, B, self.M)), (d, (B, self.N))):
            arr = np.zeros(shape)
            _ck(lib().dlg_mem_download(arr.ctypes.data, ptr, arr.nbytes), "download")
            out.append(arr)
        return tuple(out)

    def close(self):
        if self.h:
            lib().dogleg_amd_batch_numeric_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def numeric_plan(N, M, nnz, Jp, Ji, scheme=NUMERIC_FORWARD):
    """dogleg_amd_numeric_plan (host only): (C or -1, colour[N], K, device bytes).  nnz == 0: dense (Jp, Ji ignored)"""
    if nnz > 0:
        Jp = np.ascontiguousarray(Jp, dtype=np.int32)
        Ji = np.ascontiguousarray(Ji, dtype=np.int32)
    colour = np.full(max(N, 1), -1, dtype=np.int32)
    K, nbytes = C.c_int(-1), C.c_double(-1.0)
    ncol = lib().dogleg_amd_numeric_plan(N, M, nnz, iptr(Jp) if nnz > 0 else None, iptr(Ji) if nnz > 0 else None, scheme,
                                         iptr(colour), C.byref(K), C.byref(nbytes))
    return ncol, colour[:N], K.value, nbytes.value


class DeviceNumeric:
    """dogleg_amd_numeric_create: the numeric-Jacobian adapter over a values-only single-problem callback (values_cb: the
    address of a dogleg_callback_device_values_t) on the pattern (Jp, Ji) of Jt; nnz == 0: dense.  .cb / .cookie go to
    optimize_device and its kin.  lower / upper: (N,) arrays.  Creation that the library refuses raises DlgError with its
    message."""

    def __init__(self, N, M, nnz, Jp, Ji, values_cb, values_cookie, scheme=None, delta_rel=0.0, delta_abs=0.0, lower=None,
                 upper=None, bounds_on_device=False):
        L = lib()
        self.N, self.M, self.nnz = N, M, nnz
        opt = None
        if scheme is not None:
            opt, self._keep = numeric_options(scheme, delta_rel, delta_abs, lower, upper, bounds_on_device)
        self.scheme = NUMERIC_FORWARD if scheme is None else scheme
        if nnz > 0:
            Jp = np.ascontiguousarray(Jp, dtype=np.int32)
            Ji = np.ascontiguousarray(Ji, dtype=np.int32)
        self.h = L.dogleg_amd_numeric_create(N, M, nnz, iptr(Jp) if nnz > 0 else None, iptr(Ji) if nnz > 0 else None, values_cb,
                                             values_cookie, C.byref(opt) if opt is not None else None)
        if not self.h:
            raise DlgError((L.dlg_last_error() or b"").decode())
        self.K = L.dogleg_amd_numeric_buffers(self.h, None, None, None)
        self.C = (self.K - 1) // (2 if self.scheme == NUMERIC_CENTRAL else 1)
        self.cb = C.cast(L.dogleg_amd_numeric_callback, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def invoke(self, p_dev, x_dev, J_dev, stream=None):
        """the adapter itself, as a solver would call it (asynchronous: dlg_device_sync or a download follows)"""
        lib().dogleg_amd_numeric_callback(_dev(p_dev), _dev(x_dev), _dev(J_dev), _dev(stream), self.h)

    def stats(self):
        """{invocations, f_calls, copies, launches, ms_f, ms_library} since the handle was made"""
        out = (C.c_double * 6)()
        lib().dogleg_amd_numeric_stats(self.h, out, 6)
        return dict(zip(("invocations", "f_calls", "copies", "launches", "ms_f", "ms_library"), (float(v) for v in out)))

    def buffers(self):
        """(p_copies (K, N), x_copies (K, M), divisor (N,)) downloaded, as the last invocation left them"""
        a, b, d = C.c_void_p(), C.c_void_p(), C.c_void_p()
        K = lib().dogleg_amd_numeric_buffers(self.h, C.byref(a), C.byref(b), C.byref(d))
        out = []
        for ptr, shape in ((a, (K, self.N)), (b, (K, self.M)), (d, (self.N,))):
            arr = np.zeros(shape)
            _ck(lib().dlg_mem_download(arr.ctypes.data, ptr, arr.nbytes), "download")
            out.append(arr)
        return tuple(out)

    def close(self):
        if self.h:
            lib().dogleg_amd_numeric_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def last_solve_timing():
    """{phase: (ms, calls)} of the calling thread's last dogleg_optimize* solve (DOGLEG_AMD_TIMING=1 must have been set)"""
    ms, n = (C.c_double * 7)(), (C.c_int * 7)()
    lib().dogleg_amd_last_solve_timing(ms, n)
    keys = ("pattern", "callback", "inputs", "point_eval", "take_step", "trace", "run_optimizer")
    return {k: (ms[i], n[i]) for i, k in enumerate(keys)}
