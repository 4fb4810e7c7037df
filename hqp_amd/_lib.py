"""ctypes binding of the C-ABI library ``libhqpkkt.so`` (include/hqpkkt.h).

There is no CPU fallback: if the HIP extension is missing this module raises,
and every numeric entry point returns ``HQPKKT_E_DEVICE`` without a gfx950 GPU.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HQPKKT_LIB") or os.path.join(_HERE, "libhqpkkt.so")  # override: instrumented builds

OK, E_SIZES, E_MEM, E_SING, E_FORMAT, E_NULL, E_RANGE, E_INTERN, E_DEVICE = 0, 1, 3, 4, 6, 8, 10, 17, 100
MODE_FULL, MODE_REDUCED, MODE_STAGED = 0, 1, 2
LOC_HOST, LOC_DEVICE = 0, 1
DYN_DENSE, DYN_SPARSE, DYN_PROFILE = 0, 1, 3
HESS_CSR, HESS_DENSE = 0, 1
HQPKKT_HESS_UPDATE_RANK = 4
HQPKKT_BFGS_REPORT = 8
HQPKKT_DSCALE_REPORT = 8
HQPKKT_QBFGS_FULL, HQPKKT_QBFGS_PATTERN = 0, 1
HQPKKT_QBFGS_REPORT = 8
HQPKKT_EIG_MAX_STEPS = 128
HQPKKT_EIG_REPORT = 10
HQPKKT_EIG_END_REL = 2.0 ** -40

# every symbol include/hqpkkt.h declares
SYMBOLS = [
    "hqpkkt_default_opts", "hqpkkt_create", "hqpkkt_destroy", "hqpkkt_analyze",
    "hqpkkt_set_values", "hqpkkt_factor", "hqpkkt_step", "hqpkkt_residual", "hqpkkt_solve",
    "hqpkkt_get_sbw", "hqpkkt_get_perm", "hqpkkt_set_tol", "hqpkkt_set_eps",
    "hqpkkt_set_stream", "hqpkkt_get_stats", "hqpkkt_strerror", "hqpkkt_debug_get",
    "hqpkkt_selftest_mfma", "hqpkkt_set_profile", "hqpkkt_get_profile",
    "hqpkkt_profile_class_name", "hqpkkt_set_shard", "hqpkkt_debug_read",
    "hqpkkt_default_ip_opts", "hqpkkt_mehrotra", "hqpkkt_franke",
    "hqpkkt_set_stages", "hqpkkt_debug_stage_ranks", "hqpkkt_debug_stage_block", "hqpkkt_debug_dgemm", "hqpkkt_debug_dgemm2", "hqpkkt_debug_dgemm_full", "hqpkkt_debug_sk_table", "hqpkkt_debug_gemm_form",
    "hqpkkt_analyze_staged", "hqpkkt_set_values_staged", "hqpkkt_set_shard_stream",
    "hqpkkt_values_staging", "hqpkkt_detect_stages", "hqpkkt_stage_staging", "hqpkkt_set_stage_block",
    "hqpkkt_debug_factor_block", "hqpkkt_debug_solve_top_stamps", "hqpkkt_set_dynamics_form", "hqpkkt_set_dense_columns",
    "hqpkkt_debug_sk_profile", "hqpkkt_debug_gemv_profile",
    "hqpkkt_set_packed_panels", "hqpkkt_debug_dgemm_packed", "hqpkkt_debug_gemv_packed", "hqpkkt_debug_carried_packed",
    "hqpkkt_set_dense_rows", "hqpkkt_debug_dgemm_ctrl_rows", "hqpkkt_debug_sk_ctrl_rows",
    "hqpkkt_set_hessian_form", "hqpkkt_set_stage_hessian", "hqpkkt_debug_stage_hessian", "hqpkkt_debug_hess_symv",
    "hqpkkt_set_packed_hessians", "hqpkkt_debug_hess_symv_timed",
    "hqpkkt_update_stage_hessians", "hqpkkt_hessian_product",
    "hqpkkt_bfgs_update_stage_hessians", "hqpkkt_bfgs_report",
    "hqpkkt_hessian_row_stats", "hqpkkt_restart_stage_hessians", "hqpkkt_gerschgorin_stage_hessians",
    "hqpkkt_eigen_control_stage_hessians", "hqpkkt_eigen_report",
    "hqpkkt_debug_gemm_schedule",
    "hqpkkt_debug_gemv_dense", "hqpkkt_debug_symv", "hqpkkt_debug_symv_batch", "hqpkkt_debug_symv_map",
    "hqpkkt_debug_rows_gemv",
    "hqpkkt_q_values", "hqpkkt_q_product", "hqpkkt_q_row_stats", "hqpkkt_q_set_diagonal", "hqpkkt_q_gerschgorin",
    "hqpkkt_q_dscale_setup", "hqpkkt_q_dscale_update", "hqpkkt_q_dscale_report", "hqpkkt_lagrangian_gradient",
    "hqpkkt_q_blocks", "hqpkkt_q_bfgs_update", "hqpkkt_q_bfgs_report",
    "hqpkkt_q_eigen_control", "hqpkkt_q_eigen_report",
    "hqpkkt_lagrangian_gradient_staged",
]
RCCL_LIB_PATH = os.path.join(_HERE, "libhqpkkt_rccl.so")
RCCL_SYMBOLS = ["hqpkkt_rccl_unique_id", "hqpkkt_rccl_create", "hqpkkt_rccl_create_from_env",
                "hqpkkt_rccl_comm_info", "hqpkkt_rccl_exchange", "hqpkkt_rccl_destroy", "hqpkkt_rccl_origin"]

XCHG_ALLGATHER, XCHG_ALLREDUCE_SUM, XCHG_BCAST_BASE = 0, 1, 16
# int fn(void *ctx, int op, double *buf, long long slot_elems, int nslots)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_int)


class Opts(C.Structure):
    _fields_ = [("mode", C.c_int), ("device", C.c_int), ("loc", C.c_int), ("tol", C.c_double),
                ("eps", C.c_double), ("pivot_eps", C.c_double), ("leaf_size", C.c_int),
                ("max_pivots", C.c_int), ("zd_policy", C.c_int), ("slack_policy", C.c_int),
                ("no_small_fronts", C.c_int), ("upd_pingpong_mb", C.c_int), ("amalgamation", C.c_int),
                ("ordering", C.c_int)]


class HessUpdate(C.Structure):  # hqpkkt_hess_update
    _fields_ = [("r", C.c_int), ("U", C.POINTER(C.c_void_p)), ("coef", C.c_void_p), ("beta", C.c_void_p), ("diag", C.c_void_p)]


class BfgsUpdate(C.Structure):  # hqpkkt_bfgs_update
    _fields_ = [("s", C.c_void_p), ("y", C.c_void_p), ("gamma", C.c_double), ("alpha", C.c_double), ("v", C.c_void_p)]


class DScaleUpdate(C.Structure):  # hqpkkt_dscale_update
    _fields_ = [("s", C.c_void_p), ("y", C.c_void_p), ("gamma", C.c_double), ("bsize", C.c_int), ("v", C.c_void_p)]


class QBfgsUpdate(C.Structure):  # hqpkkt_q_bfgs_update_args
    _fields_ = [("s", C.c_void_p), ("y", C.c_void_p), ("gamma", C.c_double), ("alpha", C.c_double), ("bsize", C.c_int), ("fill", C.c_int),
                ("v", C.c_void_p), ("Qs", C.c_void_p)]


class EigenControl(C.Structure):  # hqpkkt_eigen_control
    _fields_ = [("eps", C.c_double), ("floor_from_bfgs", C.c_int), ("floor", C.c_void_p), ("max_steps", C.c_int)]


class QEigenControl(C.Structure):  # hqpkkt_q_eigen_control_args
    _fields_ = [("eps", C.c_double), ("bsize", C.c_int), ("floor_from_bfgs", C.c_int), ("floor", C.c_void_p), ("max_steps", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("dim", C.c_int), ("sbw", C.c_int), ("n_supernodes", C.c_int),
                ("n_levels", C.c_int), ("max_front", C.c_int), ("nnz_kkt", C.c_longlong),
                ("nnz_factor", C.c_longlong), ("flops_factor", C.c_longlong),
                ("bytes_panels", C.c_longlong), ("bytes_updates", C.c_longlong),
                ("n_2x2", C.c_int), ("n_perturbed", C.c_int), ("refine_rounds", C.c_int),
                ("kmax", C.c_double), ("ms_assemble", C.c_float), ("ms_factor", C.c_float),
                ("ms_step", C.c_float), ("ms_residual", C.c_float), ("ms_solve", C.c_float),
                ("shard_rank", C.c_int), ("shard_count", C.c_int), ("n_top", C.c_int),
                ("n_exchange_blocks", C.c_int), ("flops_local", C.c_longlong),
                ("flops_top", C.c_longlong), ("bytes_exchange_factor", C.c_longlong),
                ("bytes_exchange_step", C.c_longlong), ("n_slow_pivots", C.c_int),
                ("n_poll_fallbacks", C.c_int)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class IpOpts(C.Structure):
    _fields_ = [("eps", C.c_double), ("max_iters", C.c_int), ("gammaf", C.c_double),
                ("norm_data", C.c_double), ("hot_start", C.c_int), ("max_warm_iters", C.c_int),
                ("init_method", C.c_int), ("reserved", C.c_int * 1),
                ("norm_Q", C.c_double), ("norm_C", C.c_double), ("norm_d", C.c_double), ("qp_mu0", C.c_double)]


class DgemmOperand(C.Structure):
    _fields_ = [("p", C.c_void_p), ("rows", C.c_longlong), ("ld", C.c_longlong), ("col0", C.c_longlong)]


class DgemmCase(C.Structure):
    """hqpkkt_dgemm_case (include/hqpkkt.h)"""
    _fields_ = [("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("K2", C.c_int),
                ("lower", C.c_int), ("mirror", C.c_int), ("flags", C.c_int), ("cin_is_c", C.c_int),
                ("alpha", C.c_double), ("beta", C.c_double),
                ("A", DgemmOperand), ("B", DgemmOperand), ("A2", DgemmOperand), ("B2", DgemmOperand), ("Cin", DgemmOperand),
                ("C", C.c_void_p), ("c_rows", C.c_longlong), ("ldc", C.c_longlong), ("c_row0", C.c_longlong), ("c_col0", C.c_longlong),
                ("form", C.c_int), ("tile_map", C.c_int), ("ldsdma", C.c_int), ("nsplit", C.c_int), ("tiles", C.c_longlong),
                ("krange", C.c_void_p), ("krange_by", C.c_int)]


class CtrlRowsCase(C.Structure):
    """hqpkkt_ctrl_rows_case (include/hqpkkt.h)"""
    _fields_ = [("M", C.c_int), ("N", C.c_int), ("mu", C.c_int), ("grid", C.c_int), ("A", DgemmOperand), ("B", DgemmOperand),
                ("C", C.c_void_p), ("c_rows", C.c_longlong), ("ldc", C.c_longlong),
                ("Cu", C.c_void_p), ("cu_rows", C.c_longlong), ("ldcu", C.c_longlong),
                ("taken", C.c_int), ("fallbacks", C.c_int), ("form", C.c_int), ("tiles", C.c_longlong)]


class GemvCase(C.Structure):
    """hqpkkt_gemv_case (include/hqpkkt.h)"""
    _fields_ = [("M", C.c_int), ("N", C.c_int), ("A", DgemmOperand), ("A2", DgemmOperand), ("n2", C.c_int), ("part_chunks", C.c_int),
                ("x", C.c_void_p), ("x_len", C.c_longlong), ("x2", C.c_void_p), ("x2_len", C.c_longlong), ("add", C.c_void_p), ("add2", C.c_void_p),
                ("scale", C.c_double), ("y", C.c_void_p), ("y2", C.c_void_p), ("xoff", C.c_longlong), ("yoff", C.c_longlong),
                ("chunks", C.c_int), ("vec16", C.c_int)]


class RowsCase(C.Structure):
    """hqpkkt_rows_case (include/hqpkkt.h)"""
    _fields_ = [("nblocks", C.c_int)] + [(k, C.c_void_p) for k in ("rows", "cols", "ld", "col0", "off", "E")] + [("e_len", C.c_longlong), ("row_index", C.c_void_p),
                ("n", C.c_int), ("m", C.c_int)] + [(k, C.c_void_p) for k in ("x", "t", "tz", "zw", "r3", "y", "dz", "dw", "xc")]


class GemmCaps(C.Structure):
    """hqpkkt_gemm_caps (include/hqpkkt.h)"""
    _fields_ = [(k, C.c_int) for k in ("variant", "cus", "grid", "unequal", "flags")] + \
               [(k, C.c_longlong) for k in ("sk_tiles", "cnt_elems", "ws_elems", "ws2_elems")]


class GemmLaunch(C.Structure):
    """hqpkkt_gemm_launch (include/hqpkkt.h)"""
    _fields_ = [(k, C.c_int) for k in ("M", "N", "K", "K2", "lower", "mirror", "second_stream", "ntiles")] + \
               [(k, C.c_ulonglong) for k in ("a", "b", "a2", "b2", "c")] + \
               [(k, C.c_longlong) for k in ("lda", "ldb", "lda2", "ldb2", "ldc", "c0")] + \
               [("mu", C.c_int), ("by", C.c_int), ("panel", C.c_void_p)]


class GemmScheduleOut(C.Structure):
    """hqpkkt_gemm_schedule_out (include/hqpkkt.h)"""
    _fields_ = [(k, C.c_int) for k in ("form", "nsplit", "variant", "list", "stride", "seg", "same_key")] + \
               [(k, C.c_longlong) for k in ("tiles", "nslab", "pieces", "order_len")]


class IpResult(C.Structure):
    _fields_ = [("result", C.c_int), ("iters", C.c_int), ("n_factor", C.c_int), ("n_solve", C.c_int),
                ("gap", C.c_double), ("mu", C.c_double), ("phi", C.c_double), ("pcost", C.c_double),
                ("alpha", C.c_double), ("ms_total", C.c_float), ("attempts", C.c_int)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def lib():
    """Load the HIP extension; fail loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  hqp_amd has no CPU fallback.")
    try:
        # PyTorch is the plumbing for device memory / streams / torch.distributed.  Its
        # wheel bundles its own HIP runtime; load it FIRST so that the extension binds to
        # the same libamdhip64 (two runtimes in one process lose the GPU).
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.c_void_p  # vectors go as raw addresses
    L.hqpkkt_default_opts.argtypes = [C.POINTER(Opts)]
    L.hqpkkt_create.argtypes = [C.POINTER(Opts), C.POINTER(vp)]
    L.hqpkkt_destroy.argtypes = [vp]
    L.hqpkkt_analyze.argtypes = [vp, C.c_int, C.c_int, C.c_int] + [vp] * 6 + [ip]
    L.hqpkkt_set_values.argtypes = [vp, dp, dp, dp]
    L.hqpkkt_factor.argtypes = [vp, dp, dp]
    L.hqpkkt_step.argtypes = [vp] + [dp] * 10
    L.hqpkkt_residual.argtypes = [vp] + [dp] * 10 + [C.POINTER(C.c_double)]
    L.hqpkkt_solve.argtypes = [vp] + [dp] * 10 + [C.POINTER(C.c_double)]
    L.hqpkkt_get_sbw.argtypes = [vp, ip]
    L.hqpkkt_get_perm.argtypes = [vp, vp]
    L.hqpkkt_set_tol.argtypes = [vp, C.c_double]
    L.hqpkkt_set_eps.argtypes = [vp, C.c_double]
    L.hqpkkt_set_stream.argtypes = [vp, vp]
    L.hqpkkt_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.hqpkkt_strerror.restype = C.c_char_p
    L.hqpkkt_strerror.argtypes = [C.c_int]
    L.hqpkkt_debug_get.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_longlong)]
    L.hqpkkt_selftest_mfma.argtypes = [C.c_int, C.POINTER(C.c_double)]
    L.hqpkkt_set_profile.argtypes = [vp, C.c_int]
    L.hqpkkt_get_profile.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    L.hqpkkt_profile_class_name.restype = C.c_char_p
    L.hqpkkt_profile_class_name.argtypes = [C.c_int]
    L.hqpkkt_set_shard.argtypes = [vp, C.c_int, C.c_int, EXCHANGE_FN, vp]
    L.hqpkkt_debug_read.argtypes = [vp, C.c_int, C.c_int, vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.hqpkkt_default_ip_opts.argtypes = [C.POINTER(IpOpts)]
    L.hqpkkt_mehrotra.argtypes = [vp, C.POINTER(IpOpts)] + [dp] * 7 + [C.POINTER(IpResult)]
    L.hqpkkt_franke.argtypes = [vp, C.POINTER(IpOpts)] + [dp] * 7 + [C.POINTER(IpResult)]
    L.hqpkkt_set_stages.argtypes = [vp, C.c_int, vp, vp]
    L.hqpkkt_set_dynamics_form.argtypes = [vp, C.c_int]
    L.hqpkkt_set_dense_columns.argtypes = [vp, C.c_int]
    L.hqpkkt_set_packed_panels.argtypes = [vp, C.c_int]
    L.hqpkkt_set_dense_rows.argtypes = [vp, C.c_int]
    L.hqpkkt_set_hessian_form.argtypes = [vp, C.c_int]
    L.hqpkkt_set_stage_hessian.argtypes = [vp, C.c_int, vp, C.c_longlong]
    L.hqpkkt_debug_stage_hessian.argtypes = [vp, C.c_int, vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.hqpkkt_debug_hess_symv.argtypes = [vp, vp, vp]
    L.hqpkkt_set_packed_hessians.argtypes = [vp, C.c_int]
    L.hqpkkt_debug_hess_symv_timed.argtypes = [vp, vp, vp, C.c_int, C.POINTER(C.c_double)]
    L.hqpkkt_update_stage_hessians.argtypes = [vp, C.POINTER(HessUpdate)]
    L.hqpkkt_hessian_product.argtypes = [vp, vp, vp]
    L.hqpkkt_bfgs_update_stage_hessians.argtypes = [vp, C.POINTER(BfgsUpdate)]
    L.hqpkkt_bfgs_report.argtypes = [vp, vp]
    L.hqpkkt_hessian_row_stats.argtypes = [vp, vp, vp]
    L.hqpkkt_restart_stage_hessians.argtypes = [vp, C.c_double, vp]
    L.hqpkkt_gerschgorin_stage_hessians.argtypes = [vp, C.c_double]
    L.hqpkkt_eigen_control_stage_hessians.argtypes = [vp, C.POINTER(EigenControl)]
    L.hqpkkt_eigen_report.argtypes = [vp, vp, vp]
    L.hqpkkt_q_values.argtypes = [vp, vp]
    L.hqpkkt_q_product.argtypes = [vp, vp, vp]
    L.hqpkkt_q_row_stats.argtypes = [vp, vp, vp]
    L.hqpkkt_q_set_diagonal.argtypes = [vp, vp]
    L.hqpkkt_q_gerschgorin.argtypes = [vp, C.c_double]
    L.hqpkkt_q_dscale_setup.argtypes = [vp, C.c_double]
    L.hqpkkt_q_dscale_update.argtypes = [vp, C.POINTER(DScaleUpdate)]
    L.hqpkkt_q_dscale_report.argtypes = [vp, vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.hqpkkt_lagrangian_gradient.argtypes = [vp] * 6
    L.hqpkkt_lagrangian_gradient_staged.argtypes = [vp] * 6
    L.hqpkkt_q_blocks.argtypes = [vp, C.c_int, vp, vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.hqpkkt_q_bfgs_update.argtypes = [vp, C.POINTER(QBfgsUpdate)]
    L.hqpkkt_q_bfgs_report.argtypes = [vp, vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.hqpkkt_q_eigen_control.argtypes = [vp, C.POINTER(QEigenControl)]
    L.hqpkkt_q_eigen_report.argtypes = [vp, vp, vp, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    L.hqpkkt_debug_stage_ranks.argtypes = [vp, vp, C.c_int]
    L.hqpkkt_analyze_staged.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int] + [vp] * 6
    L.hqpkkt_set_values_staged.argtypes = [vp, dp, vp, vp, dp, dp]
    L.hqpkkt_values_staging.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.hqpkkt_set_shard_stream.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    L.hqpkkt_debug_dgemm.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_double)] * 2
    L.hqpkkt_debug_stage_block.argtypes = [vp, C.c_int, vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.hqpkkt_debug_dgemm2.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_double)] * 2 + [C.POINTER(C.c_longlong)]
    L.hqpkkt_debug_dgemm_full.argtypes = [C.c_int, C.POINTER(DgemmCase)]
    L.hqpkkt_debug_sk_table.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_longlong, C.POINTER(C.c_longlong),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.hqpkkt_debug_dgemm_ctrl_rows.argtypes = [C.c_int, C.POINTER(CtrlRowsCase)]
    L.hqpkkt_debug_sk_ctrl_rows.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int), C.c_longlong, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    L.hqpkkt_debug_sk_profile.argtypes = [C.POINTER(C.c_int), C.c_longlong, C.c_int, C.POINTER(C.c_int), C.c_longlong, C.POINTER(C.c_longlong)]
    L.hqpkkt_debug_gemv_profile.argtypes = [C.c_int] * 4 + [vp, C.c_longlong, C.c_longlong, vp, vp, vp, C.c_double, vp]
    L.hqpkkt_debug_dgemm_packed.argtypes = [C.c_int, C.POINTER(DgemmCase), vp, C.c_longlong, vp]
    L.hqpkkt_debug_gemv_packed.argtypes = [C.c_int] * 4 + [vp, C.c_longlong, vp, vp, vp, vp, C.c_double, vp]
    L.hqpkkt_debug_carried_packed.argtypes = [C.c_int] * 4 + [vp, C.c_longlong, C.c_longlong, vp, C.c_longlong, vp, vp, vp] + [C.c_longlong] * 4
    L.hqpkkt_debug_gemm_form.argtypes = [C.c_int] * 7 + [C.c_longlong] * 3 + [C.c_int, C.POINTER(C.c_longlong)] + [C.POINTER(C.c_int)] * 3
    L.hqpkkt_debug_gemm_schedule.argtypes = [C.POINTER(GemmCaps), C.POINTER(GemmLaunch), C.POINTER(GemmLaunch), C.POINTER(GemmScheduleOut),
                                             C.POINTER(C.c_int), C.c_longlong, C.POINTER(C.c_int), C.c_longlong]
    L.hqpkkt_debug_gemv_dense.argtypes = [C.c_int, C.c_int, C.POINTER(GemvCase)]
    L.hqpkkt_debug_rows_gemv.argtypes = [C.c_int, C.c_int, C.POINTER(RowsCase)]
    L.hqpkkt_debug_symv.argtypes = [C.c_int, C.POINTER(GemvCase)]
    L.hqpkkt_debug_symv_batch.argtypes = [C.c_int, C.c_int, C.POINTER(GemvCase), vp, C.c_longlong, vp, C.c_longlong, C.c_int, C.c_int]
    L.hqpkkt_debug_symv_map.restype = C.c_longlong
    L.hqpkkt_debug_symv_map.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_longlong]
    L.hqpkkt_debug_solve_top_stamps.argtypes = [vp, vp, C.c_int]
    L.hqpkkt_debug_factor_block.argtypes = [C.c_int, C.c_int, vp, C.c_double, C.c_double, C.c_int, C.c_int] + [vp] * 7
    _lib = L
    return L


_rccl = None


def rccl_lib():
    """libhqpkkt_rccl.so (include/hqpkkt_rccl.h): the RCCL transport of a sharded system."""
    global _rccl
    if _rccl is None:
        lib()  # torch (and its RCCL) first
        R = C.CDLL(RCCL_LIB_PATH)
        R.hqpkkt_rccl_unique_id.argtypes = [C.c_char_p]
        R.hqpkkt_rccl_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        R.hqpkkt_rccl_exchange.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]
        R.hqpkkt_rccl_destroy.argtypes = [C.c_void_p]
        R.hqpkkt_rccl_comm_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        R.hqpkkt_rccl_origin.restype = C.c_char_p
        _rccl = R
    return _rccl


def strerror(code):
    return lib().hqpkkt_strerror(code).decode()
