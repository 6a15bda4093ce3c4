"""ctypes binding of include/dantzig_amd.h (the C ABI of the HIP engine).

There is no CPU fallback: if the shared library is missing or no MI355X is visible the
calls raise, loudly.  Build the library with `python -m dantzig_amd._build` (or
`__graft_entry__.build()`); it is kept in-tree next to this file.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdantzig_amd.so")

# dzg_status
OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT, SINGULAR, PANIC, RUNNING, NEAR_TIE, NODE_LIMIT = range(9)
E_DEVICE, E_ARG, E_NOMEM = -1, -2, -3
STRICT, FAST, AUTO = 0, 1, 2
PRICE_AUTO, PRICE_SEQ, PRICE_WAVE, PRICE_TREE = 0, 1, 2, 3
STEP_PRIMAL, STEP_DUAL = 0, 1
NEAR_TIE_COUNT, NEAR_TIE_STOP = 0, 1
(K_STATUS, K_FTRAN, K_RATIO, K_BTRAN, K_PRICE, K_UPDATE, K_BASIS_UPDATE, K_LU, K_XCHG1, K_XCHG2,
 K_COUNT) = range(11)
KERNEL_CLASSES = ["status", "ftran", "ratio", "btran", "price", "update", "basis_update", "lu",
                  "exchange1", "exchange2"]

EXPORTS = [
    "dzg_abi_version", "dzg_status_str", "dzg_last_error", "dzg_device_count",
    "dzg_opts_default", "dzg_solver_create", "dzg_solver_run", "dzg_solver_result",
    "dzg_solver_destroy", "dzg_core_solve", "dzg_model_solve", "dzg_build_standard_form",
    "dzg_kernel_lu_solve", "dzg_kernel_neg_t_dot", "dzg_kernel_first_pivot",
    "dzg_kernel_second_pivot", "dzg_gen_dense_lp", "dzg_gen_sparse_lp", "dzg_merge_candidates",
    "dzg_shard_record_doubles", "dzg_shard_phase1", "dzg_shard_phase2", "dzg_shard_phase3",
    "dzg_solver_poll", "dzg_solver_set_budget", "dzg_comm_unique_id", "dzg_shard_comm_init",
    "dzg_shard_run", "dzg_shard_run_lockstep", "dzg_solver_stream", "dzg_solver_refactor",
    "dzg_gen_dense_lp_block", "dzg_solver_set_profile", "dzg_kernel_neg_t_dot_csc",
    "dzg_shard_comm_size", "dzg_solver_upload_columns", "dzg_debug_hold_cus", "dzg_debug_hold_wait",
    "dzg_core_solve_full_csc", "dzg_debug_live_lists", "dzg_debug_rl_listed",
    "dzg_debug_basis_inverse", "dzg_batch_solve", "dzg_model_solve_batch", "dzg_mip_opts_default",
    "dzg_mip_solve", "dzg_mip_last_warm_stats", "dzg_debug_cand_reduce", "dzg_debug_chain_instance",
    "dzg_debug_chain_price_counts", "dzg_debug_wk_mismatch", "dzg_debug_chain_price_rule",
    "dzg_solver_duals", "dzg_batch_solve_duals", "dzg_model_solve_duals",
    "dzg_model_solve_batch_duals", "dzg_model_map_duals",
    "dzg_solver_ranging", "dzg_batch_solve_ranging", "dzg_model_solve_ranging",
    "dzg_model_solve_batch_ranging",
    "dzg_solver_ray", "dzg_batch_solve_rays", "dzg_model_solve_rays", "dzg_model_solve_batch_rays",
    "dzg_model_map_ray",
    "dzg_batch_solve_fast", "dzg_model_solve_batch_fast", "dzg_debug_batch_fast_inverse",
    "dzg_solver_reoptimize",
    "dzg_solver_extend", "dzg_solver_dims", "dzg_debug_matrix", "dzg_debug_matrix_rows",
    "dzg_debug_extend_ms",
    "dzg_solver_remove",
    "dzg_batch_solve_from", "dzg_debug_batch_restart_ms",
    "dzg_batch_solve_fast_from", "dzg_debug_batch_fast_restart_ms",
    "dzg_batch_solve_post", "dzg_debug_batch_post_ms", "dzg_batch_resolve_post",
    "dzg_batch_create", "dzg_batch_destroy", "dzg_batch_update", "dzg_batch_set_start",
    "dzg_batch_resolve", "dzg_debug_batch_traffic",
    "dzg_mip_solve_nodes", "dzg_mip_last_fast_stats", "dzg_mip_node_opts_default",
    "dzg_debug_mip_fast_node",
]

BATCH_MAX_ROWS = 128  # DZG_BATCH_MAX_ROWS
DUALS_FRESH, DUALS_CARRIED = 1, 2
DUALS_SOURCE_NAMES = {DUALS_FRESH: "fresh", DUALS_CARRIED: "carried"}
RAY_PRIMAL, RAY_FARKAS = 1, 2  # DZG_RAY_PRIMAL, DZG_RAY_FARKAS


class Lp(C.Structure):
    _fields_ = [
        ("m", C.c_int64), ("n", C.c_int64), ("n_struct", C.c_int64),
        ("a", C.c_void_p), ("lda", C.c_int64), ("var_col", C.c_void_p),
        ("c", C.c_void_p), ("constant", C.c_double),
        ("basis", C.c_void_p), ("nonbasis", C.c_void_p), ("x", C.c_void_p), ("z", C.c_void_p),
        ("col_ptr", C.c_void_p), ("row_idx", C.c_void_p), ("val", C.c_void_p),
        ("xbar", C.c_void_p), ("zbar", C.c_void_p),
    ]


class Opts(C.Structure):
    _fields_ = [
        ("numerics", C.c_int32), ("price_kernel", C.c_int32), ("device", C.c_int32),
        ("auto_strict_rows", C.c_int32), ("max_iter", C.c_int64), ("epsilon", C.c_double),
        ("log_capacity", C.c_int64), ("poll_interval", C.c_int32), ("profile", C.c_int32),
        ("col_begin", C.c_int64), ("col_end", C.c_int64), ("rank", C.c_int32),
        ("world", C.c_int32), ("stream", C.c_void_p), ("refactor_interval", C.c_int64),
        ("a_is_block", C.c_int32), ("near_tie_action", C.c_int32),
        ("replicate_matrix", C.c_int32), ("auto_restart_rows", C.c_int32), ("tie_tol", C.c_double),
        ("seven_launches", C.c_int32), ("auto_strict_budget_s", C.c_int32),
        ("shard_rows", C.c_int32), ("reserved0", C.c_int32),
    ]


class Pivot(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("entering", C.c_int64),
                ("leaving", C.c_int64), ("mu", C.c_double)]


class Result(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("numerics_used", C.c_int32), ("iterations", C.c_int64),
        ("objective", C.c_double),
        ("basis", C.c_void_p), ("nonbasis", C.c_void_p), ("x", C.c_void_p), ("xbar", C.c_void_p),
        ("z", C.c_void_p), ("zbar", C.c_void_p), ("log", C.c_void_p), ("log_cap", C.c_int64),
        ("kernel_ms", C.c_double * K_COUNT), ("kernel_launches", C.c_int64 * K_COUNT),
        ("price_bytes", C.c_double), ("solve_ms", C.c_double), ("max_pivot_error", C.c_double),
        ("near_ties", C.c_int64), ("first_near_tie", C.c_int64), ("min_margin", C.c_double),
        ("margins", C.c_void_p), ("dense_columns", C.c_int64), ("refactors", C.c_int64),
        ("chain_fallbacks", C.c_int64), ("price_pass_used", C.c_int32),
        ("price_rows_copy", C.c_int32), ("state_drift", C.c_double),
    ]


class Model(C.Structure):
    _fields_ = [
        ("nvars", C.c_int64), ("has_lb", C.c_void_p), ("has_ub", C.c_void_p),
        ("lb", C.c_void_p), ("ub", C.c_void_p),
        ("obj_nterms", C.c_int64), ("obj_var", C.c_void_p), ("obj_coef", C.c_void_p),
        ("obj_const", C.c_double),
        ("ncons", C.c_int64), ("con_ptr", C.c_void_p), ("con_var", C.c_void_p),
        ("con_coef", C.c_void_p), ("con_b", C.c_void_p),
    ]


class ModelResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("numerics_used", C.c_int32), ("iterations", C.c_int64),
                ("objective", C.c_double), ("values", C.c_void_p), ("m", C.c_int64),
                ("n", C.c_int64), ("near_ties", C.c_int64), ("first_near_tie", C.c_int64)]


class Duals(C.Structure):
    _fields_ = [("source", C.c_int32), ("reserved", C.c_int32), ("y", C.c_void_p), ("d", C.c_void_p),
                ("primal_obj", C.c_double), ("dual_obj", C.c_double), ("primal_infeas", C.c_double),
                ("dual_infeas", C.c_double), ("z_diff", C.c_double)]


class ModelDuals(C.Structure):
    _fields_ = [("con_dual", C.c_void_p), ("var_rc", C.c_void_p), ("lb_dual", C.c_void_p),
                ("ub_dual", C.c_void_p), ("core", Duals)]


class RangingReq(C.Structure):
    _fields_ = [("ncost", C.c_int64), ("cost_ptr", C.c_void_p), ("cost_idx", C.c_void_p),
                ("cost_val", C.c_void_p), ("nrhs", C.c_int64), ("rhs_ptr", C.c_void_p),
                ("rhs_idx", C.c_void_p), ("rhs_val", C.c_void_p), ("pivot_tol", C.c_double)]


class Ranging(C.Structure):
    _fields_ = [("cost_lo", C.c_void_p), ("cost_hi", C.c_void_p), ("cost_lo_var", C.c_void_p),
                ("cost_hi_var", C.c_void_p), ("rhs_lo", C.c_void_p), ("rhs_hi", C.c_void_p),
                ("rhs_lo_var", C.c_void_p), ("rhs_hi_var", C.c_void_p)]


class Ray(C.Structure):
    _fields_ = [("kind", C.c_int32), ("proven", C.c_int32), ("var", C.c_int64), ("pos", C.c_int64),
                ("mu", C.c_double), ("value", C.c_double), ("violation", C.c_double),
                ("d", C.c_void_p), ("y", C.c_void_p)]


class ModelRay(C.Structure):
    _fields_ = [("var", C.c_void_p), ("con", C.c_void_p), ("lb", C.c_void_p), ("ub", C.c_void_p),
                ("core", Ray)]


class Reopt(C.Structure):
    _fields_ = [("rhs", C.c_void_p), ("c", C.c_void_p), ("constant", C.c_double),
                ("set_constant", C.c_int32), ("reserved", C.c_int32)]


class BatchStart(C.Structure):
    _fields_ = [("basis", C.c_void_p), ("nonbasis", C.c_void_p)]


class BatchPost(C.Structure):
    _fields_ = [("du", C.c_void_p), ("req", C.c_void_p), ("rg", C.c_void_p), ("ry", C.c_void_p)]


class BatchChange(C.Structure):
    _fields_ = [("lp", C.c_int64), ("rhs", C.c_void_p), ("c", C.c_void_p), ("constant", C.c_double),
                ("set_constant", C.c_int32), ("reserved", C.c_int32)]


class Extend(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("n_cols", C.c_int64), ("rows", C.c_void_p), ("ld_rows", C.c_int64),
                ("rhs", C.c_void_p), ("cols", C.c_void_p), ("ld_cols", C.c_int64), ("c_cols", C.c_void_p)]


class Remove(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("rows", C.c_void_p), ("n_cols", C.c_int64), ("cols", C.c_void_p)]


class ModelRangingReq(C.Structure):
    _fields_ = [("nvar", C.c_int64), ("var", C.c_void_p), ("nrow", C.c_int64), ("row_ptr", C.c_void_p),
                ("row_idx", C.c_void_p), ("row_coef", C.c_void_p), ("pivot_tol", C.c_double)]


class StdForm(C.Structure):
    _fields_ = [
        ("m", C.c_int64), ("n", C.c_int64), ("n_struct", C.c_int64), ("lda", C.c_int64),
        ("a", C.c_void_p), ("var_col", C.c_void_p), ("c", C.c_void_p), ("constant", C.c_double),
        ("basis", C.c_void_p), ("nonbasis", C.c_void_p), ("x", C.c_void_p), ("z", C.c_void_p),
        ("pos_var", C.c_void_p), ("neg_var", C.c_void_p),
    ]


class MipOpts(C.Structure):
    _fields_ = [("node_limit", C.c_int64), ("nodes_per_round", C.c_int32), ("warm_start", C.c_int32),
                ("pivots_per_launch", C.c_int64), ("int_tol", C.c_double), ("abs_gap", C.c_double),
                ("rel_gap", C.c_double)]


class MipWarmStats(C.Structure):
    _fields_ = [("nodes_warm", C.c_int64), ("nodes_restarted", C.c_int64),
                ("warm_iterations", C.c_int64), ("restart_iterations", C.c_int64)]


class MipNodeOpts(C.Structure):
    _fields_ = [("numerics", C.c_int32), ("reserved", C.c_int32), ("pivots_per_launch", C.c_int64),
                ("refactor_every", C.c_int64), ("route", C.c_void_p), ("route_cap", C.c_int64)]


class MipFastStats(C.Structure):
    _fields_ = [("nodes_fast", C.c_int64), ("nodes_rejected", C.c_int64),
                ("fast_iterations", C.c_int64), ("strict_iterations", C.c_int64)]


class MipDebugNode(C.Structure):
    _fields_ = [("status", C.c_int32), ("route", C.c_int32), ("iterations", C.c_int64),
                ("fast_iterations", C.c_int64), ("objective", C.c_double)]


class MipNode(C.Structure):
    _fields_ = [("id", C.c_int64), ("parent", C.c_int64), ("branch_var", C.c_int64),
                ("direction", C.c_int32), ("status", C.c_int32), ("bound", C.c_double),
                ("iterations", C.c_int64), ("objective", C.c_double)]


class MipResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("has_incumbent", C.c_int32), ("objective", C.c_double),
                ("values", C.c_void_p), ("best_bound", C.c_double), ("nodes_solved", C.c_int64),
                ("nodes_batched", C.c_int64), ("nodes_sequential", C.c_int64), ("nodes_fast", C.c_int64),
                ("nodes_pruned", C.c_int64), ("nodes_dropped", C.c_int64), ("rounds", C.c_int64),
                ("lp_iterations", C.c_int64), ("incumbent_node", C.c_int64), ("failed_node", C.c_int64),
                ("log", C.c_void_p), ("log_cap", C.c_int64), ("log_count", C.c_int64)]


class Candidate(C.Structure):
    _fields_ = [("ratio", C.c_double), ("pos", C.c_int64), ("y", C.c_double),
                ("ybar", C.c_double), ("dy", C.c_double)]


class DantzigAmdError(RuntimeError):
    """A call into the HIP engine failed (no GPU, bad argument, out of memory)."""


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DantzigAmdError(
                f"{LIB_PATH} is missing: build the HIP engine first "
                "(python -m dantzig_amd._build). dantzig_amd has no CPU fallback.")
        _lib = C.CDLL(LIB_PATH)
        _lib.dzg_status_str.restype = C.c_char_p
        _lib.dzg_last_error.restype = C.c_char_p
        _lib.dzg_merge_candidates.restype = C.c_int64
        _lib.dzg_solver_destroy.restype = None
        _lib.dzg_opts_default.restype = None
        _lib.dzg_gen_dense_lp.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p]
        _lib.dzg_gen_dense_lp_block.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_int64,
                                                C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                C.c_void_p]
        _lib.dzg_solver_run.argtypes = [C.c_void_p, C.c_int64]
        _lib.dzg_solver_result.argtypes = [C.c_void_p, C.c_void_p]
        _lib.dzg_solver_destroy.argtypes = [C.c_void_p]
        _lib.dzg_shard_record_doubles.restype = C.c_int64
        _lib.dzg_shard_record_doubles.argtypes = [C.c_void_p]
        _lib.dzg_shard_phase1.argtypes = [C.c_void_p, C.c_void_p]
        _lib.dzg_shard_phase2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.dzg_shard_phase3.argtypes = [C.c_void_p, C.c_void_p]
        _lib.dzg_solver_poll.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.dzg_solver_set_budget.argtypes = [C.c_void_p, C.c_int64]
        _lib.dzg_comm_unique_id.argtypes = [C.c_void_p]
        _lib.dzg_shard_comm_init.argtypes = [C.c_void_p, C.c_void_p]
        _lib.dzg_shard_run.argtypes = [C.c_void_p, C.c_int64]
        _lib.dzg_shard_comm_size.argtypes = [C.c_void_p]
        _lib.dzg_shard_run_lockstep.argtypes = [C.c_void_p, C.c_int32, C.c_int64]
        _lib.dzg_solver_stream.restype = C.c_void_p
        _lib.dzg_solver_stream.argtypes = [C.c_void_p]
        _lib.dzg_solver_refactor.argtypes = [C.c_void_p]
        _lib.dzg_solver_set_profile.argtypes = [C.c_void_p, C.c_int32]
        _lib.dzg_core_solve_full_csc.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
        _lib.dzg_debug_hold_cus.argtypes = [C.c_int32, C.c_int32, C.c_double]
        _lib.dzg_debug_live_lists.restype = C.c_int64
        _lib.dzg_debug_live_lists.argtypes = [C.c_void_p, C.c_void_p]
        _lib.dzg_debug_basis_inverse.restype = C.c_int
        _lib.dzg_debug_basis_inverse.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        _lib.dzg_debug_cand_reduce.restype = C.c_int
        _lib.dzg_debug_cand_reduce.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.dzg_debug_chain_instance.restype = C.c_int
        _lib.dzg_debug_chain_instance.argtypes = [C.c_int32] * 7
        _lib.dzg_debug_chain_price_counts.argtypes = [C.c_void_p, C.c_void_p]
        _lib.dzg_debug_wk_mismatch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        _lib.dzg_debug_chain_price_rule.restype = C.c_int
        _lib.dzg_debug_chain_price_rule.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                                    C.c_int32, C.c_int32]
        _lib.dzg_batch_solve.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        _lib.dzg_model_solve_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _lib.dzg_batch_solve_fast.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                              C.c_void_p]
        _lib.dzg_model_solve_batch_fast.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _lib.dzg_debug_batch_fast_inverse.restype = C.c_int
        _lib.dzg_debug_batch_fast_inverse.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                                      C.c_void_p, C.c_void_p]
        _lib.dzg_solver_duals.argtypes = [C.c_void_p, C.c_void_p]
        _lib.dzg_batch_solve_duals.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                               C.c_void_p]
        _lib.dzg_model_solve_duals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.dzg_model_solve_batch_duals.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]
        _lib.dzg_model_map_duals.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        _lib.dzg_solver_ranging.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.dzg_batch_solve_ranging.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.dzg_model_solve_ranging.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
        _lib.dzg_model_solve_batch_ranging.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.dzg_solver_ray.argtypes = [C.c_void_p, C.c_void_p]
        _lib.dzg_batch_solve_rays.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                              C.c_void_p, C.c_void_p]
        _lib.dzg_model_solve_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.dzg_model_solve_batch_rays.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p]
        _lib.dzg_model_map_ray.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_int64, C.c_void_p]
        _lib.dzg_solver_reoptimize.argtypes = [C.c_void_p, C.c_void_p]
        _lib.dzg_solver_extend.argtypes = [C.c_void_p, C.c_void_p]
        _lib.dzg_solver_remove.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.dzg_solver_dims.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.dzg_batch_solve_from.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_void_p]
        _lib.dzg_debug_batch_restart_ms.restype = C.c_double
        _lib.dzg_debug_batch_restart_ms.argtypes = []
        _lib.dzg_batch_solve_fast_from.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                   C.c_int64, C.c_void_p]
        _lib.dzg_debug_batch_fast_restart_ms.restype = C.c_double
        _lib.dzg_debug_batch_fast_restart_ms.argtypes = []
        _lib.dzg_batch_solve_post.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                              C.c_int64, C.c_void_p, C.c_void_p]
        _lib.dzg_debug_batch_post_ms.restype = C.c_double
        _lib.dzg_debug_batch_post_ms.argtypes = []
        _lib.dzg_batch_create.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                          C.c_void_p]
        _lib.dzg_batch_destroy.restype = None
        _lib.dzg_batch_destroy.argtypes = [C.c_void_p]
        _lib.dzg_batch_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        _lib.dzg_batch_set_start.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _lib.dzg_batch_resolve.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        _lib.dzg_batch_resolve_post.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        _lib.dzg_debug_batch_traffic.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.dzg_debug_matrix.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]
        _lib.dzg_debug_matrix_rows.restype = C.c_int64
        _lib.dzg_debug_matrix_rows.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]
        _lib.dzg_debug_extend_ms.argtypes = [C.c_void_p, C.c_void_p]
        _lib.dzg_mip_opts_default.restype = None
        _lib.dzg_mip_opts_default.argtypes = [C.c_void_p]
        _lib.dzg_mip_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.dzg_mip_last_warm_stats.restype = None
        _lib.dzg_mip_last_warm_stats.argtypes = [C.c_void_p]
        _lib.dzg_mip_node_opts_default.restype = None
        _lib.dzg_mip_node_opts_default.argtypes = [C.c_void_p]
        _lib.dzg_mip_solve_nodes.argtypes = [C.c_void_p] * 6
        _lib.dzg_mip_last_fast_stats.restype = None
        _lib.dzg_mip_last_fast_stats.argtypes = [C.c_void_p]
        _lib.dzg_debug_mip_fast_node.argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_int64] + [C.c_void_p] * 7
        _lib.dzg_solver_upload_columns.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                                   C.c_int64]
    return _lib


def ptr(a: np.ndarray | None) -> C.c_void_p:
    return C.c_void_p(None if a is None else a.ctypes.data)


def f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def i64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int64)


def status_str(code: int) -> str:
    return lib().dzg_status_str(int(code)).decode()


def check(rc: int, what: str) -> int:
    """Negative return codes are call failures: raise.  Non-negative are solver outcomes."""
    if rc < 0:
        msg = lib().dzg_last_error().decode()
        raise DantzigAmdError(f"{what}: {status_str(rc)} ({msg})")
    return rc


class RangingBuffers:
    """One dzg_ranging_req / dzg_ranging pair and the arrays they point at.  cost_dirs / rhs_dirs:
    lists of {index: coefficient}."""

    def __init__(self, cost_dirs, rhs_dirs, pivot_tol: float = 0.0):
        def csr(dirs):
            ptr_, idx, val = [0], [], []
            for d in dirs:
                for j, v in d.items():
                    idx.append(int(j))
                    val.append(float(v))
                ptr_.append(len(idx))
            return i64(ptr_), i64(idx + [0]), f64(val + [0.0])

        self.nc, self.nr = len(cost_dirs), len(rhs_dirs)
        self.cost = csr(cost_dirs)
        self.rhs = csr(rhs_dirs)
        self.pivot_tol = float(pivot_tol)
        self.lo = [np.zeros(max(self.nc, 1)), np.zeros(max(self.nr, 1))]
        self.hi = [np.zeros(max(self.nc, 1)), np.zeros(max(self.nr, 1))]
        self.lo_var = [np.zeros(max(self.nc, 1), dtype=np.int64), np.zeros(max(self.nr, 1), dtype=np.int64)]
        self.hi_var = [np.zeros(max(self.nc, 1), dtype=np.int64), np.zeros(max(self.nr, 1), dtype=np.int64)]

    def fill(self, req: RangingReq, out: Ranging) -> None:
        req.ncost, req.nrhs, req.pivot_tol = self.nc, self.nr, self.pivot_tol
        req.cost_ptr, req.cost_idx, req.cost_val = (ptr(a) for a in self.cost)
        req.rhs_ptr, req.rhs_idx, req.rhs_val = (ptr(a) for a in self.rhs)
        self.fill_out(out)

    def fill_out(self, out: Ranging) -> None:
        out.cost_lo, out.cost_hi = ptr(self.lo[0]), ptr(self.hi[0])
        out.cost_lo_var, out.cost_hi_var = ptr(self.lo_var[0]), ptr(self.hi_var[0])
        out.rhs_lo, out.rhs_hi = ptr(self.lo[1]), ptr(self.hi[1])
        out.rhs_lo_var, out.rhs_hi_var = ptr(self.lo_var[1]), ptr(self.hi_var[1])

    def side(self, which: int):
        """(lo, hi, lo_var, hi_var) of the cost (0) or right-hand-side (1) directions."""
        n = self.nc if which == 0 else self.nr
        return (self.lo[which][:n].copy(), self.hi[which][:n].copy(), self.lo_var[which][:n].copy(),
                self.hi_var[which][:n].copy())


def check_ray(rc: int, what: str) -> int:
    """check(), but a route without rays (the C call says so) is a NotImplementedError."""
    if rc < 0:
        msg = lib().dzg_last_error().decode()
        if "rays are not supported" in msg:
            raise NotImplementedError(f"{what}: {msg}")
    return check(rc, what)


def check_ranging(rc: int, what: str) -> int:
    """check(), but a route without ranging (the C call says so) is a NotImplementedError."""
    if rc < 0:
        msg = lib().dzg_last_error().decode()
        if "ranging is not supported" in msg:
            raise NotImplementedError(f"{what}: {msg}")
    return check(rc, what)


def check_reopt(rc: int, what: str) -> int:
    """check(), but a route without re-optimisation (the C call says so) is a NotImplementedError."""
    if rc < 0:
        msg = lib().dzg_last_error().decode()
        if "reoptimize is not supported" in msg:
            raise NotImplementedError(f"{what}: {msg}")
    return check(rc, what)


def check_extend(rc: int, what: str) -> int:
    """check(), but a route that cannot grow or shrink its LP (the C call says so) is a
    NotImplementedError."""
    if rc < 0:
        msg = lib().dzg_last_error().decode()
        if "extend is not supported" in msg or "remove is not supported" in msg:
            raise NotImplementedError(f"{what}: {msg}")
    return check(rc, what)


def default_opts(**kw) -> Opts:
    o = Opts()
    lib().dzg_opts_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown option {k!r}")
        setattr(o, k, v)
    return o


def default_mip_opts(**kw) -> MipOpts:
    o = MipOpts()
    lib().dzg_mip_opts_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown MIP option {k!r}")
        setattr(o, k, int(v) if k == "warm_start" else v)
    return o


def default_mip_node_opts(**kw) -> MipNodeOpts:
    """dzg_mip_node_opts (dzg_mip_solve_nodes): numerics takes STRICT / FAST or "strict" / "fast"."""
    o = MipNodeOpts()
    lib().dzg_mip_node_opts_default(C.byref(o))
    for k, v in kw.items():
        if k == "reserved" or not hasattr(o, k):
            raise TypeError(f"unknown MIP node option {k!r}")
        if k == "numerics" and isinstance(v, str):
            if v not in ("strict", "fast"):
                raise ValueError(f"node numerics must be 'strict' or 'fast', not {v!r}")
            v = FAST if v == "fast" else STRICT
        setattr(o, k, v)
    return o


def mip_last_fast_stats() -> MipFastStats:
    """What the FAST node attempts did in this thread's last search (zeros after any other)."""
    out = MipFastStats()
    lib().dzg_mip_last_fast_stats(C.byref(out))
    return out


def mip_last_warm_stats() -> MipWarmStats:
    """What warm_start did in this thread's last dzg_mip_solve (zeros after a cold search)."""
    out = MipWarmStats()
    lib().dzg_mip_last_warm_stats(C.byref(out))
    return out


def require_gpu() -> None:
    if lib().dzg_device_count() <= 0:
        raise DantzigAmdError("no HIP device visible: dantzig_amd runs on an MI355X only "
                              "(there is no CPU fallback)")
