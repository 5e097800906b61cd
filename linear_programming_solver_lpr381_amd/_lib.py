"""ctypes loader for liblpx.so -- the C ABI declared in include/lpx.h.

There is no CPU fallback anywhere in this package: if the shared library is missing, or no
gfx950 device is visible when a compute entry point is called, the call raises.
"""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
# LPX_LIB_PATH: diagnostic builds only (e.g. the -DLPX_STAMPS library of tools/diag_select_stamps.py)
LIB_PATH = os.environ.get("LPX_LIB_PATH") or os.path.join(_PKG, "liblpx.so")

# status / error codes (include/lpx.h)
OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT, RUNNING, CUTOFF = 0, 1, 2, 3, 4, 5
CUT_INTEGER, CUT_INCOMPLETE, CUT_ERROR, CUT_NOT_OPTIMAL = 0, 10, 11, 12
EINVAL, EDEVICE, ENOMEM = -1, -2, -3
BDUAL_SKIP_FIXED = 1        # LPX_BDUAL_SKIP_FIXED (lpx_bounded_dual_run2)
BDUAL_LONG_STEP, BDUAL_CUTOFF = 2, 4        # LPX_BDUAL_LONG_STEP, LPX_BDUAL_CUTOFF (lpx_bounded_dual_run3)
NODE_LAUNCHES, NODE_ONCHIP, NODE_AUTO = 0, 1, 2     # LPX_NODE_* (lpx_bounded_node3, lpx_solve_bnb_bounded3)
NODE_FORMS = {"launches": NODE_LAUNCHES, "onchip": NODE_ONCHIP, "auto": NODE_AUTO}
E_GE_PRESENT, E_NEG_RHS, E_REVISED_PRECOND, E_SINGULAR, E_KNAP_SHAPE, E_UNKNOWN_ALGO, E_PARSE = (
    -10, -11, -12, -13, -14, -15, -16)

STATUS_NAMES = {OPTIMAL: "OPTIMAL", UNBOUNDED: "UNBOUNDED", INFEASIBLE: "INFEASIBLE",
                ITER_LIMIT: "ITER_LIMIT", CUTOFF: "CUTOFF"}

dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)
PIVOT_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int)


class Stats(C.Structure):
    _fields_ = [("pivots", C.c_int64), ("launches", C.c_int64), ("loop_ms", C.c_double),
                ("h2d_ms", C.c_double), ("d2h_ms", C.c_double), ("update_ms_sum", C.c_double),
                ("update_launches", C.c_int64), ("fdf_pivots", C.c_int64), ("cleanup_pivots", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RunOpts(C.Structure):
    _fields_ = [("eps", C.c_double), ("ratio_tol", C.c_double), ("max_iter", C.c_int),
                ("fdf_guard", C.c_int), ("cleanup", C.c_int), ("batch", C.c_int),
                ("use_graph", C.c_int), ("profile", C.c_int), ("resident", C.c_int)]


ALLREDUCE_CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double), C.c_int)
TEXT_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.POINTER(C.c_uint8), C.c_int, C.c_int)


# test seams (include/lpx_test.h): only the CPU test-suite sets these
TEST_NODE_LP = C.CFUNCTYPE(C.c_int, C.c_void_p, dp, C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp,
                           C.POINTER(C.c_int64))
TEST_KNAP_RELAX = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, ip, ip, C.POINTER(C.c_int8), dp, dp, ip, dp)


class Problem(C.Structure):
    _fields_ = [("sense", C.c_int), ("n", C.c_int), ("m", C.c_int), ("c", dp), ("A", dp), ("rel", ip), ("b", dp)]


class SolveOpts(C.Structure):
    _fields_ = [("max_iter", C.c_int), ("batch", C.c_int), ("render_iterations", C.c_int),
                ("dual_flags", C.c_int), ("bnb_mode", C.c_int), ("bnb_search", C.c_int),
                ("concurrent_nodes", C.c_int), ("rank", C.c_int), ("world", C.c_int),
                ("max_nodes", C.c_int64), ("allreduce_max", ALLREDUCE_CB), ("allreduce_user", C.c_void_p),
                ("text_cb", TEXT_CB), ("text_user", C.c_void_p),
                ("bnb_dive", C.c_int)]


class TestSeams(C.Structure):
    """include/lpx_test.h: test-only stand-ins for the device loops (never installed by the package itself)."""
    _fields_ = [("node_lp", TEST_NODE_LP), ("knap_relax", TEST_KNAP_RELAX), ("user", C.c_void_p),
                ("fail_after_nodes", C.c_int64)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int), ("has_solution", C.c_int), ("optimal_value", C.c_double),
                ("n", C.c_int), ("x", dp), ("R", C.c_int), ("C", C.c_int), ("T", dp), ("basis", ip),
                ("n_pivots", C.c_int), ("trace", ip), ("report", C.c_char_p), ("summary", C.c_char_p),
                ("lp_solves", C.c_int64), ("nodes", C.c_int64), ("n_log", C.c_int), ("node_log", ip),
                ("node_z", dp), ("aux", C.c_double * 4), ("stats", Stats), ("n_cuts", C.c_int), ("cuts", dp)]


class Ranging(C.Structure):
    """lpx_ranging: the report of lpx_solve_ranging in user terms (freed by lpx_ranging_free)."""
    _fields_ = [("n", C.c_int), ("m", C.c_int), ("valid", C.c_int), ("min_rhs", C.c_double), ("min_dj", C.c_double),
                ("cost_lo", dp), ("cost_hi", dp), ("cost_lo_at", ip), ("cost_hi_at", ip), ("reduced_cost", dp),
                ("rhs_lo", dp), ("rhs_hi", dp), ("rhs_lo_at", ip), ("rhs_hi_at", ip), ("dual", dp)]


class CutOpts(C.Structure):
    """lpx_cut_opts (include/lpx.h): options of the GMI cut round and loop."""
    _fields_ = [("cuts_per_round", C.c_int), ("max_rounds", C.c_int), ("max_active", C.c_int), ("purge", C.c_int),
                ("away", C.c_double), ("coef_eps", C.c_double), ("max_dynamism", C.c_double), ("purge_tol", C.c_double),
                ("int_tol", C.c_double)]


class SessionOpts(C.Structure):
    """lpx_session_opts (include/lpx.h): capacity and run options of a warm post-optimal session."""
    _fields_ = [("extra_rows", C.c_int), ("extra_cols", C.c_int), ("max_iter", C.c_int), ("batch", C.c_int),
                ("want_tableau", C.c_int)]


class BoundedInfo(C.Structure):
    """lpx_bounded_info (include/lpx.h): bound states of lpx_solve_bounded's final tableau (freed by lpx_bounded_info_free)."""
    _fields_ = [("ncols", C.c_int), ("n", C.c_int), ("flip", C.POINTER(C.c_uint8)), ("ub", dp), ("lower", dp)]


class BranchPick(C.Structure):
    """lpx_branch_pick (include/lpx.h): the branching variable of a solved bounded tableau."""
    _fields_ = [("var", C.c_int32), ("candidates", C.c_int32), ("x_var", C.c_double), ("z", C.c_double)]


class NodeRecord(C.Structure):
    """lpx_node_record (include/lpx.h): what one lpx_bounded_node call did."""
    _fields_ = [("status", C.c_int32), ("events", C.c_int32), ("kind0", C.c_int64), ("kind1", C.c_int64),
                ("flips", C.c_int64), ("unrepairable", C.c_int64), ("pick", BranchPick)]


class CutLoopRecord(C.Structure):
    """lpx_cut_loop_record (include/lpx.h): what one lpx_bounded_cut_loop call did; z_before / z_after are the caller's arrays."""
    _fields_ = [("rounds", C.c_int32), ("added", C.c_int32), ("purged", C.c_int32), ("stop", C.c_int32),
                ("status", C.c_int32), ("R", C.c_int32), ("C", C.c_int32), ("pad", C.c_int32), ("events", C.c_int64),
                ("pick", BranchPick), ("z_before", dp), ("z_after", dp)]


class BnbCutInfo(C.Structure):
    """lpx_bnb_cut_info (include/lpx.h): the cut loop at the root of lpx_solve_bnb_bounded9 (freed by lpx_bnb_cut_info_free)."""
    _fields_ = [("ran", C.c_int32), ("spare", C.c_int32), ("rounds", C.c_int32), ("added", C.c_int32), ("purged", C.c_int32),
                ("stop", C.c_int32), ("status", C.c_int32), ("R", C.c_int32), ("C", C.c_int32), ("n_z", C.c_int32),
                ("events", C.c_int64), ("z_before", dp), ("z_after", dp)]


CUTLOOP_STOPS = ("integral", "stalled", "rounds", "infeasible", "iter_limit", "status")     # LPX_CUTLOOP_*


class BnbNodeLog(C.Structure):
    """lpx_bnb_node_log (include/lpx.h): one node of lpx_solve_bnb_bounded."""
    _fields_ = [("depth", C.c_int32), ("K", C.c_int32), ("status", C.c_int32), ("events", C.c_int32),
                ("flips", C.c_int32), ("var", C.c_int32), ("z", C.c_double)]


class BnbBoundedInfo(C.Structure):
    """lpx_bnb_bounded_info (include/lpx.h): counters and node log of lpx_solve_bnb_bounded (freed by lpx_bnb_bounded_info_free)."""
    _fields_ = [("nodes", C.c_int64), ("events", C.c_int64), ("flips", C.c_int64), ("incumbents", C.c_int64),
                ("pruned_bound", C.c_int64), ("pruned_infeasible", C.c_int64), ("max_K", C.c_int64),
                ("constant", C.c_double), ("n_log", C.c_int64), ("log", C.POINTER(BnbNodeLog))]


class BnbDiversInfo(C.Structure):
    """lpx_bnb_divers_info (include/lpx.h): rounds, steals and the per-node round / diver of lpx_solve_bnb_bounded4 (freed by
    lpx_bnb_divers_info_free)."""
    _fields_ = [("rounds", C.c_int64), ("steals", C.c_int64), ("largest_batch", C.c_int64), ("round", ip), ("diver", ip)]


class BnbPlungeInfo(C.Structure):
    """lpx_bnb_plunge_info (include/lpx.h): the records launched and dropped, the longest chain and the per-node step of
    lpx_solve_bnb_bounded5 (freed by lpx_bnb_plunge_info_free)."""
    _fields_ = [("launched", C.c_int64), ("dropped", C.c_int64), ("longest_chain", C.c_int64), ("step", ip)]


PROBE_NONE = -2
BRANCH_MOST_FRACTIONAL, BRANCH_STRONG = 0, 1
BRANCHINGS = {"most_fractional": BRANCH_MOST_FRACTIONAL, "strong": BRANCH_STRONG}


class ProbeHead(C.Structure):
    """lpx_probe_head (include/lpx.h): how many candidates a probe launch evaluated on one handle, of how many, and the node's z."""
    _fields_ = [("count", C.c_int32), ("candidates", C.c_int32), ("z", C.c_double)]


class ProbeRecord(C.Structure):
    """lpx_probe_record (include/lpx.h): one child of one candidate as its probe left it."""
    _fields_ = [("status", C.c_int32), ("events", C.c_int32), ("kind0", C.c_int32), ("kind1", C.c_int32), ("flips", C.c_int32),
                ("var", C.c_int32), ("dir", C.c_int32), ("pad", C.c_int32), ("x_var", C.c_double), ("lower", C.c_double),
                ("upper", C.c_double), ("z", C.c_double)]


class BnbStrongInfo(C.Structure):
    """lpx_bnb_strong_info (include/lpx.h): the probe counters of lpx_solve_bnb_bounded6."""
    _fields_ = [("probe_launches", C.c_int64), ("probes", C.c_int64), ("probe_events", C.c_int64), ("probe_limit", C.c_int64),
                ("pruned_by_probe", C.c_int64), ("changed_picks", C.c_int64)]


class GuardRecord(C.Structure):
    """lpx_guard_record (include/lpx.h): the pivots a node made in Bland mode and the event index of the first (-1: none)."""
    _fields_ = [("bland_events", C.c_int32), ("first_bland", C.c_int32)]


class BnbGuardInfo(C.Structure):
    """lpx_bnb_guard_info (include/lpx.h): the stall-guard counters of lpx_solve_bnb_bounded7."""
    _fields_ = [("guarded_nodes", C.c_int64), ("bland_events", C.c_int64), ("max_events", C.c_int64)]


class PrimalRecord(C.Structure):
    """lpx_primal_record (include/lpx.h): what one entry of lpx_node_batch_primal did."""
    _fields_ = [("status", C.c_int32), ("events", C.c_int32), ("kind0", C.c_int64), ("kind1", C.c_int64), ("flips", C.c_int64),
                ("z", C.c_double)]


class PackedModels(C.Structure):
    """lpx_packed_models (include/lpx.h): count models of one shape as contiguous arrays; a stride of 0 shares one copy."""
    _fields_ = [("count", C.c_int32), ("m", C.c_int32), ("n", C.c_int32), ("sense", C.c_int32),
                ("c", dp), ("A", dp), ("b", dp), ("lower", dp), ("upper", dp),
                ("c_stride", C.c_int64), ("A_stride", C.c_int64), ("b_stride", C.c_int64), ("lower_stride", C.c_int64),
                ("upper_stride", C.c_int64)]


class PackedResults(C.Structure):
    """lpx_packed_results (include/lpx.h): caller-allocated output arrays of lpx_solve_packed; rec, basis, at_upper may be NULL."""
    _fields_ = [("status", ip), ("x", dp), ("value", dp), ("rec", C.POINTER(PrimalRecord)), ("basis", ip),
                ("at_upper", C.POINTER(C.c_uint8))]


class PackedDualModels(C.Structure):
    """lpx_packed_dual_models (include/lpx.h): lpx_packed_models plus rel ([count][m] of LPX_LE / LPX_GE, or NULL) and its stride."""
    _fields_ = PackedModels._fields_ + [("rel", ip), ("rel_stride", C.c_int64)]


class PackedDualRecord(C.Structure):
    """lpx_packed_dual_record (include/lpx.h): what one model of lpx_solve_packed_dual did."""
    _fields_ = [("status", C.c_int32), ("events", C.c_int32), ("kind0", C.c_int64), ("kind1", C.c_int64), ("passes", C.c_int64),
                ("dualize_flips", C.c_int64), ("z", C.c_double)]


class PackedDualResults(C.Structure):
    """lpx_packed_dual_results (include/lpx.h): caller-allocated output arrays; rec, basis, at_upper, y and d may be NULL."""
    _fields_ = [("status", ip), ("x", dp), ("value", dp), ("rec", C.POINTER(PackedDualRecord)), ("basis", ip),
                ("at_upper", C.POINTER(C.c_uint8)), ("y", dp), ("d", dp)]


class PackedBaseModel(C.Structure):
    """lpx_packed_base_model (include/lpx.h): the one model of lpx_packed_base_open; b is the base right-hand side."""
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("sense", C.c_int32), ("c", dp), ("A", dp), ("b", dp), ("lower", dp), ("upper", dp),
                ("rel", ip)]


class PackedCostRecord(C.Structure):
    """lpx_packed_cost_record (include/lpx.h): what one scenario of lpx_packed_base_solve_costs did, loop by loop."""
    _fields_ = [("status", C.c_int32), ("primal_events", C.c_int32), ("dual_events", C.c_int32), ("pad", C.c_int32),
                ("primal_kind0", C.c_int64), ("primal_kind1", C.c_int64), ("primal_flips", C.c_int64),
                ("dual_kind0", C.c_int64), ("dual_kind1", C.c_int64), ("dual_passes", C.c_int64), ("z", C.c_double)]


class PackedCostResults(C.Structure):
    """lpx_packed_cost_results (include/lpx.h): caller-allocated output arrays; rec, basis, at_upper, y and d may be NULL."""
    _fields_ = [("status", ip), ("x", dp), ("value", dp), ("rec", C.POINTER(PackedCostRecord)), ("basis", ip),
                ("at_upper", C.POINTER(C.c_uint8)), ("y", dp), ("d", dp)]


PBNB_DONE, PBNB_ROOT, PBNB_NODES, PBNB_NODE_ITER, PBNB_EVENTS, PBNB_DEPTH, PBNB_REFUSED = range(7)    # LPX_PBNB_* (lpx_solve_packed_bnb)
PBNB_STOPS = ("done", "root", "nodes", "node_iter", "events", "depth", "refused")


class PackedBnbModels(C.Structure):
    """lpx_packed_bnb_models (include/lpx.h): lpx_packed_models plus is_int ([n] bytes shared by every model, or NULL = all)."""
    _fields_ = PackedModels._fields_ + [("is_int", C.POINTER(C.c_uint8))]


class PackedBnbDualModels(C.Structure):
    """lpx_packed_bnb_dual_models (include/lpx.h): lpx_packed_dual_models plus is_int ([n] bytes shared by every model, or NULL = all)."""
    _fields_ = PackedDualModels._fields_ + [("is_int", C.POINTER(C.c_uint8))]


class PackedBnbOpts(C.Structure):
    """lpx_packed_bnb_opts (include/lpx.h): the search flags and the budgets of lpx_solve_packed_bnb, per model."""
    _fields_ = [("search_flags", C.c_int32), ("max_iter", C.c_int32), ("max_depth", C.c_int32), ("log_cap", C.c_int32),
                ("max_nodes", C.c_int64), ("max_events", C.c_int64)]


class PackedBnbRecord(C.Structure):
    """lpx_packed_bnb_record (include/lpx.h): the counters of one model's search, 88 bytes."""
    _fields_ = [("status", C.c_int32), ("stop", C.c_int32), ("nodes", C.c_int64), ("events", C.c_int64), ("flips", C.c_int64),
                ("incumbents", C.c_int64), ("pruned_bound", C.c_int64), ("pruned_infeasible", C.c_int64), ("max_K", C.c_int32),
                ("deepest", C.c_int32), ("root_events", C.c_int32), ("logged", C.c_int32), ("best", C.c_double),
                ("constant", C.c_double)]


class PackedBnbResults(C.Structure):
    """lpx_packed_bnb_results (include/lpx.h): caller-allocated output arrays; rec and log may be NULL."""
    _fields_ = [("status", ip), ("x", dp), ("value", dp), ("rec", C.POINTER(PackedBnbRecord)), ("log", C.POINTER(BnbNodeLog))]


class FixList(C.Structure):
    """lpx_fix_list (include/lpx.h): the caller-owned list of the columns a node tightened, as the triples of a bound edit."""
    _fields_ = [("cap", C.c_int32), ("n", C.c_int32), ("cols", ip), ("lower", dp), ("upper", dp)]


class BnbFixInfo(C.Structure):
    """lpx_bnb_fix_info (include/lpx.h): the reduced-cost tightening counters of lpx_solve_bnb_bounded10."""
    _fields_ = [("tightened_nodes", C.c_int64), ("tightened_cols", C.c_int64), ("max_per_node", C.c_int64)]


class Parsed(C.Structure):
    _fields_ = [("sense", C.c_int), ("n", C.c_int), ("m", C.c_int), ("c", dp), ("A", dp), ("rel", ip),
                ("b", dp), ("ragged", C.c_int)]


class LpxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"liblpx error {code}: {msg}")
        self.code = code


_lib = None


def lib() -> C.CDLL:
    """Loads liblpx.so (built in-tree by __graft_entry__.build()). Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.lpx_abi_version.restype = C.c_int
    L.lpx_device_count.restype = C.c_int
    L.lpx_init.argtypes = [C.c_int]
    L.lpx_last_error.argtypes = [C.c_char_p, C.c_int]
    L.lpx_device_name.argtypes = [C.c_char_p, C.c_int]
    u8p = C.POINTER(C.c_uint8)
    L.lpx_comm_unique_id.argtypes = [u8p]
    L.lpx_comm_init.argtypes = [C.c_int, C.c_int, u8p]
    L.lpx_comm_init_tcp.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int]
    L.lpx_comm_allreduce_max.argtypes = [dp, C.c_int]
    L.lpx_comm_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64), dp, C.POINTER(C.c_int)]
    L.lpx_comm_destroy.argtypes = []
    L.lpx_default_opts.argtypes = [C.POINTER(RunOpts), C.c_int]
    L.lpx_default_opts.restype = None
    L.lpx_tableau_create.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    L.lpx_tableau_destroy.argtypes = [vp]
    L.lpx_tableau_destroy.restype = None
    L.lpx_tableau_upload.argtypes = [vp, dp, ip]
    L.lpx_tableau_download.argtypes = [vp, dp, ip]
    L.lpx_tableau_snapshot.argtypes = [vp]
    L.lpx_tableau_restore.argtypes = [vp]
    L.lpx_tableau_device_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int)]
    L.lpx_tableau_trace.argtypes = [vp, ip, C.c_int, C.POINTER(C.c_int)]
    L.lpx_tableau_shape.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lpx_primal_run.argtypes = [vp, C.POINTER(RunOpts), PIVOT_CB, vp, C.POINTER(Stats)]
    L.lpx_dual_run.argtypes = [vp, C.POINTER(RunOpts), PIVOT_CB, vp, C.POINTER(Stats)]
    L.lpx_forced_pivots_run.argtypes = [vp, ip, ip, C.c_int, C.c_double, ip, C.POINTER(RunOpts),
                                        C.POINTER(Stats)]
    L.lpx_primal_tableau.argtypes = [dp, C.c_int, C.c_int, ip, C.c_double, C.c_int, PIVOT_CB, vp,
                                     C.POINTER(Stats)]
    L.lpx_dual_tableau.argtypes = [dp, C.c_int, C.c_int, ip, C.c_double, C.c_double, C.c_int, C.c_int,
                                   C.c_int, PIVOT_CB, vp, C.POINTER(Stats)]
    L.lpx_revised_create.argtypes = [C.c_int, C.c_int, dp, dp, dp, C.POINTER(vp)]
    L.lpx_revised_destroy.argtypes = [vp]
    L.lpx_revised_destroy.restype = None
    L.lpx_revised_run.argtypes = [vp, C.POINTER(RunOpts), PIVOT_CB, vp, C.POINTER(Stats)]
    L.lpx_revised_result.argtypes = [vp, ip, ip, dp, dp]
    L.lpx_revised_binv.argtypes = [vp, dp]
    L.lpx_revised_iteration_view.argtypes = [vp, dp, dp]
    _sens = [C.POINTER(Problem), dp, C.c_int, C.c_int, ip]
    L.lpx_sensitivity_range_report.argtypes = _sens + [C.c_char_p, C.c_char_p, C.c_int]
    L.lpx_sensitivity_range.argtypes = _sens + [C.c_char_p, dp, dp]
    L.lpx_sensitivity_apply_change.argtypes = _sens + [C.c_char_p, C.c_double, ip, ip, C.c_char_p, C.c_int]
    L.lpx_sensitivity_shadow_prices.argtypes = _sens + [C.c_char_p, C.c_int]
    L.lpx_sensitivity_solve_duality.argtypes = _sens + [C.POINTER(SolveOpts), C.POINTER(Result)]
    L.lpx_revised_profile.argtypes = [vp, C.c_int, dp, C.POINTER(C.c_int)]
    L.lpx_revised_refactor.argtypes = [vp]
    L.lpx_revised_set_refactor_mode.argtypes = [vp, C.c_int]
    L.lpx_revised_set_drift_policy.argtypes = [vp, C.c_int, C.c_double]
    L.lpx_revised_residual.argtypes = [vp, dp, dp]
    L.lpx_revised_refactor_stats.argtypes = [vp, ip, ip, ip, dp, dp, ip]
    L.lpx_revised_set_refactor.argtypes = [vp, C.c_int]
    L.lpx_invert.argtypes = [dp, C.c_int, dp]
    L.lpx_invert_blocked.argtypes = [dp, C.c_int, dp, dp]
    L.lpx_revised_trace.argtypes = [vp, ip, C.c_int, C.POINTER(C.c_int)]
    L.lpx_revised_solve.argtypes = [dp, C.c_int, C.c_int, dp, dp, ip, ip, dp, dp, C.c_double, C.c_int,
                                    PIVOT_CB, vp, C.POINTER(Stats)]
    L.lpx_tableau_solution.argtypes = [vp, C.c_int, dp, dp]
    L.lpx_tableau_set_shape.argtypes = [vp, C.c_int, C.c_int]
    L.lpx_tableau_build_child.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double]
    L.lpx_tableau_basis.argtypes = [vp, ip]
    L.lpx_tableau_solution2.argtypes = [vp, C.c_int, dp, dp, ip]
    L.lpx_store_create.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    L.lpx_store_destroy.argtypes = [vp]
    L.lpx_store_destroy.restype = None
    L.lpx_store_save.argtypes = [vp, vp, C.POINTER(C.c_int)]
    L.lpx_store_release.argtypes = [vp, C.c_int]
    L.lpx_store_save_multi.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_int, C.POINTER(C.c_int)]
    L.lpx_multi_solution.argtypes = [C.POINTER(vp), C.c_int, C.c_int, dp, dp, ip, C.c_int]
    L.lpx_tableau_build_child_from_store.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]
    L.lpx_tableau_build_node.argtypes = [vp, vp, C.c_int, ip, dp, dp, dp]
    L.lpx_tableau_build_children_from_store.argtypes = [C.POINTER(vp), C.POINTER(vp), ip, C.c_int, ip, ip, ip, dp]
    L.lpx_tableau_build_nodes.argtypes = [C.POINTER(vp), vp, C.c_int, ip, ip, dp, dp, dp]
    L.lpx_multi_run.argtypes = [C.POINTER(vp), C.POINTER(C.c_int), C.c_int, C.POINTER(RunOpts), C.POINTER(RunOpts),
                                C.POINTER(C.c_int), C.POINTER(Stats)]
    L.lpx_multi_run_some.argtypes = [C.POINTER(vp), C.POINTER(C.c_int), C.c_int, C.POINTER(RunOpts), C.POINTER(RunOpts),
                                     C.POINTER(C.c_int), C.POINTER(Stats), C.c_int]
    L.lpx_multi_run_begin.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(C.c_int), C.c_int, C.POINTER(RunOpts), C.POINTER(RunOpts), C.c_int]
    L.lpx_multi_run_end.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(Stats)]
    L.lpx_knapsack_create.argtypes = [dp, dp, C.c_int, C.c_double, C.POINTER(vp)]
    L.lpx_knapsack_destroy.argtypes = [vp]
    L.lpx_knapsack_destroy.restype = None
    L.lpx_knapsack_order.argtypes = [vp, ip]
    L.lpx_knapsack_relax_batch.argtypes = [vp, C.c_int, ip, ip, C.POINTER(C.c_int8), dp, dp, ip, dp]
    L.lpx_knapsack_relax_batch2.argtypes = [vp, C.c_int, ip, ip, C.POINTER(C.c_int8), dp, dp, ip, dp]
    L.lpx_test_set_seams.argtypes = [C.POINTER(TestSeams)]
    L.lpx_test_set_seams.restype = None
    L.lpx_test_comm_exchange_id.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_uint8)]
    L.lpx_knapsack_expand_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), ip, C.POINTER(C.c_int8), C.POINTER(C.c_int64),
                                            dp, dp, ip, dp]
    L.lpx_knapsack_expand_begin.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), ip, C.POINTER(C.c_int8), C.POINTER(C.c_int64)]
    L.lpx_knapsack_expand_finish.argtypes = [vp, dp, dp, ip, dp]
    L.lpx_knapsack_node_list.argtypes = [vp, C.c_int64, ip, C.POINTER(C.c_int8), C.c_int, C.POINTER(C.c_int)]
    L.lpx_default_solve_opts.argtypes = [C.POINTER(SolveOpts)]
    L.lpx_default_solve_opts.restype = None
    L.lpx_solve.argtypes = [C.POINTER(Problem), C.c_char_p, C.POINTER(SolveOpts), C.POINTER(Result)]
    L.lpx_result_free.argtypes = [C.POINTER(Result)]
    L.lpx_result_free.restype = None
    L.lpx_tableau_ranging.argtypes = [vp, C.c_double, dp, ip, dp, ip, dp, ip, dp, ip, dp, dp]
    L.lpx_tableau_ranging_pairs.argtypes = [vp, C.c_double, C.c_int, ip, ip, dp, ip, dp, ip]
    L.lpx_solve_ranging.argtypes = [C.POINTER(Problem), C.c_char_p, C.POINTER(SolveOpts), C.POINTER(Result), C.POINTER(Ranging)]
    L.lpx_ranging_free.argtypes = [C.POINTER(Ranging)]
    L.lpx_ranging_free.restype = None
    L.lpx_default_cut_opts.argtypes = [C.POINTER(CutOpts)]
    L.lpx_default_cut_opts.restype = None
    L.lpx_tableau_gmi_round.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.POINTER(CutOpts), C.POINTER(C.c_int), ip,
                                        C.POINTER(C.c_int), ip]
    L.lpx_tableau_gmi_round_bounded.argtypes = L.lpx_tableau_gmi_round.argtypes
    L.lpx_bounded_cut_loop.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.POINTER(CutOpts),
                                       C.POINTER(RunOpts), C.c_int, C.c_int, C.POINTER(CutLoopRecord)]
    L.lpx_solve_cuts.argtypes = [C.POINTER(Problem), C.POINTER(SolveOpts), C.POINTER(CutOpts), C.POINTER(Result)]
    L.lpx_tableau_rhs_update.argtypes = [vp, C.c_int, ip, dp]
    L.lpx_tableau_objective_update.argtypes = [vp, C.c_int, ip, dp, C.c_int, ip, dp]
    L.lpx_tableau_add_column.argtypes = [vp, C.c_int, ip, dp, C.c_double]
    L.lpx_tableau_add_row.argtypes = [vp, C.c_int, ip, dp, dp]
    L.lpx_default_session_opts.argtypes = [C.POINTER(SessionOpts)]
    L.lpx_default_session_opts.restype = None
    L.lpx_session_open.argtypes = [C.POINTER(Problem), C.POINTER(SessionOpts), C.POINTER(vp), C.POINTER(Result)]
    L.lpx_session_set_rhs.argtypes = [vp, C.c_int, ip, dp, C.POINTER(Result)]
    L.lpx_session_set_cost.argtypes = [vp, C.c_int, ip, dp, C.POINTER(Result)]
    L.lpx_session_add_variable.argtypes = [vp, C.c_double, dp, C.POINTER(Result)]
    L.lpx_session_add_constraint.argtypes = [vp, dp, C.c_int, C.c_double, C.POINTER(Result)]
    L.lpx_session_ranging.argtypes = [vp, C.POINTER(Ranging)]
    L.lpx_session_shape.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lpx_session_close.argtypes = [vp]
    L.lpx_session_close.restype = None
    L.lpx_tableau_set_bounds.argtypes = [vp, C.c_int, dp]
    L.lpx_tableau_bound_flags.argtypes = [vp, u8p]
    L.lpx_bounded_run.argtypes = [vp, C.POINTER(RunOpts), PIVOT_CB, vp, C.POINTER(Stats)]
    L.lpx_bounded_counts.argtypes = [vp, C.POINTER(C.c_int64)]
    L.lpx_tableau_bounded_solution.argtypes = [vp, C.c_int, dp, dp, u8p]
    L.lpx_solve_bounded.argtypes = [C.POINTER(Problem), dp, dp, C.POINTER(SolveOpts), C.POINTER(Result), C.POINTER(BoundedInfo)]
    L.lpx_bounded_info_free.argtypes = [C.POINTER(BoundedInfo)]
    L.lpx_bounded_info_free.restype = None
    L.lpx_tableau_bound_state.argtypes = [vp, dp, dp, u8p]
    L.lpx_tableau_change_bounds.argtypes = [vp, C.c_int, ip, dp, dp]
    L.lpx_bounded_dual_run.argtypes = [vp, C.POINTER(RunOpts), PIVOT_CB, vp, C.POINTER(Stats)]
    L.lpx_bounded_open.argtypes = [C.POINTER(Problem), dp, dp, C.POINTER(SolveOpts), C.POINTER(vp), C.POINTER(Result)]
    L.lpx_bounded_set_bounds.argtypes = [vp, C.c_int, ip, dp, dp, C.POINTER(Result)]
    L.lpx_bounded_close.argtypes = [vp]
    L.lpx_bounded_close.restype = None
    L.lpx_tableau_dualize.argtypes = [vp, C.c_double, C.POINTER(C.c_int64)]
    L.lpx_bounded_dual_run2.argtypes = [vp, C.POINTER(RunOpts), C.c_int, PIVOT_CB, vp, C.POINTER(Stats)]
    L.lpx_tableau_branch_pick.argtypes = [vp, C.c_int, u8p, C.c_double, C.POINTER(BranchPick)]
    L.lpx_bounded_node.argtypes = [vp, C.c_int, ip, dp, dp, C.POINTER(RunOpts), C.c_int, u8p, C.c_double, C.POINTER(NodeRecord)]
    L.lpx_solve_bnb_bounded.argtypes = [C.POINTER(Problem), dp, dp, u8p, C.POINTER(SolveOpts), C.c_int64, C.POINTER(Result),
                                        C.POINTER(BnbBoundedInfo)]
    L.lpx_bnb_bounded_info_free.argtypes = [C.POINTER(BnbBoundedInfo)]
    L.lpx_bnb_bounded_info_free.restype = None
    L.lpx_bounded_dual_run3.argtypes = [vp, C.POINTER(RunOpts), C.c_int, C.c_double, PIVOT_CB, vp, C.POINTER(Stats)]
    L.lpx_bounded_node2.argtypes = [vp, C.c_int, ip, dp, dp, C.POINTER(RunOpts), C.c_int, C.c_double, C.c_int, u8p, C.c_double,
                                    C.POINTER(NodeRecord)]
    L.lpx_solve_bnb_bounded2.argtypes = [C.POINTER(Problem), dp, dp, u8p, C.POINTER(SolveOpts), C.c_int64, C.c_int, C.POINTER(Result),
                                         C.POINTER(BnbBoundedInfo)]
    L.lpx_bounded_node_fits.argtypes = [C.c_int, C.c_int]
    L.lpx_bounded_node3.argtypes = [vp, C.c_int, ip, dp, dp, C.POINTER(RunOpts), C.c_int, C.c_double, C.c_int, u8p, C.c_double,
                                    C.c_int, C.POINTER(NodeRecord)]
    L.lpx_solve_bnb_bounded3.argtypes = [C.POINTER(Problem), dp, dp, u8p, C.POINTER(SolveOpts), C.c_int64, C.c_int, C.c_int,
                                         C.POINTER(Result), C.POINTER(BnbBoundedInfo)]
    L.lpx_tableau_clone.argtypes = [vp, C.POINTER(vp)]
    L.lpx_node_batch_create.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(vp)]
    L.lpx_node_batch_destroy.argtypes = [vp]
    L.lpx_node_batch_destroy.restype = None
    L.lpx_node_batch_run.argtypes = [vp, C.c_int, ip, ip, ip, dp, dp, C.POINTER(RunOpts), C.c_int, dp, C.c_int, u8p, C.c_double,
                                     C.POINTER(NodeRecord), ip]
    L.lpx_solve_bnb_bounded4.argtypes = [C.POINTER(Problem), dp, dp, u8p, C.POINTER(SolveOpts), C.c_int64, C.c_int, C.c_int,
                                         C.POINTER(Result), C.POINTER(BnbBoundedInfo), C.POINTER(BnbDiversInfo)]
    L.lpx_bnb_divers_info_free.argtypes = [C.POINTER(BnbDiversInfo)]
    L.lpx_bnb_divers_info_free.restype = None
    L.lpx_node_batch_plunge.argtypes = [vp, C.c_int, ip, ip, ip, dp, dp, C.POINTER(RunOpts), C.c_int, dp, dp, ip, C.c_int, C.c_int, u8p,
                                        C.c_double, C.POINTER(NodeRecord), ip, ip]
    L.lpx_solve_bnb_bounded5.argtypes = [C.POINTER(Problem), dp, dp, u8p, C.POINTER(SolveOpts), C.c_int64, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(Result), C.POINTER(BnbBoundedInfo), C.POINTER(BnbDiversInfo),
                                         C.POINTER(BnbPlungeInfo)]
    L.lpx_bnb_plunge_info_free.argtypes = [C.POINTER(BnbPlungeInfo)]
    L.lpx_bnb_plunge_info_free.restype = None
    L.lpx_bounded_probe.argtypes = [vp, C.POINTER(RunOpts), C.c_int, C.c_double, C.c_double, C.c_int, u8p, C.c_double, C.c_int, C.c_int,
                                    C.POINTER(ProbeHead), C.POINTER(ProbeRecord)]
    L.lpx_node_batch_run_probe.argtypes = [vp, C.c_int, ip, ip, ip, dp, dp, C.POINTER(RunOpts), C.c_int, dp, dp, C.c_int, u8p, C.c_double,
                                           C.c_int, C.c_int, C.POINTER(NodeRecord), C.POINTER(ProbeHead), C.POINTER(ProbeRecord), ip]
    L.lpx_solve_bnb_bounded6.argtypes = [C.POINTER(Problem), dp, dp, u8p, C.POINTER(SolveOpts), C.c_int64, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.POINTER(Result), C.POINTER(BnbBoundedInfo), C.POINTER(BnbDiversInfo),
                                         C.POINTER(BnbStrongInfo)]
    L.lpx_bnb_strong_info_free.argtypes = [C.POINTER(BnbStrongInfo)]
    L.lpx_bnb_strong_info_free.restype = None
    L.lpx_bounded_node4.argtypes = [vp, C.c_int, ip, dp, dp, C.POINTER(RunOpts), C.c_int, C.c_double, C.c_int, C.c_int, u8p, C.c_double,
                                    C.c_int, C.POINTER(NodeRecord), C.POINTER(GuardRecord)]
    L.lpx_node_batch_run2.argtypes = [vp, C.c_int, ip, ip, ip, dp, dp, C.POINTER(RunOpts), C.c_int, dp, C.c_int, C.c_int, u8p, C.c_double,
                                      C.POINTER(NodeRecord), C.POINTER(GuardRecord), ip]
    L.lpx_solve_bnb_bounded7.argtypes = [C.POINTER(Problem), dp, dp, u8p, C.POINTER(SolveOpts), C.c_int64, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(Result), C.POINTER(BnbBoundedInfo), C.POINTER(BnbDiversInfo),
                                         C.POINTER(BnbGuardInfo)]
    L.lpx_solve_bounded_dual.argtypes = [C.POINTER(Problem), dp, dp, C.c_int, C.POINTER(SolveOpts), C.POINTER(Result),
                                         C.POINTER(BoundedInfo)]
    L.lpx_bounded_run2.argtypes = [vp, C.POINTER(RunOpts), C.c_int, PIVOT_CB, vp, C.POINTER(Stats)]
    L.lpx_node_batch_primal.argtypes = [vp, C.c_int, ip, C.POINTER(RunOpts), C.POINTER(PrimalRecord), ip]
    L.lpx_solve_bounded2.argtypes = [C.POINTER(Problem), dp, dp, C.POINTER(SolveOpts), C.c_int, C.POINTER(Result), C.POINTER(BoundedInfo)]
    L.lpx_solve_bounded_batch.argtypes = [C.c_int, C.POINTER(C.POINTER(Problem)), C.POINTER(dp), C.POINTER(dp), C.POINTER(SolveOpts),
                                          C.POINTER(Result), C.POINTER(BoundedInfo)]
    L.lpx_packed_fits.argtypes = [C.c_int, C.c_int]
    L.lpx_solve_packed.argtypes = [C.POINTER(PackedModels), C.POINTER(RunOpts), C.POINTER(PackedResults), C.POINTER(Stats)]
    L.lpx_solve_packed_dual.argtypes = [C.POINTER(PackedDualModels), C.c_int, C.POINTER(RunOpts), C.POINTER(PackedDualResults),
                                        C.POINTER(Stats)]
    L.lpx_packed_base_open.argtypes = [C.POINTER(PackedBaseModel), C.c_int, C.POINTER(RunOpts), C.POINTER(PackedDualResults),
                                       C.POINTER(vp)]
    L.lpx_packed_base_solve.argtypes = [vp, C.c_int32, dp, C.c_int, C.POINTER(RunOpts), C.POINTER(PackedDualResults), C.POINTER(Stats)]
    L.lpx_packed_base_solve_costs.argtypes = [vp, C.c_int32, dp, dp, C.c_int, C.POINTER(RunOpts), C.POINTER(RunOpts),
                                              C.POINTER(PackedCostResults), C.POINTER(Stats)]
    L.lpx_packed_base_close.argtypes = [vp]
    L.lpx_solve_packed_bnb.argtypes = [C.POINTER(PackedBnbModels), C.POINTER(PackedBnbOpts), C.POINTER(PackedBnbResults),
                                       C.POINTER(Stats)]
    L.lpx_solve_packed_bnb_dual.argtypes = [C.POINTER(PackedBnbDualModels), C.POINTER(PackedBnbOpts), C.POINTER(PackedBnbResults),
                                            C.POINTER(Stats)]
    L.lpx_solve_bnb_bounded_dual.argtypes = [C.POINTER(Problem), dp, dp, u8p, C.POINTER(SolveOpts), C.c_int64, C.c_int, C.c_int,
                                             C.POINTER(Result), C.POINTER(BnbBoundedInfo)]
    L.lpx_solve_bnb_bounded8.argtypes =[C.POINTER(Problem), dp, dp, u8p, C.POINTER(SolveOpts), C.c_int64, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.POINTER(Result), C.POINTER(BnbBoundedInfo), C.POINTER(BnbDiversInfo),
                                         C.POINTER(BnbGuardInfo)]
    L.lpx_solve_bnb_bounded9.argtypes = [C.POINTER(Problem), dp, dp, u8p, C.POINTER(SolveOpts), C.c_int64, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.POINTER(CutOpts), C.POINTER(Result), C.POINTER(BnbBoundedInfo),
                                         C.POINTER(BnbDiversInfo), C.POINTER(BnbGuardInfo), C.POINTER(BnbCutInfo)]
    L.lpx_bnb_cut_info_free.argtypes = [C.POINTER(BnbCutInfo)]
    L.lpx_bnb_cut_info_free.restype = None
    L.lpx_bounded_node5.argtypes = [vp, C.c_int, ip, dp, dp, C.POINTER(RunOpts), C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, u8p,
                                    C.c_double, C.c_int, C.POINTER(NodeRecord), C.POINTER(GuardRecord), C.POINTER(FixList)]
    L.lpx_node_batch_run3.argtypes = [vp, C.c_int, ip, ip, ip, dp, dp, C.POINTER(RunOpts), C.c_int, dp, C.c_int, dp, C.c_int, u8p,
                                      C.c_double, C.POINTER(NodeRecord), C.POINTER(GuardRecord), C.POINTER(FixList), ip]
    L.lpx_solve_bnb_bounded10.argtypes = [C.POINTER(Problem), dp, dp, u8p, C.POINTER(SolveOpts), C.c_int64, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.POINTER(CutOpts), C.c_int, C.POINTER(Result), C.POINTER(BnbBoundedInfo),
                                          C.POINTER(BnbDiversInfo), C.POINTER(BnbGuardInfo), C.POINTER(BnbCutInfo),
                                          C.POINTER(BnbFixInfo)]
    L.lpx_parse_text.argtypes = [C.c_char_p, C.POINTER(Parsed)]
    L.lpx_parsed_free.argtypes = [C.POINTER(Parsed)]
    L.lpx_parsed_free.restype = None
    L.lpx_format_number.argtypes = [C.c_double, C.c_char_p, C.c_int]
    _lib = L
    return L


def last_error() -> str:
    buf = C.create_string_buffer(1024)
    lib().lpx_last_error(buf, 1024)
    return buf.value.decode(errors="replace")


def check(rc: int) -> int:
    """Raises LpxError for negative return codes, passes statuses through."""
    if rc < 0:
        raise LpxError(rc, last_error())
    return rc


def default_opts(dual: bool = False, **kw) -> RunOpts:
    o = RunOpts()
    lib().lpx_default_opts(C.byref(o), 1 if dual else 0)
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown run option {k!r}")
        setattr(o, k, v)
    return o


def cut_opts(**kw) -> CutOpts:
    """lpx_default_cut_opts with keyword overrides."""
    o = CutOpts()
    lib().lpx_default_cut_opts(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown cut option {k!r}")
        setattr(o, k, v)
    return o


NULL_CB = C.cast(None, PIVOT_CB)
