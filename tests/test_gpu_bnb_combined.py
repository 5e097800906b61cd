"""GPU tests of the driver lpx_solve_bnb_bounded10 with its switches combined, through LPSolver.SolveBnbBounded: root cuts, the
on-chip root solve on a handle with spare capacity, the stall guard and reduced-cost tightening in one search, bit for bit against
the composed restatement (tests/_bnb_combined_ref.py, itself pinned to scipy.optimize.milp and to the restatements of the single
switches by tests/test_bnb_combined_reference.py): node log, round and diver of every record, every counter, the cut loop's
record, solution and value bits.  Also: the root form changes nothing of a search with root cuts; tighten = 0 with root cuts is
lpx_solve_bnb_bounded9 through the C ABI; and a shape with no spare capacity runs no round and still tightens.

What the searches of the first test do (the restatement's counts, which the device equals bit for bit; cuts added, then tightened
nodes / tightened columns / Bland events for W = 1 and W = 4, flags 0 | LONG + CUTOFF; Bland events are those at S = 1, none at 0):
  ip(24, 6)    30 cuts   65/260/3 | 65/260/1       67/398/12 | 66/387/5        (S = 0 tightens the same columns)
  ip(32, 8)    32 cuts   234/806/49 | 235/804/15   282/1397/58 | 283/1405/12   (S = 0: 233/805 | 233/803, 282/1396 | 283/1407)
  bm(24, 8, 2) 32 cuts   70/275/5 | 72/282/5       87/391/9 | 87/390/7         (S = 0: 70/275 | 70/274, 87/391 | 87/390)
  general       5 cuts   32/83/7 | 32/83/0         31/84/4 | 31/84/0
  lowers        5 cuts   32/83/7 | 32/83/0         31/84/4 | 31/84/0"""
import ctypes as C

import numpy as np
import pytest

import _bnb_combined_ref as CB
import _bounded_long_ref as L
import _bnb_cuts_ref as X
from _node_helpers import bits as _bits, u64 as _u64
from test_gpu_bnb_cuts import _same_cuts
from test_gpu_bnb_tighten import _same_solve

pytestmark = pytest.mark.gpu

LONG, CUT = L.LONG_STEP, L.CUTOFF_FLAG
MODELS = [("ip", 24, 6), ("ip", 32, 8), ("bm", 24, 8, 2), "general", "lowers"]
FORMS = [("launches", 0), ("onchip", 0), ("onchip", 1)]


def _problem(gpu, name):
    c, A, rel, b, upper, lower, mask, sense = CB.model(name)
    return gpu.LPProblem.from_arrays(sense, c, A, rel, b), dict(upper=upper, lower=lower, integer=mask)


def _solve(gpu, name, **kw):
    prob, bounds = _problem(gpu, name)
    try:
        return gpu.LPSolver().SolveBnbBounded(prob, **bounds, **kw), 0
    except gpu.SolverException as e:
        if getattr(e, "result", None) is None:
            raise
        return e.result, e.code


# ---- 1. bit for bit against the composed restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("F,S", FORMS)
@pytest.mark.parametrize("flags", [0, LONG | CUT])
@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("name", MODELS, ids=str)
def test_the_combined_driver_bit_for_bit(gpu, name, W, flags, F, S):
    want = CB.search(name, W, flags, S)
    assert want["nodes"] < 1500
    res, rc = _solve(gpu, name, tighten=True, root_cuts=4, cuts_per_round=8, root_form=F, stall_events=S, divers=W,
                     long_step=bool(flags & LONG), cutoff=bool(flags & CUT))
    bi = res.BnbInfo
    print(name, "W", W, "flags", flags, F, "S", S, "nodes", res.Nodes, "cuts added", bi["cuts_added"], bi["cut_stop"], "shape", bi["cut_R"],
          bi["cut_C"], "tightened nodes", bi["tightened_nodes"], "cols", bi["tightened_cols"], "Bland events", bi["bland_events"])
    _same_solve(res, rc, want)
    assert res.BnbLog.tobytes() == want["log"].tobytes()
    _same_cuts(res, want["cut"])
    assert want["cut"]["ran"] == 1 and bi["cuts_added"] >= 1 and bi["tightened_nodes"] >= 1
    assert bi["cut_spare"] > 0
    if S == 1 and CB.is_binary(name):
        assert bi["bland_events"] >= 1 and bi["guarded_nodes"] >= 1
    if S == 0:
        assert bi["bland_events"] == 0


# ---- 2. the root form, with spare capacity on the root's handle -----------------------------------------------------------------
@pytest.mark.parametrize("tighten", [False, True])
@pytest.mark.parametrize("name", [("ip", 24, 6), ("bm", 40, 16, 6)], ids=str)
def test_the_root_form_changes_nothing_of_a_search_with_root_cuts(gpu, name, tighten):
    kw = dict(divers=4, root_cuts=4, cuts_per_round=8, long_step=True, cutoff=True, tighten=tighten)
    want, wrc = _solve(gpu, name, root_form="launches", **kw)
    assert wrc == 0 and len(want.BnbLog) > 1 and want.BnbInfo["cut_ran"] == 1 and want.BnbInfo["cut_spare"] > 0
    assert want.BnbInfo["cuts_added"] >= 1
    ref = CB.search(name, 4, LONG | CUT, 0, tighten_on=tighten)
    assert want.BnbLog.tobytes() == ref["log"].tobytes()
    for form in ("onchip", "auto"):
        got, grc = _solve(gpu, name, root_form=form, **kw)
        assert grc == 0 and got.BnbLog.tobytes() == want.BnbLog.tobytes(), form
        assert got.BnbRound.tolist() == want.BnbRound.tolist() and got.BnbDiver.tolist() == want.BnbDiver.tolist()
        assert got.BnbInfo == want.BnbInfo, form
        assert np.array_equal(_u64(got.CutZ), _u64(want.CutZ)) and len(got.CutZ) == want.BnbInfo["cut_rounds"] >= 1
        assert got.Status == want.Status and _bits(got.OptimalValue) == _bits(want.OptimalValue)
        assert np.array_equal(_u64(got.Solution), _u64(want.Solution))


# ---- 3. tighten = 0 with root cuts is lpx_solve_bnb_bounded9, through the C ABI -------------------------------------------------
@pytest.mark.parametrize("root_form", ["launches", "onchip"])
@pytest.mark.parametrize("W", [1, 4])
def test_tighten_zero_with_root_cuts_is_bounded9_byte_for_byte(gpu, W, root_form):
    from linear_programming_solver_lpr381_amd.solver import _problem_struct
    lib, _lib = gpu._lib.lib(), gpu._lib
    prob, bounds = _problem(gpu, ("ip", 24, 6))
    n = prob.NumVars
    ps, hold = _problem_struct(prob)
    up = np.ascontiguousarray(bounds["upper"], dtype=np.float64)
    upp = up.ctypes.data_as(_lib.dp)
    co = gpu.CutOpts(cuts_per_round=8, max_rounds=4).to_c()
    form = _lib.NODE_FORMS[root_form]
    seen = []
    for entry in (9, 10):
        r, info, dinfo, ginfo = _lib.Result(), _lib.BnbBoundedInfo(), _lib.BnbDiversInfo(), _lib.BnbGuardInfo()
        cinfo, finfo = _lib.BnbCutInfo(), _lib.BnbFixInfo(9, 9, 9)
        if entry == 9:
            rc = lib.lpx_solve_bnb_bounded9(C.byref(ps), None, upp, None, None, 0, LONG | CUT, W, 1, form, C.byref(co), C.byref(r),
                                            C.byref(info), C.byref(dinfo), C.byref(ginfo), C.byref(cinfo))
        else:
            rc = lib.lpx_solve_bnb_bounded10(C.byref(ps), None, upp, None, None, 0, LONG | CUT, W, 1, form, C.byref(co), 0, C.byref(r),
                                             C.byref(info), C.byref(dinfo), C.byref(ginfo), C.byref(cinfo), C.byref(finfo))
            assert (finfo.tightened_nodes, finfo.tightened_cols, finfo.max_per_node) == (0, 0, 0)
        try:
            assert rc == 0 and info.n_log >= 1 and cinfo.ran == 1 and cinfo.added >= 1 and cinfo.n_z == cinfo.rounds >= 1
            k = info.n_log
            seen.append((C.string_at(info.log, k * C.sizeof(_lib.BnbNodeLog)),
                         [int(getattr(info, f)) for f in ("nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K")],
                         [int(dinfo.rounds), int(dinfo.steals), int(dinfo.largest_batch)],
                         np.ctypeslib.as_array(dinfo.round, (k,)).tolist(), np.ctypeslib.as_array(dinfo.diver, (k,)).tolist(),
                         [int(ginfo.guarded_nodes), int(ginfo.bland_events), int(ginfo.max_events)],
                         [int(getattr(cinfo, f)) for f in ("ran", "spare", "rounds", "added", "purged", "stop", "status", "R", "C", "n_z", "events")],
                         _u64(np.ctypeslib.as_array(cinfo.z_before, (cinfo.n_z,))).tolist(),
                         _u64(np.ctypeslib.as_array(cinfo.z_after, (cinfo.n_z,))).tolist(),
                         int(r.status), int(_bits(r.optimal_value)), _u64(np.ctypeslib.as_array(r.x, (n,))).tolist()))
        finally:
            lib.lpx_bnb_bounded_info_free(C.byref(info)); lib.lpx_bnb_divers_info_free(C.byref(dinfo))
            lib.lpx_bnb_cut_info_free(C.byref(cinfo)); lib.lpx_result_free(C.byref(r))
    assert seen[0] == seen[1]
    want = CB.search(("ip", 24, 6), W, LONG | CUT, 1, tighten_on=False)
    assert seen[1][0] == want["log"].tobytes() and seen[1][5][1] == want["bland_events"]


# ---- 4. no spare capacity: no round, tightening switched on ---------------------------------------------------------------------
def test_a_shape_that_just_fits_runs_no_round_with_tightening_on(gpu):
    """4 x 3004 fits the on-chip node and 5 x 3005 does not: a = 0, no round, the first 24 nodes of the search with tighten = 1
    (they find no incumbent, so every fix_bound is still -inf: the log is that of the search without cuts and tightening)."""
    name = ("bm", 3000, 3, 1)
    assert X.node_fits(4, 3004) and not X.node_fits(5, 3005)
    want = CB.search(name, 4, LONG | CUT, 0, max_nodes=24)
    assert want["cut"] == {"spare": 0, "ran": 0} and len(want["log"]) > 0
    res, rc = _solve(gpu, name, tighten=True, root_cuts=4, divers=4, long_step=True, cutoff=True, max_nodes=24)
    assert rc == (gpu._lib.ITER_LIMIT if want["rc"] == L.ITER_LIMIT else 0)
    assert res.BnbLog.tobytes() == want["log"].tobytes()
    assert res.BnbRound.tolist() == want["round"].tolist() and res.BnbDiver.tolist() == want["diver"].tolist()
    for k in ("nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K", "rounds", "steals", "largest_batch",
              "guarded_nodes", "bland_events", "max_events", "tightened_nodes", "tightened_cols", "max_per_node"):
        assert res.BnbInfo[k] == want[k], k
    print("nodes", res.Nodes, "tightened nodes", res.BnbInfo["tightened_nodes"], "cols", res.BnbInfo["tightened_cols"])
    _same_cuts(res, want["cut"])
