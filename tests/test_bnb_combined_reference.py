"""The NumPy restatement of lpx_solve_bnb_bounded10 with its switches combined (tests/_bnb_combined_ref.py) against independent
answers: with a switch off it is, byte for byte, the restatement that never had the switch (_bnb_tighten_ref.solve_tighten without
root cuts, _bnb_cuts_ref.solve_cuts without tightening and guard, _bnb_divers_ref.solve_divers without all three); with root
cuts, tightening and the stall guard together it reaches the optimum of scipy.optimize.milp on 0/1 and general-integer models
under both flag sets, W = 1 and 4, S = 0 and 1, with the cuts, the tightened columns and the Bland events asserted to be there;
and on every tightened node of a search on cut handles a twin that takes the reported triples as an edit makes no event and no
flip and ends in the same state.  CPU only; the GPU tests compare the device against this restatement bit for bit."""
import numpy as np
import pytest

import _bnb_combined_ref as CB
import _bnb_cuts_ref as X
import _bnb_divers_ref as DV
import _bnb_tighten_ref as R
import _bounded_long_ref as L
import _gmi_ref as G
from test_bnb_bounded_reference import milp

REL = 1e-9
LONG, CUT = L.LONG_STEP, L.CUTOFF_FLAG
MODELS = [("ip", 24, 6), ("ip", 32, 8), ("bm", 24, 8, 2), ("bm", 40, 16, 6), "general", "lowers", "min"]
COUNTERS = ("rc", "status", "nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K", "rounds", "steals",
            "largest_batch")
GUARD = ("guarded_nodes", "bland_events", "max_events")
FIX = ("tightened_nodes", "tightened_cols", "max_per_node")


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, keys):
    assert got["log"].tobytes() == want["log"].tobytes(), "node log differs"
    assert got["round"].tolist() == want["round"].tolist() and got["diver"].tolist() == want["diver"].tolist()
    for k in keys:
        assert got[k] == want[k], k
    assert _u64(got["x"]).tolist() == _u64(want["x"]).tolist() and _u64(got["value"]).tolist() == _u64(want["value"]).tolist()


def _same_cut(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        if k in ("z_before", "z_after"):
            assert _u64(got[k]).tolist() == _u64(want[k]).tolist(), k
        elif k == "traces":
            assert [t.tolist() for t in got[k]] == [t.tolist() for t in want[k]]
        elif k in ("x_var", "z"):
            assert _u64(got[k]) == _u64(want[k]), k
        else:
            assert got[k] == want[k], k


def _kw(name):
    c, A, rel, b, upper, lower, is_int, sense = CB.model(name)
    return (c, A, b, upper), dict(lower=lower, is_int=is_int, sense=sense, rel=rel)


# ---- 1. the reductions, byte for byte ------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 1])
@pytest.mark.parametrize("W,flags", [(1, 0), (4, LONG | CUT)])
@pytest.mark.parametrize("name", [("ip", 24, 6), ("bm", 24, 8, 2), "lowers"], ids=str)
def test_without_root_cuts_it_is_the_tightening_search(oracle, name, W, flags, S):
    args, kw = _kw(name)
    got = CB.solve_combined(*args, W, None, S, True, flags, **kw)
    want = R.solve_tighten(*args, W, S, search_flags=flags, **kw)
    _same(got, want, COUNTERS + GUARD + FIX)
    assert got["cut"] is None and got["tightened_cols"] >= 1


@pytest.mark.parametrize("W,flags", [(1, 0), (4, LONG | CUT)])
@pytest.mark.parametrize("name", [("ip", 24, 6), ("bm", 24, 8, 2), "lowers", "min"], ids=str)
def test_without_tightening_and_guard_it_is_the_search_with_root_cuts(oracle, name, W, flags):
    args, kw = _kw(name)
    o = G.CutOpts(cuts_per_round=8, max_rounds=4)
    got = CB.solve_combined(*args, W, o, 0, False, flags, **kw)
    want = X.solve_cuts(*args, W, o, search_flags=flags, **kw)
    _same(got, want, COUNTERS)
    _same_cut(got["cut"], want["cut"])
    assert got["cut"]["added"] >= 1 and got["tightened_nodes"] == got["bland_events"] == 0


def test_a_root_the_cuts_make_infeasible_ends_as_the_search_with_root_cuts_does(oracle):
    args, kw = _kw("infeasible")
    o = G.CutOpts(cuts_per_round=8, max_rounds=4)
    got = CB.solve_combined(*args, 4, o, 1, True, LONG | CUT, **kw)
    want = X.solve_cuts(*args, 4, o, search_flags=LONG | CUT, **kw)
    assert got["cut"]["stop"] == want["cut"]["stop"] == "infeasible"
    assert (got["rc"], got["status"], got["nodes"], len(got["log"])) == (want["rc"], want["status"], 0, 0) and got["x"] is None


@pytest.mark.parametrize("W,flags", [(1, 0), (4, LONG | CUT)])
@pytest.mark.parametrize("name", [("ip", 24, 6), ("bm", 24, 8, 2), "lowers"], ids=str)
def test_with_everything_off_it_is_the_search_by_divers(oracle, name, W, flags):
    args, kw = _kw(name)
    got = CB.solve_combined(*args, W, None, 0, False, flags, **kw)
    want = DV.solve_divers(*args, W, search_flags=flags, **kw)
    _same(got, want, COUNTERS)
    assert got["cut"] is None and got["tightened_nodes"] == got["bland_events"] == 0


# ---- 2. the optimum of milp, and that every switch did something ----------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 1])
@pytest.mark.parametrize("flags", [0, LONG | CUT])
@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("name", MODELS, ids=str)
def test_cuts_tightening_and_guard_together_reach_the_optimum_of_milp(oracle, name, W, flags, S):
    c, A, rel, b, upper, lower, is_int, sense = CB.model(name)
    out = CB.search(name, W, flags, S)
    st, want = milp(c, A, rel, b, upper, lower, is_int, sense)
    cut = out["cut"]
    print(name, "W", W, "flags", flags, "S", S, "nodes", out["nodes"], "cuts", cut["added"], cut["stop"], "tightened nodes",
          out["tightened_nodes"], "cols", out["tightened_cols"], "bland events", out["bland_events"], "optimum", out["value"], want)
    assert out["rc"] == 0 and out["status"] == st == L.OPTIMAL and out["nodes"] < 1500
    assert abs(out["value"] - want) <= REL * max(1.0, abs(want))
    x = out["x"]
    lo = np.zeros(len(c)) if lower is None else lower
    assert np.array_equal(x, np.rint(x)) and (x >= lo).all() and (x <= upper).all() and (A @ x <= b + 1e-9).all()
    assert abs(float(c @ x) - want) <= REL * max(1.0, abs(want))
    assert cut["ran"] == 1 and cut["added"] >= 1
    if CB.is_binary(name):
        assert out["tightened_cols"] >= out["tightened_nodes"] >= 1
        if S == 1:
            assert out["bland_events"] >= 1 and out["guarded_nodes"] >= 1
    if S == 0:
        assert out["bland_events"] == 0
    if name == "min":                                         # the cuts close the search: nothing is left to tighten
        assert cut["stop"] == "integral" and out["nodes"] == 1 and out["tightened_cols"] == 0


# ---- 3. the defining property of tightening, on handles with cut rows -----------------------------------------------------------
@pytest.mark.parametrize("W,flags,S", [(1, 0, 0), (4, LONG | CUT, 1)])
def test_a_twin_that_takes_the_triples_as_an_edit_makes_no_event_on_cut_handles(oracle, W, flags, S):
    name = ("ip", 24, 6)
    args, kw = _kw(name)
    n = 24
    twins, seen = {}, {"checked": 0, "basic_slack": 0, "ld": None}

    def on_node(index, d, h, cols, lo, up, cutoff, fix_bound):
        twins[index] = (h.clone(), cols.copy(), lo.copy(), up.copy(), cutoff)

    def on_done(index, d, h, rec):
        twin, cols, lo, up, cutoff = twins.pop(index)
        fc, fl, fu = rec["fixed"]
        if not len(fc):
            return
        first = twin.node4(cols, lo, up, n, None, R.EPS, R.SKIP_FIXED | flags, cutoff, S)
        assert first["status"] == rec["status"] == L.OPTIMAL and _u64(first["z"]) == _u64(rec["z"])
        assert (first["bland_events"], first["first_bland"]) == (rec["bland_events"], rec["first_bland"])
        assert fc.tolist() == sorted(set(fc.tolist())) and fc.max() < n
        second = twin.node4(fc, fl, fu, n, None, R.EPS, R.SKIP_FIXED | flags, cutoff, S)
        assert (second["status"], second["events"], second["flips"]) == (L.OPTIMAL, 0, 0), second
        assert np.array_equal(_u64(twin.ub), _u64(h.ub)) and np.array_equal(_u64(twin.lo), _u64(h.lo))
        assert np.array_equal(_u64(twin.T), _u64(h.T)) and twin.basis.tolist() == h.basis.tolist()
        assert twin.flip.tolist() == h.flip.tolist()
        assert np.isinf(h.ub[n:]).all(), "a slack column was given a bound"
        seen["checked"] += 1
        seen["basic_slack"] += bool((h.basis >= n).any())
        seen["ld"] = h.T.shape

    o = G.CutOpts(cuts_per_round=8, max_rounds=4)
    out = CB.solve_combined(*args, W, o, S, True, flags, on_node=on_node, on_done=on_done, **kw)
    print("tightened nodes", out["tightened_nodes"], "with a basic column >= nint", seen["basic_slack"], "shape", seen["ld"])
    assert out["rc"] == 0 and seen["checked"] == out["tightened_nodes"] >= 1
    assert out["cut"]["added"] >= 1 and seen["ld"] == (out["cut"]["R"], out["cut"]["C"]) and seen["ld"][0] > 7
    assert seen["basic_slack"] >= 1, "no tightened node had a basic column at or above nint"
