"""CPU checks of the NumPy restatement of the stall guard (tests/_bounded_guard_ref.py, written from include/lpx.h): without the
guard it is the existing loop bit for bit; the plain search of binary_model(40, 16, 6) by one diver ends at a node that cycles
with an exact period and a constant objective; with the guard the same search ends at the optimum scipy.optimize.milp finds; and
a search on which the guard never fires keeps its log bit for bit."""
import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bnb_divers_ref as V
import _bounded_guard_ref as G
import _bounded_long_ref as L
import _bounded_ref as B
from _node_helpers import covering_with_fixed, u64

INF = np.inf
COVERING = ((15, 48), (31, 32), (63, 190), (129, 4), (16, 47))


@pytest.mark.parametrize("flags", L.FLAG_SETS)
@pytest.mark.parametrize("m,n", COVERING)
def test_stall_zero_is_dual_run3_bit_for_bit(m, n, flags):
    T, basis, ub = covering_with_fixed(m, n, 1)
    cut = -INF
    if flags & L.CUTOFF_FLAG:                               # the objective after 10 events: the cutoff fires inside the run
        cut = float(L.dual_run3(T, basis, ub, None, L.SKIP_FIXED | (flags & L.LONG_STEP), max_iter=10)[1][-1, -1])
    want = L.dual_run3(T, basis, ub, None, L.SKIP_FIXED | flags, cut)
    got = G.dual_run4(T, basis, ub, None, L.SKIP_FIXED | flags, cut, 0)
    assert got[0] == want[0] and got[5] == want[5] and got[6] == (0, -1)
    assert got[4].tolist() == want[4].tolist() and len(want[4]) > 0
    assert np.array_equal(u64(got[1]), u64(want[1])) and got[2].tolist() == want[2].tolist() and got[3].tolist() == want[3].tolist()


def test_the_plain_search_ends_at_a_node_that_cycles():
    out, nodes, before = G.cycling_case()
    assert out["rc"] == L.ITER_LIMIT and out["nodes"] == 2850 and len(nodes) == 2850         # node 2849 is the last one
    assert out["log"]["status"][-1] == L.ITER_LIMIT and out["log"]["depth"][-1] == 15 and out["log"]["events"][-1] == 10000
    assert out["status"] == L.OPTIMAL and abs(out["value"] - 260.0) <= 1e-9 * 260.0           # the incumbent so far
    assert out["guarded_nodes"] == 0 and out["bland_events"] == 0 and out["max_events"] == 10000
    ref = V.solve_divers(*N.binary_model(*G.SMALL), np.ones(G.SMALL[0]), 1)                    # stall_events = 0 is that search
    assert ref["log"].tobytes() == out["log"].tobytes() and ref["rc"] == out["rc"]
    zs = []
    h = before.clone()
    rec = h.node4(*nodes[-1], G.SMALL[0], zs=zs)
    assert rec["status"] == L.ITER_LIMIT and rec["events"] == 10000
    tr = h.trace[2000:]                                     # past whatever leads into the cycle
    period = next(p for p in range(1, 2001) if np.array_equal(tr[p:], tr[:-p]))
    assert 2 <= period <= 2000
    z = np.array(zs[2000:])
    assert z.max() - z.min() <= 1e-9                        # the objective stands still


@pytest.mark.parametrize("S", [8, 50, 200])
def test_the_guarded_search_ends_at_the_optimum(S):
    c, A, b = N.binary_model(*G.SMALL)
    out = G.small_search(S)
    best = G.milp_value(c, A, b, np.ones(G.SMALL[0]))
    assert abs(best - 268.0) <= 1e-9 * 268.0
    assert out["rc"] == 0 and out["status"] == L.OPTIMAL and abs(out["value"] - best) <= 1e-9 * best
    assert out["max_events"] < 1000 and out["guarded_nodes"] >= 1
    if S == 50:
        assert (out["nodes"], out["guarded_nodes"], out["bland_events"], out["events"]) == (3575, 2, 10, 25900)
    # up to the first guarded node the log is the unguarded one
    plain = G.cycling_case()[0]["log"]
    assert out["log"][:2849].tobytes() == plain[:2849].tobytes()


def test_a_search_on_which_the_guard_never_fires_keeps_its_log():
    c, A0, b0 = B.binary_bounded(60, 12)[3]
    want = V.solve_divers(c, A0, b0, np.ones(60), 1)
    got = G.solve_guard(c, A0, b0, np.ones(60), 1, 50)
    assert want["rc"] == 0 and (want["nodes"], want["events"]) == (10367, 83597)
    assert got["guarded_nodes"] == 0 and got["bland_events"] == 0
    assert got["log"].tobytes() == want["log"].tobytes() and got["round"].tolist() == want["round"].tolist()
    for k in ("rc", "status", "nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K", "rounds", "steals"):
        assert got[k] == want[k], k
    assert np.array_equal(u64(got["x"]), u64(want["x"])) and got["value"] == want["value"]
