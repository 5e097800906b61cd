"""CPU checks of the restatement of the search by W divers (tests/_bnb_divers_ref.py, the rule of lpx_solve_bnb_bounded4): one
diver is the sequential driver record for record, the rule is deterministic, every W reaches the sequential optimum, and the
node and round counts are those the rule gives when it is read as include/lpx.h states it."""
import functools

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bnb_divers_ref as V
import _bounded_long_ref as L

REL = 1e-9
LONG, CUT = L.LONG_STEP, L.CUTOFF_FLAG


@functools.lru_cache(maxsize=None)
def _divers(n, m, seed, W, flags=0):
    c, A, b = N.binary_model(n, m, seed)
    return V.solve_divers(c, A, b, np.ones(n), W, search_flags=flags)


@functools.lru_cache(maxsize=None)
def _sequential(n, m, seed, flags=0):
    c, A, b = N.binary_model(n, m, seed)
    return L.solve2(c, A, b, np.ones(n), search_flags=flags)


@pytest.mark.parametrize("flags", [0, LONG | CUT])
@pytest.mark.parametrize("n,m,seed", [(16, 8, 1), (32, 16, 2)])
def test_one_diver_is_the_sequential_driver(n, m, seed, flags):
    got, want = _divers(n, m, seed, 1, flags), _sequential(n, m, seed, flags)
    assert got["log"].tobytes() == want["log"].tobytes() and len(got["log"]) == want["nodes"] > 100
    for k in ("rc", "status", "nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K"):
        assert got[k] == want[k], k
    assert np.array_equal(got["x"].view(np.uint64), want["x"].view(np.uint64))
    assert np.float64(got["value"]).view(np.uint64) == np.float64(want["value"]).view(np.uint64)
    assert got["rounds"] == got["nodes"] and got["steals"] == 0 and got["largest_batch"] == 1
    assert got["round"].tolist() == list(range(got["nodes"])) and not got["diver"].any()


def test_two_runs_give_identical_logs():
    c, A, b = N.binary_model(16, 8, 1)
    a = V.solve_divers(c, A, b, np.ones(16), 8, search_flags=LONG | CUT)
    again = V.solve_divers(c, A, b, np.ones(16), 8, search_flags=LONG | CUT)
    assert a["log"].tobytes() == again["log"].tobytes()
    assert a["round"].tolist() == again["round"].tolist() and a["diver"].tolist() == again["diver"].tolist()
    assert np.array_equal(a["x"].view(np.uint64), again["x"].view(np.uint64))


@pytest.mark.parametrize("flags", [0, LONG | CUT])
@pytest.mark.parametrize("W", [2, 8, 64])
@pytest.mark.parametrize("n,m,seed", [(16, 8, 1), (32, 16, 2)])
def test_every_width_reaches_the_sequential_optimum(n, m, seed, W, flags):
    got, want = _divers(n, m, seed, W, flags), _sequential(n, m, seed, flags)
    assert got["rc"] == 0 and got["status"] == want["status"] == L.OPTIMAL
    assert abs(got["value"] - want["value"]) <= REL * abs(want["value"])
    assert got["largest_batch"] <= W and got["rounds"] < got["nodes"]
    # every round names each diver at most once, in ascending order
    for r in np.unique(got["round"]):
        d = got["diver"][got["round"] == r]
        assert np.all(np.diff(d) > 0)


# model, flags, W: nodes, events, rounds, sum over the rounds of the largest event count
COUNTS = {
    ((12, 6, 1), 0, 1): (25, None, 25, None),
    ((12, 6, 1), 0, 3): (23, None, 9, None),
    ((12, 6, 1), 0, 8): (17, None, 5, None),
    ((16, 8, 1), 0, 8): (387, 1212, 51, 334),
    ((16, 8, 1), 0, 64): (61, 199, 6, 27),
    ((32, 16, 2), 0, 8): (2559, 17080, 327, 4518),
    ((32, 16, 2), 0, 64): (4797, 32292, 85, 1656),
    ((32, 16, 2), LONG | CUT, 8): (2573, 12527, 328, 4222),
    ((32, 16, 2), LONG | CUT, 64): (4803, 23139, 88, 1787),
    ((40, 20, 1), 0, 8): (1659, 10441, 211, 3034),
    ((40, 20, 1), 0, 64): (2483, 17085, 47, 930),
}
# model, flags: nodes, events of the sequential driver (the first column of the same table)
SEQUENTIAL = {((16, 8, 1), 0): (197, 630), ((32, 16, 2), 0): (1995, 13454), ((32, 16, 2), LONG | CUT): (1987, 9829),
              ((40, 20, 1), 0): (1993, 12023)}


@pytest.mark.parametrize("model,flags,W", sorted(COUNTS))
def test_counts_of_the_rule(model, flags, W):
    nodes, events, rounds, critical = COUNTS[(model, flags, W)]
    got = _divers(*model, W, flags)
    assert (got["nodes"], got["rounds"]) == (nodes, rounds)
    if events is not None:
        assert (got["events"], got["critical_events"]) == (events, critical)


@pytest.mark.parametrize("model,flags", sorted(SEQUENTIAL))
def test_sequential_counts_of_the_table(model, flags):
    want = _sequential(*model, flags)
    assert (want["nodes"], want["events"]) == SEQUENTIAL[(model, flags)]
    one = _divers(*model, 1, flags)                          # and one diver counts the same
    assert (one["nodes"], one["events"], one["rounds"]) == (want["nodes"], want["events"], want["nodes"])


def test_node_limit_cuts_a_round_short():
    c, A, b = N.binary_model(16, 8, 1)
    full = _divers(16, 8, 1, 8)
    limit = int(np.flatnonzero(full["round"] == 5)[1]) + 1          # inside round 5
    got = V.solve_divers(c, A, b, np.ones(16), 8, max_nodes=limit)
    assert got["rc"] == L.ITER_LIMIT and got["nodes"] == limit
    assert got["log"].tobytes() == full["log"][:limit].tobytes()
    assert got["round"].tolist() == full["round"][:limit].tolist() and got["diver"].tolist() == full["diver"][:limit].tolist()
