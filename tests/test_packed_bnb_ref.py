"""The NumPy restatement of the packed branch and bound (tests/_packed_bnb_ref.py) against independent answers: record for record
against _bounded_long_ref.solve2 where the new budgets do not bind (which also shows that one path array indexed by depth serves a
depth-first stack with the ceil child first), against scipy.optimize.milp at the REL of test_bnb_bounded_reference.py, and every
stop code once with its record pinned.  CPU only; tests/test_gpu_packed_bnb.py compares the device against this restatement."""
import numpy as np
import pytest

import _bounded_long_ref as L
import _packed_bnb_ref as R
from test_bnb_bounded_reference import REL, milp

SMALL = ("general", "lowers", "min", "mixed")
DEEP = 64       # the general-integer models branch on one variable more than once: deeper than max_depth = 0 (= n) allows


def _same_as_solve2(out, want):
    assert want["rc"] == 0 and out["stop"] == R.DONE and out["status"] == want["status"]
    for k in R.COUNTERS:
        assert out[k] == want[k], k
    assert out["log"].tobytes() == want["log"].tobytes() and out["logged"] == out["nodes"]
    assert out["deepest"] == want["log"]["depth"].max() and out["constant"] == want["constant"]
    if want["status"] == R.OPTIMAL:
        assert out["x"].tobytes() == want["x"].tobytes() and out["value"] == want["value"]


@pytest.mark.parametrize("flags", L.FLAG_SETS)
@pytest.mark.parametrize("n,m,seed", R.BINARY)
def test_binary_models_are_solve2_and_milp(oracle, n, m, seed, flags):
    c, A, b, upper = R.binary(n, m, seed)
    out = R.solve(c, A, b, upper, search_flags=flags)
    _same_as_solve2(out, L.solve2(c, A, b, upper, search_flags=flags))
    # the models of the GPU tests: small, yet every path of the search is taken
    print(n, m, seed, flags, "nodes", out["nodes"], "deepest", out["deepest"], "max_K", out["max_K"])
    assert 31 <= out["nodes"] <= 297 and 7 <= out["deepest"] <= 19 and 5 <= out["max_K"] <= 12
    assert out["incumbents"] >= 2 and out["pruned_bound"] > 0
    st, want = milp(c, A, np.zeros(m), b, upper)
    assert st == out["status"] == R.OPTIMAL and abs(out["value"] - want) <= REL * max(1.0, abs(want))
    x = out["x"]
    assert np.array_equal(x, np.rint(x)) and (x >= 0).all() and (x <= 1).all() and (A @ x <= b + 1e-9).all()


@pytest.mark.parametrize("flags", L.FLAG_SETS)
@pytest.mark.parametrize("name", SMALL)
def test_small_models_are_solve2_and_milp(oracle, name, flags):
    c, A, b, upper, lower, is_int, sense = R.small(name)
    out = R.solve(c, A, b, upper, lower, is_int, sense, search_flags=flags, max_depth=DEEP)
    _same_as_solve2(out, L.solve2(c, A, b, upper, lower=lower, is_int=is_int, sense=sense, search_flags=flags))
    st, want = milp(c, A, np.zeros(len(b)), b, upper, lower, is_int, sense)
    assert st == out["status"] == R.OPTIMAL and abs(out["value"] - want) <= REL * max(1.0, abs(want))
    if name != "mixed":
        assert out["deepest"] > len(c)                  # what max_depth = 0 would have stopped


def test_the_equality_pair_is_a_negative_rhs(oracle):
    """2 x1 + 2 x2 + 2 x3 = 3 as its pair of <= rows: milp finds no integer point, and the packed call never searches it -- the
    second row's right-hand side is -3, which lpx_solve_packed and so this call refuse with LPX_E_NEG_RHS.  (A model of <= rows
    whose shifted right-hand sides are >= 0 always holds its shifted origin, so the search itself cannot end INFEASIBLE; infeasible
    NODES are met in every binary model above.)"""
    c, A, b, upper, lower, is_int, sense = R.small("infeasible")
    assert A.shape == (2, 3) and b.tolist() == [3.0, -3.0]
    st, _ = milp(c, A, np.zeros(2), b, upper)
    assert st == R.INFEASIBLE
    out = R.solve(c, A, b, upper, lower, is_int, sense)
    assert (out["status"], out["stop"], out["nodes"], out["best"]) == (R.E_NEG_RHS, R.ROOT, 0, -np.inf) and not out["x"].any()


def test_refusals_in_front_of_the_root(oracle):
    c, A, b, upper = R.binary(8, 3, 1)
    for up, lo, mask in ((np.full(8, np.inf), None, None),                          # an integer variable without an upper bound
                         (np.full(8, 1.5), None, None), (upper, np.full(8, 0.5), None),      # fractional bounds
                         (np.full(8, -1.0), None, np.zeros(8, dtype=np.uint8)),     # upper < lower on a continuous variable
                         (upper, np.full(8, np.nan), None)):
        out = R.solve(c, A, b, up, lo, mask)
        assert (out["status"], out["stop"], out["nodes"]) == (R.EINVAL, R.ROOT, 0)
    # the bounds check comes in front of the sign of the shifted right-hand side, the integer check too
    assert R.solve(c, A, -b, np.full(8, 1.5))["status"] == R.EINVAL and R.solve(c, A, -b, upper)["status"] == R.E_NEG_RHS
    # a continuous variable may have any bounds: the mask takes the check away
    assert R.solve(c, A, b, np.full(8, 1.5), None, np.zeros(8, dtype=np.uint8))["status"] == R.OPTIMAL
    # an unbounded root: a continuous variable without an upper bound and no row that holds it
    A2 = A.copy(); A2[:, 0] = 0.0
    up = upper.copy(); up[0] = np.inf
    mask = np.ones(8, dtype=np.uint8); mask[0] = 0
    out = R.solve(c, A2, b, up, None, mask)
    assert (out["status"], out["stop"], out["nodes"]) == (R.UNBOUNDED, R.ROOT, 0) and out["root_events"] > 0
    out = R.solve(c, A, b, upper, max_iter=1)            # the root's own iteration limit
    assert (out["status"], out["stop"], out["root_events"]) == (R.ITER_LIMIT, R.ROOT, 1)


def test_every_stop_code_once(oracle):
    c, A, b, upper = R.binary(12, 4, 3)
    full = R.solve(c, A, b, upper)
    assert (full["status"], full["stop"], full["nodes"], full["events"], full["deepest"]) == (R.OPTIMAL, R.DONE, 75, 182, 10)

    one = R.solve(c, A, b, upper, max_nodes=1)
    assert (one["status"], one["stop"], one["nodes"], one["incumbents"], one["logged"]) == (R.ITER_LIMIT, R.NODES, 1, 0, 1)
    assert one["value"] == 0.0 and not one["x"].any() and one["best"] == -np.inf
    assert one["log"].tobytes() == full["log"][:1].tobytes()

    short = R.solve(c, A, b, upper, max_nodes=full["nodes"] - 1)
    want = L.solve2(c, A, b, upper, max_nodes=full["nodes"] - 1)
    assert want["rc"] == R.ITER_LIMIT and (short["status"], short["stop"], short["nodes"]) == (R.ITER_LIMIT, R.NODES, 74)
    assert short["log"].tobytes() == full["log"][:74].tobytes() == want["log"].tobytes()
    assert short["x"].tobytes() == want["x"].tobytes() and short["value"] == want["value"]      # the incumbent so far

    # max_events is tested in front of a pop: the search stops in front of the first node whose predecessors made max_events
    # events or more.  One below the total binds only if the last node made exactly one event; here it made more, so the search
    # ends DONE with the full record; half the total stops it
    done = np.cumsum(full["log"]["events"])
    assert full["log"]["events"][-1] == 4
    ev = R.solve(c, A, b, upper, max_events=full["events"] - 1)
    assert (ev["status"], ev["stop"], ev["nodes"], ev["events"]) == (R.OPTIMAL, R.DONE, 75, 182)
    ev = R.solve(c, A, b, upper, max_events=full["events"] - 4)
    assert (ev["status"], ev["stop"], ev["nodes"], ev["events"]) == (R.ITER_LIMIT, R.EVENTS, 74, 178)
    ev = R.solve(c, A, b, upper, max_events=91)
    k = int(np.searchsorted(done, 91)) + 1
    assert (ev["status"], ev["stop"], ev["nodes"], ev["events"]) == (R.ITER_LIMIT, R.EVENTS, k, int(done[k - 1])) and k < 74
    assert ev["events"] >= 91 and ev["log"].tobytes() == full["log"][:k].tobytes()

    exact = R.solve(c, A, b, upper, max_depth=full["deepest"])
    assert exact["stop"] == R.DONE and exact["log"].tobytes() == full["log"].tobytes()
    shallow = R.solve(c, A, b, upper, max_depth=full["deepest"] - 1)
    first = int(np.flatnonzero((full["log"]["depth"] == full["deepest"] - 1) & (full["log"]["var"] >= 0))[0])
    assert (shallow["status"], shallow["stop"], shallow["nodes"], shallow["deepest"]) == (R.ITER_LIMIT, R.DEPTH, first + 1, 9)
    assert shallow["log"].tobytes() == full["log"][:first + 1].tobytes()

    c2, A2, b2, upper2 = R.binary(16, 6, 4)             # its root makes 12 events, the busiest node 15: max_iter = 14 lets the root pass
    full2 = R.solve(c2, A2, b2, upper2)
    node = int(np.argmax(full2["log"]["events"]))
    assert (full2["root_events"], int(full2["log"]["events"][node]), node) == (12, 15, 48)
    lim = R.solve(c2, A2, b2, upper2, max_iter=14)
    assert (lim["status"], lim["stop"], lim["nodes"]) == (R.ITER_LIMIT, R.NODE_ITER, node + 1)
    assert lim["log"]["status"][-1] == R.ITER_LIMIT and lim["log"]["events"][-1] == 14
    assert lim["log"][:node].tobytes() == full2["log"][:node].tobytes() and lim["incumbents"] > 0 and lim["x"].any()

    capped = R.solve(c, A, b, upper, log_cap=10)
    assert capped["logged"] == 10 and capped["nodes"] == 75 and capped["log"].tobytes() == full["log"][:10].tobytes()


def test_solve_all_shares_what_has_no_batch_axis(oracle):
    c, A, b, upper = R.binary(8, 3, 1)
    bs = np.stack([b, b + 1.0, b - 1.0])
    outs = R.solve_all(c, A, bs, 1.0)
    assert len(outs) == 3
    for o, bi in zip(outs, bs):
        w = R.solve(c, A, bi, upper)
        assert o["log"].tobytes() == w["log"].tobytes() and o["value"] == w["value"]
