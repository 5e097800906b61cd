"""CPU checks of the restatement of the plunge (tests/_bnb_plunge_ref.py, the rule of lpx_solve_bnb_bounded5): plunge = 1 is the
search by W divers record for record, one diver with any plunge is the sequential driver, every (W, D) reaches the optimum, and
the instances the GPU tests use are not vacuous: they hold chains of three and more nodes, chains that end at their cap, and
records dropped because the incumbent moved inside a round."""
import functools

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bnb_divers_ref as V
import _bnb_plunge_ref as P
import _bounded_long_ref as L

REL = 1e-9
LONG, CUT = L.LONG_STEP, L.CUTOFF_FLAG
MODELS = [(16, 8, 1), (32, 16, 2)]          # the instances of the GPU driver tests
KEYS = ("rc", "status", "nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K")


@functools.lru_cache(maxsize=None)
def _plunge(n, m, seed, W, D, flags=0, max_nodes=0):
    c, A, b = N.binary_model(n, m, seed)
    return P.solve_plunge(c, A, b, np.ones(n), W, D, search_flags=flags, max_nodes=max_nodes)


@functools.lru_cache(maxsize=None)
def _divers(n, m, seed, W, flags=0):
    c, A, b = N.binary_model(n, m, seed)
    return V.solve_divers(c, A, b, np.ones(n), W, search_flags=flags)


@functools.lru_cache(maxsize=None)
def _sequential(n, m, seed, flags=0):
    c, A, b = N.binary_model(n, m, seed)
    return L.solve2(c, A, b, np.ones(n), search_flags=flags)


def _same(got, want, keys=KEYS):
    assert got["log"].tobytes() == want["log"].tobytes()
    for k in keys:
        assert got[k] == want[k], k
    assert np.array_equal(got["x"].view(np.uint64), want["x"].view(np.uint64))
    assert np.float64(got["value"]).view(np.uint64) == np.float64(want["value"]).view(np.uint64)


@pytest.mark.parametrize("flags", [0, LONG | CUT])
@pytest.mark.parametrize("W", [1, 2, 8, 64])
@pytest.mark.parametrize("n,m,seed", MODELS)
def test_plunge_of_one_is_the_search_by_divers(n, m, seed, W, flags):
    got, want = _plunge(n, m, seed, W, 1, flags), _divers(n, m, seed, W, flags)
    _same(got, want, KEYS + ("rounds", "steals", "largest_batch"))
    assert got["round"].tolist() == want["round"].tolist() and got["diver"].tolist() == want["diver"].tolist()
    assert not got["step"].any() and got["dropped"] == 0 and got["launched"] == got["nodes"] and got["longest_chain"] == 1


@pytest.mark.parametrize("flags", [0, LONG | CUT])
@pytest.mark.parametrize("D", [2, 5, 64])
@pytest.mark.parametrize("n,m,seed", MODELS)
def test_one_diver_is_the_sequential_driver(n, m, seed, D, flags):
    got, want = _plunge(n, m, seed, 1, D, flags), _sequential(n, m, seed, flags)
    _same(got, want)
    assert got["dropped"] == 0 and got["launched"] == got["nodes"] and got["rounds"] < got["nodes"]
    assert 3 <= got["longest_chain"] <= D or D == 2 and got["longest_chain"] == 2
    # a record's step counts up inside its round
    for r in np.unique(got["round"])[:50]:
        s = got["step"][got["round"] == r]
        assert s.tolist() == list(range(len(s)))


@pytest.mark.parametrize("flags", [0, LONG | CUT])
@pytest.mark.parametrize("W,D", [(2, 2), (8, 8), (64, 2), (8, 64), (64, 64)])
@pytest.mark.parametrize("n,m,seed", MODELS)
def test_every_width_and_depth_reaches_the_optimum(n, m, seed, W, D, flags):
    got, want = _plunge(n, m, seed, W, D, flags), _sequential(n, m, seed, flags)
    assert got["rc"] == 0 and got["status"] == want["status"] == L.OPTIMAL
    assert abs(got["value"] - want["value"]) <= REL * abs(want["value"])
    assert got["launched"] == got["nodes"] + got["dropped"] and got["longest_chain"] <= D and got["largest_batch"] <= W
    # every round names each diver's chain once, divers ascending, steps counting up
    for r in np.unique(got["round"])[:50]:
        sel = got["round"] == r
        d, s = got["diver"][sel], got["step"][sel]
        assert np.all(np.diff(d) >= 0)
        for k in np.unique(d):
            assert s[d == k].tolist() == list(range(int((d == k).sum())))


def test_optimum_agrees_with_scipy():
    milp = pytest.importorskip("scipy.optimize").milp
    from scipy.optimize import Bounds, LinearConstraint
    for n, m, seed in MODELS:
        c, A, b = N.binary_model(n, m, seed)
        ref = milp(-np.asarray(c), constraints=LinearConstraint(A, -np.inf, b), integrality=np.ones(n), bounds=Bounds(0, 1))
        assert ref.success
        for W, D in ((1, 64), (8, 8)):
            got = _plunge(n, m, seed, W, D, LONG | CUT)
            assert abs(got["value"] + ref.fun) <= 1e-6 * max(1.0, abs(ref.fun))


def test_the_gpu_instances_are_not_vacuous():
    """Chains of three and more, chains at their cap, dropped records, and no refusal inside a chain (the restatement raises
    on one): what the GPU driver tests rely on."""
    seen_dropped = False
    for n, m, seed in MODELS:
        for flags in (0, LONG | CUT):
            for W in (1, 2, 8, 64):
                for D in (2, 8, 64):
                    got = _plunge(n, m, seed, W, D, flags)
                    written = [c[2] for c in got["chains"]]
                    assert max(written) >= min(D, 3), (n, W, D)
                    if D == 2 or (n == 32 and D == 8):          # binary_model(16, 8, 1) has no chain longer than 7
                        assert any(c[2] == c[4] for c in got["chains"]), "no chain ends at its cap"
                    assert got["refusals"] == 0
                    seen_dropped = seen_dropped or got["dropped"] > 0
                    if W == 1:
                        assert got["dropped"] == 0
    assert seen_dropped
    assert _plunge(16, 8, 1, 8, 8)["dropped"] > 0 or _plunge(32, 16, 2, 8, 8)["dropped"] > 0


def test_node_limit_cuts_a_round_short():
    n, m, seed, W, D = 16, 8, 1, 8, 4
    full = _plunge(n, m, seed, W, D)
    limit = int(np.flatnonzero(full["round"] == 3)[2]) + 1          # inside round 3
    got = _plunge(n, m, seed, W, D, 0, limit)
    assert got["rc"] == L.ITER_LIMIT and got["nodes"] == limit
    # A cap is what the limit leaves after the caps handed out before it, whether or not those chains use theirs: a round can
    # end short of the limit, and the search then goes on with smaller caps.  No round may be able to overshoot.
    before = 0
    for r in range(got["rounds"]):
        caps = [c[4] for c in got["chains"] if c[0] == r]
        assert sum(caps) <= limit - before and max(caps) <= D
        before += sum(c[3] for c in got["chains"] if c[0] == r)
    assert before == limit and any(c[4] < D for c in got["chains"])
    first = int((full["round"] == 0).sum())                     # the first round holds one chain: the limit does not reach it
    assert got["log"][:first].tobytes() == full["log"][:first].tobytes()
