"""CPU checks of the restatement of GMI cuts on bounded handles and of cut-and-branch at the bounded root (tests/_bnb_cuts_ref.py):
the optimum against scipy.optimize.milp, the validity of every cut at every integer feasible point, the integer notion under a
fractional bound, the monotone bound of the rounds, and the search without cuts record for record."""
import functools

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bnb_cuts_ref as X
import _bnb_divers_ref as V
import _bounded_long_ref as L
import _bounded_ref as B
import _gmi_ref as G

REL = 1e-9
LONG, CUT = L.LONG_STEP, L.CUTOFF_FLAG
SMALL = sorted(N.small_models())
BINARY = [(16, 6, 1), (24, 8, 2), (32, 12, 3), (40, 16, 6)]
SETTINGS = [(2, 4), (4, 8), (8, 8)]
FLAGS = [0, LONG | CUT]


def _model(name):
    if isinstance(name, str):
        return N.small_models()[name]
    n, m, seed = name
    c, A, b = N.binary_model(n, m, seed)
    return c, A, np.zeros(m, dtype=np.int32), b, np.ones(n), None, None, 0


@functools.lru_cache(maxsize=None)
def _solve(name, rounds, K, flags, W=1, want_cuts=False):
    c, A, rel, b, upper, lower, mask, sense = _model(name)
    o = None if rounds is None else G.CutOpts(cuts_per_round=K, max_rounds=rounds)
    return X.solve_cuts(c, A, b, upper, W, o, lower=lower, is_int=mask, sense=sense, rel=rel, search_flags=flags, want_cuts=want_cuts)


@functools.lru_cache(maxsize=None)
def _milp(name):
    from scipy.optimize import Bounds, LinearConstraint, milp
    c, A, rel, b, upper, lower, mask, sense = _model(name)
    n = len(c)
    lower = np.zeros(n) if lower is None else lower
    lo = np.where(np.asarray(rel) == 2, b, -np.inf)
    sol = milp(c if sense == 1 else -c, constraints=LinearConstraint(A, lo, b), bounds=Bounds(lower, upper),
               integrality=np.ones(n) if mask is None else mask.astype(float))
    return None if sol.status != 0 else (sol.fun if sense == 1 else -sol.fun)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("rounds,K", SETTINGS)
@pytest.mark.parametrize("name", SMALL + BINARY, ids=str)
def test_optimum_is_milps(name, rounds, K, flags):
    got, want = _solve(name, rounds, K, flags), _milp(name)
    assert got["rc"] == 0 and got["cut"]["ran"] == 1
    if want is None:
        assert got["status"] == L.INFEASIBLE
        assert got["nodes"] == 0 and got["cut"]["stop"] == "infeasible" and got["cut"]["rounds"] == 1     # ends at the root
        return
    assert got["status"] == L.OPTIMAL
    assert abs(got["value"] - want) <= REL * abs(want), (got["value"], want)
    if got["cut"]["stop"] == "integral":
        assert got["nodes"] == 1 and got["incumbents"] == 1


def _integer_points(name):
    """Every integer y = x - lower in the box [0, ub'] with A' y <= b' (the prepared rows): the integer feasible points."""
    c, A, rel, b, upper, lower, mask, sense = _model(name)
    T0, _, ub0, _, _, _, _ = N.prepare(c, A, b, lower, upper, sense, rel)
    n, m = len(c), T0.shape[0] - 1
    grids = np.indices([int(u) + 1 for u in ub0[:n]]).reshape(n, -1).T.astype(np.float64)
    ok = np.all(grids @ T0[:m, :n].T <= T0[:m, -1] + 1e-9, axis=1)
    return grids[ok]


@pytest.mark.parametrize("rounds,K", SETTINGS)
@pytest.mark.parametrize("name", SMALL + [(16, 6, 1)], ids=str)
def test_every_cut_holds_at_every_integer_feasible_point(name, rounds, K):
    got = _solve(name, rounds, K, LONG | CUT, 1, True)
    cuts = got["cut"]["cuts"]
    assert len(cuts) == got["cut"]["added"] > 0
    pts = _integer_points(name)
    if name == "infeasible":
        assert len(pts) == 0
        return
    assert len(pts) > 0
    a = np.array([k[0] for k in cuts]); cst = np.array([k[1] for k in cuts])
    assert (pts @ a.T + cst).min() >= 1.0 - 1e-9


def test_flagged_column_with_a_fractional_upper_bound_gets_continuous_alphas():
    c, A, rel, b, upper, lower, mask, sense = _model("general")
    T0, basis0, ub0, _, _, _, _ = N.prepare(c, A, b, lower, upper, sense, rel)
    st, Ts, bs, flip, _, _ = B.run(T0, basis0, ub0)
    n, Cm = len(c), T0.shape[1] - 1
    flags = X.slack_mask(T0, n, mask)
    o = G.CutOpts(cuts_per_round=8)
    h = L.Handle(Ts, bs, ub0, flip)
    src, _, al = X.handle_round(h, flags, Cm, Cm, o, Ts.shape[0] + 8, Ts.shape[1] + 8)
    assert src
    r = src[0]
    f0 = Ts[r, -1] - np.floor(Ts[r, -1])
    nb = np.ones(Cm, dtype=bool); nb[bs] = False
    as_cont = G.alphas(Ts[r, :Cm], np.zeros(Cm, dtype=bool), nb, f0, o.coef_eps)
    # a flagged, nonbasic, unflipped structural column whose integer alpha in the first cut is not its continuous one
    j = next(j for j in range(n) if flags[j] and nb[j] and not flip[j] and al[0, j] != as_cont[j])
    ub = ub0.copy(); ub[j] = 2.5                            # nonbasic at zero: the tableau is as optimal as before
    eff = X.integer_columns(flags, Cm, Cm, np.zeros(Cm), ub, Cm)
    assert flags[j] and not eff[j] and eff.sum() == flags.sum() - 1
    h2 = L.Handle(Ts, bs, ub, flip)
    src2, _, al2 = X.handle_round(h2, flags, Cm, Cm, o, Ts.shape[0] + 8, Ts.shape[1] + 8)
    assert src2[0] == r and al2[0, j] == as_cont[j] != al[0, j]
    assert h2.ub[j] == 2.5 and np.all(np.isinf(h2.ub[Cm:])) and not h2.lo[Cm:].any() and not h2.flip[Cm:].any()
    lo = np.zeros(Cm); lo[j] = 0.5                          # and a fractional lower shift alike
    assert not X.integer_columns(flags, Cm, Cm, lo, ub0, Cm)[j]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("rounds,K", SETTINGS)
@pytest.mark.parametrize("name", SMALL + BINARY, ids=str)
def test_bound_does_not_rise_over_the_rounds(name, rounds, K, flags):
    cut = _solve(name, rounds, K, flags)["cut"]
    zb, za = cut["z_before"], cut["z_after"]
    assert len(zb) == len(za) == cut["rounds"] <= rounds
    assert all(a <= b for a, b in zip(za, zb))
    assert all(za[i] == zb[i + 1] for i in range(len(zb) - 1))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("name", SMALL + BINARY[:3], ids=str)
def test_without_root_cuts_it_is_the_search_by_divers(name, W, flags):
    c, A, rel, b, upper, lower, mask, sense = _model(name)
    got = _solve(name, None, 0, flags, W)
    want = V.solve_divers(c, A, b, upper, W, lower=lower, is_int=mask, sense=sense, rel=rel, search_flags=flags)
    assert got["cut"] is None
    assert got["log"].tobytes() == want["log"].tobytes()
    assert got["round"].tolist() == want["round"].tolist() and got["diver"].tolist() == want["diver"].tolist()
    for k in ("rc", "status", "nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K", "rounds",
              "steals", "largest_batch", "value"):
        assert got[k] == want[k], k
    if want["x"] is not None:
        assert np.array_equal(got["x"].view(np.uint64), want["x"].view(np.uint64))


def test_capacity_rule_and_slack_flags():
    assert X.spare(13, 73, 64) == 64 and X.spare(4, 3004, 64) == 0
    a = X.spare(100, 150, 64)
    assert 0 < a < 64 and X.node_fits(100 + a, 150 + a) and not X.node_fits(101 + a, 151 + a)
    # an = row is two prepared rows, judged alike; a fractional coefficient, a fractional RHS or a continuous variable in the row
    # makes its slack continuous
    T0 = N.prepare(np.ones(3), np.array([[2.0, 2.0, 2.0], [1.0, 0.5, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 0.0]]),
                   np.array([3.0, 2.0, 2.5, 1.0]), None, np.ones(3), 0, np.array([2, 0, 0, 0]))[0]
    assert X.slack_mask(T0, 3, None).tolist() == [1, 1, 1, 1, 1, 0, 0, 1]
    assert X.slack_mask(T0, 3, np.array([1, 0, 1], dtype=np.uint8)).tolist() == [1, 0, 1, 0, 0, 0, 0, 0]
