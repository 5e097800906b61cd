"""The NumPy restatement of the long-step ratio test, the objective cutoff and the dual start (tests/_bounded_long_ref.py)
against independent answers: flags without the new bits against the restatement of lpx_bounded_dual_run2 bit for bit; the dual
start on covering models against HiGHS, with the pivots it saves; the flagged driver against scipy.optimize.milp on 0/1 programs
and the small general models, with the pivots the cutoff saves; dual feasibility after every OPTIMAL long-step run.  CPU only; the
GPU tests compare the device against this restatement bit for bit."""
import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bounded_dual_ref as D
import _bounded_long_ref as L
import _bounded_ref as B
from test_bnb_bounded_reference import milp

REL = 1e-9          # README "Parity bar": paths that are not bitwise agree in the objective within 1e-9 relative
# The covering optima are compared much tighter, at the bar of the sibling tests: 2.9e-15 relative (13 ulp) is what the plain loop
# (the restatement of lpx_bounded_dual_run2, an existing yardstick) leaves against HiGHS at worst on its own instances (DESIGN
# 4.14).  On each instance below the plain loop is asserted to meet it first (it leaves 0, 7.6e-16 and 0), and the long-step run
# is then held to the same bar; nothing of it comes from the long-step run.
REL_COVER = 2.9e-15
DUAL_FEAS = -1e-9   # -eps: the least reduced cost an OPTIMAL run may leave on a nonbasic column that can still move
BINARY = [(16, 8, 1), (32, 16, 2), (64, 32, 1)]

_SOLVED = {}


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    assert a[0] == b[0] and np.array_equal(_u64(a[1]), _u64(b[1])) and a[2].tolist() == b[2].tolist()
    assert a[3].tolist() == b[3].tolist() and a[4].tolist() == b[4].tolist() and a[5] == b[5]


def _solved(key, *args, **kw):
    """The flagged driver once per (model, flag set), shared by the tests below."""
    flags = kw["search_flags"]
    if (key, flags) not in _SOLVED:
        _SOLVED[key, flags] = L.solve2(*args, **kw)
    return _SOLVED[key, flags]


@pytest.mark.parametrize("flags", [0, L.SKIP_FIXED])
@pytest.mark.parametrize("n,m,seed", [(12, 6, 1), (40, 20, 1), (64, 32, 2)])
def test_without_the_new_flags_it_is_dual_run2_bit_for_bit(oracle, n, m, seed, flags):
    _, _, ub, _, Ts, bs, flip = D.root(n, m, seed)
    for j, l, u in D.children(n, m, seed):
        Tc, ubc, _ = D.change_bounds(Ts, ub, np.zeros(len(ub)), flip, [j], [l], [u])
        Tz, fz, _, bad = N.dualize(Tc, ubc, flip)
        assert bad == 0
        _same(N.dual_run2(Tz, bs, ubc, fz, flags), L.dual_run3(Tz, bs, ubc, fz, flags))
        # a cutoff without its flag is not read
        _same(N.dual_run2(Tz, bs, ubc, fz, flags), L.dual_run3(Tz, bs, ubc, fz, flags, cutoff=1e30))


def test_without_the_new_flags_on_the_covering_and_cycling_instances(oracle):
    T, basis, ub, _ = D.covering(32, 96, 1)
    _same(N.dual_run2(T, basis, ub), L.dual_run3(T, basis, ub))
    Tc, bs, ubc, flip = N.cycling_node()
    Tz, fz, _, _ = N.dualize(Tc, ubc, flip)
    _same(N.dual_run2(Tz, bs, ubc, fz, N.SKIP_FIXED), L.dual_run3(Tz, bs, ubc, fz, L.SKIP_FIXED))


@pytest.mark.parametrize("m,n", [(8, 24), (32, 96), (128, 384)])
def test_dual_start_with_the_long_step_on_covering_models(oracle, m, n):
    c, A, rel, b = L.covering_model(m, n, 1)
    _, want = D.highs_bounded(c, -A, -b, np.zeros(n), np.ones(n), maximise=False)
    plain = L.solve_bounded_dual(c, A, rel, b, 1.0, sense=1, flags=0)
    long_ = L.solve_bounded_dual(c, A, rel, b, 1.0, sense=1, flags=L.LONG_STEP)
    assert plain["status"] == long_["status"] == L.OPTIMAL and plain["counts"][2] == 0
    pivots = [r["counts"][0] + r["counts"][1] for r in (plain, long_)]
    err = [abs(r["value"] - want) / abs(want) for r in (plain, long_)]
    print("covering", (m, n), "pivots plain / long", pivots, "passes", long_["counts"][2], "relative error plain / long", err)
    assert err[0] <= REL_COVER, "the plain loop misses the bar the long step is held to"
    assert err[1] <= REL_COVER
    assert long_["counts"][2] > 0, "no column passed: the instance tests nothing"
    assert L.least_reduced_cost(long_["T"], long_["basis"], long_["ub"]) >= DUAL_FEAS
    x = long_["x"]
    assert (A @ x >= b - 1e-7).all() and (x >= -1e-9).all() and (x <= 1 + 1e-9).all()
    assert abs(float(c @ x) - want) <= REL * abs(want)
    # the dual start of a covering model is the loop on the covering tableau: same events
    T, basis, ub, _ = D.covering(m, n, 1)
    st, Tl, bl, fl, tr, counts = L.dual_run3(T, basis, ub, flags=L.LONG_STEP)
    assert tr.tolist() == long_["trace"].tolist() and np.array_equal(_u64(Tl), _u64(long_["T"]))
    if (m, n) == (128, 384):
        assert 2 * pivots[1] <= pivots[0], "the long step needs more than half the pivots of the plain loop"


def test_dual_start_on_a_mixed_model(oracle):
    c, A, rel, b, upper, lower, sense = L.mixed_model()
    out = L.solve_bounded_dual(c, A, rel, b, upper, lower, sense)
    Au = np.where((rel == 1)[:, None], -A, A); bu = np.where(rel == 1, -b, b)
    _, want = D.highs_bounded(c, Au, bu, lower, upper, maximise=False)
    assert out["status"] == L.OPTIMAL and abs(out["value"] - want) <= REL * abs(want)
    assert out["dualize_flips"] > 0 and out["counts"][2] > 0 and out["counts"][0] > 0 and out["counts"][1] > 0
    assert out["constant"] == float(c[0] * lower[0]) != 0.0
    assert L.least_reduced_cost(out["T"], out["basis"], out["ub"]) >= DUAL_FEAS
    x = out["x"]
    assert (Au @ x <= bu + 1e-7).all() and (x >= lower - 1e-9).all() and (x <= upper + 1e-9).all()


def test_dual_start_refuses_an_improving_variable_without_an_upper_bound(oracle):
    c, A, rel, b = L.covering_model(8, 24, 1)
    upper = np.ones(24); upper[[5, 9]] = np.inf
    L.prepare_dual(c, A, rel, b, None, upper, sense=1)          # Min of positive costs: nothing improves
    cneg = c.copy(); cneg[[9, 5]] = -1.0
    with pytest.raises(ValueError, match="^x6$"):
        L.prepare_dual(cneg, A, rel, b, None, upper, sense=1)


def test_an_infeasible_event_keeps_its_passes(oracle):
    """x1 + x2 >= 3 over 0 <= x <= 1: both columns pass, then no column is left."""
    from linear_programming_solver_lpr381_amd import synth
    T, basis = synth.primal_tableau_from(np.array([-1.0, -2.0]), np.array([[-1.0, -1.0]]), np.array([-3.0]))
    ub = np.array([1.0, 1.0, np.inf])
    st, Tl, bl, fl, tr, counts = L.dual_run3(T, basis, ub, flags=L.LONG_STEP)
    assert st == L.INFEASIBLE and tr.tolist() == [[-1, 0], [-1, 1]] and counts == (0, 0, 2) and fl.tolist() == [1, 1, 0]
    assert Tl[0].tolist() == [1.0, 1.0, 1.0, -1.0] and Tl[1, 3] == -3.0
    ub = np.array([1.0, np.inf, np.inf])
    st, Tl, bl, _, tr, _ = L.dual_run3(T, basis, ub, flags=L.LONG_STEP)
    assert st == L.OPTIMAL and tr.tolist() == [[-1, 0], [0, 1]]         # the +inf column stops the chain and enters
    assert L.least_reduced_cost(Tl, bl, ub) >= DUAL_FEAS


def test_cutoff_rule(oracle):
    T, basis, ub, _ = D.covering(8, 24, 1)
    z0 = T[-1, -1]
    for flags in (L.CUTOFF_FLAG, L.CUTOFF_FLAG | L.LONG_STEP):
        st, Tc, bc, fc, tr, counts = L.dual_run3(T, basis, ub, flags=flags, cutoff=z0)          # <=: equality fires
        assert st == L.CUTOFF and len(tr) == 0 and np.array_equal(_u64(Tc), _u64(T))
        full = L.dual_run3(T, basis, ub, flags=flags, cutoff=-np.inf)                           # -inf never fires
        _same(full, L.dual_run3(T, basis, ub, flags=flags & ~L.CUTOFF_FLAG))
        assert full[0] == L.OPTIMAL
        if flags & L.LONG_STEP:
            assert L.least_reduced_cost(full[1], full[2], ub) >= DUAL_FEAS
        mid = 0.5 * (z0 + full[1][-1, -1])
        st, Tc, bc, fc, tr, counts = L.dual_run3(T, basis, ub, flags=flags, cutoff=mid)
        assert st == L.CUTOFF and 0 < len(tr) < len(full[4]) and Tc[-1, -1] <= mid
        assert tr.tolist() == full[4][: len(tr)].tolist()


@pytest.mark.parametrize("flags", L.FLAG_SETS)
@pytest.mark.parametrize("n,m,seed", BINARY)
def test_flagged_driver_on_binary_programs(oracle, n, m, seed, flags):
    c, A0, b0 = N.binary_model(n, m, seed)
    out = _solved((n, m, seed), c, A0, b0, np.ones(n), search_flags=flags)
    st, want = milp(c, A0, np.zeros(m), b0, np.ones(n))
    assert out["rc"] == 0 and out["status"] == st == L.OPTIMAL and len(out["log"]) == out["nodes"]
    print("binary", (n, m, seed), "flags", flags, "nodes", out["nodes"], "pivots", out["pivots"], "passes", out["passes"],
          "optimum", out["value"], "milp", want)
    assert abs(out["value"] - want) <= REL * max(1.0, abs(want))
    x = out["x"]
    assert np.array_equal(x, np.rint(x)) and (x >= 0).all() and (x <= 1).all() and (A0 @ x <= b0 + 1e-9).all()
    assert abs(float(c @ x) - want) <= REL * max(1.0, abs(want))
    if flags == 0:
        base = N.solve(c, A0, b0, np.ones(n))
        assert base["log"].tobytes() == out["log"].tobytes() and base["value"] == out["value"], "search_flags = 0 moved the log"
    if flags & L.CUTOFF_FLAG:
        plain = _solved((n, m, seed), c, A0, b0, np.ones(n), search_flags=flags & ~L.CUTOFF_FLAG)
        assert out["pivots"] < plain["pivots"], "the cutoff saved no pivot"
        assert (out["log"]["status"] == L.CUTOFF).any()
    else:
        assert not (out["log"]["status"] == L.CUTOFF).any()
    assert bool(out["passes"]) == bool(flags & L.LONG_STEP)
    if flags & L.LONG_STEP:
        print("least reduced cost after", out["long_optimal_nodes"], "OPTIMAL long-step nodes:", out["least_rc"])
        assert out["long_optimal_nodes"] > 0 and out["least_rc"] >= DUAL_FEAS


@pytest.mark.parametrize("flags", L.FLAG_SETS)
@pytest.mark.parametrize("name", ["general", "lowers", "min", "mixed", "infeasible"])
def test_flagged_driver_on_small_models(oracle, name, flags):
    c, A, rel, b, upper, lower, is_int, sense = N.small_models()[name]
    kw = dict(lower=lower, is_int=is_int, sense=sense, rel=rel)
    out = _solved(name, c, A, b, upper, search_flags=flags, **kw)
    st, want = milp(c, A, rel, b, upper, lower, is_int, sense)
    assert out["rc"] == 0 and out["status"] == st and (st == L.INFEASIBLE) == (name == "infeasible")
    print("model", name, "flags", flags, "nodes", out["nodes"], "pivots", out["pivots"], "passes", out["passes"])
    if st == L.OPTIMAL:
        assert abs(out["value"] - want) <= REL * max(1.0, abs(want))
        x = out["x"]
        ints = np.ones(len(c), dtype=bool) if is_int is None else is_int != 0
        assert np.array_equal(x[ints], np.rint(x[ints])) and (A @ x <= b + 1e-7).all()
        assert (x >= (0 if lower is None else lower) - 1e-9).all() and (x <= upper + 1e-9).all()
        assert abs(float(c @ x) - want) <= 1e-7 * max(1.0, abs(want))
    if flags & L.LONG_STEP:
        print("least reduced cost after", out["long_optimal_nodes"], "OPTIMAL long-step nodes:", out["least_rc"])
        assert out["long_optimal_nodes"] > 0 and out["least_rc"] >= DUAL_FEAS
    if flags & L.CUTOFF_FLAG:
        plain = _solved(name, c, A, b, upper, search_flags=flags & ~L.CUTOFF_FLAG, **kw)
        if st == L.OPTIMAL:
            assert out["pivots"] < plain["pivots"], "the cutoff saved no pivot"
        else:
            # no incumbent is ever found: the cutoff stays at -inf, never fires, and the search is the plain one
            assert out["log"].tobytes() == plain["log"].tobytes()


def test_every_optimal_long_step_node_ends_dual_feasible(oracle):
    """The long-step nodes of binary_bounded(16, 8, 1), replayed: after every OPTIMAL node no nonbasic column that can still move
    (ub > 0) has a reduced cost below -1e-9."""
    c, A0, b0 = N.binary_model(16, 8, 1)
    T0, basis0, ub0, *_ = N.prepare(c, A0, b0, None, np.ones(16))
    st, Ts, bs, flip, _, _ = B.run(T0, basis0, ub0)
    h = L.Handle(Ts, bs, ub0, flip)
    worst, seen = np.inf, 0
    for j, v in ((3, 1.0), (7, 0.0), (3, 0.0), (11, 1.0), (7, 1.0), (0, 1.0), (11, 0.0)):
        rec = h.node2(np.array([j], dtype=np.int32), [v], [v], 16, flags=L.SKIP_FIXED | L.LONG_STEP)
        if rec["status"] == L.OPTIMAL:
            worst = min(worst, L.least_reduced_cost(h.T, h.basis, h.ub)); seen += 1
    print("least reduced cost after", seen, "OPTIMAL long-step nodes:", worst)
    assert seen >= 3 and worst >= DUAL_FEAS
