"""CPU checks of the restatement of lpx_packed_base_solve_costs (tests/_packed_cost_ref.py) against the cold solve of every
scenario (tests/_packed_dual_ref.py: solve from the slack basis; scipy.optimize.linprog where the dual start refuses the costs):
c_i = c0 bit-equal to the base with 0 events, c_i = c0 with b bit-equal to _packed_warm_ref.solve, equal statuses, optima within the
project's 1e-9 relative bar, primal feasibility, d = c_i - A^T y and strong duality by what they mean, refused inputs, and fewer
events than the cold solves on covering 12x60.  The scenario sets are those of tests/test_gpu_packed_cost.py."""
import numpy as np
import pytest

import _packed_cost_ref as K
import _packed_dual_ref as P
import _packed_warm_ref as W

INF = np.inf
FORMS = [False, True]                                   # without b, with b


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _linprog(c, A, rel, b, lower, upper, sense):
    """(status, optimum) by scipy's HiGHS: the independent reference where the cold dual start refuses the costs."""
    from scipy.optimize import linprog
    n = len(c)
    lo = np.zeros(n) if lower is None else np.broadcast_to(np.asarray(lower, dtype=np.float64), (n,))
    up = np.full(n, INF) if upper is None else np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,))
    sign = np.where(np.asarray(rel) == P.GE, -1.0, 1.0)
    obj = c if sense == P.MIN else -c
    r = linprog(obj, A_ub=A * sign[:, None], b_ub=b * sign, bounds=[(l, None if u == INF else u) for l, u in zip(lo, up)], method="highs")
    if r.status == 3:
        return K.UNBOUNDED, None
    if r.status == 2:
        return K.INFEASIBLE, None
    assert r.status == 0, r.message
    return K.OPTIMAL, r.fun if sense == P.MIN else -r.fun


def _check_optimal(w, c, A, rel, b, lower, upper, what):
    """An OPTIMAL answer by what it means: primal feasibility, d = c - A^T y, complementary bounds, strong duality."""
    m, n = A.shape
    lo = np.zeros(n) if lower is None else np.broadcast_to(np.asarray(lower, dtype=np.float64), (n,))
    up = np.full(n, INF) if upper is None else np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,))
    ge = rel == P.GE
    Ax = A @ w.x
    viol = np.where(ge, b - Ax, Ax - b)
    assert (viol <= 1e-9 * np.maximum(1.0, np.abs(b))).all(), (what, viol.max())
    assert (w.x >= lo - 1e-9 * np.maximum(1.0, np.abs(lo))).all() and (w.x <= up + 1e-9 * np.maximum(1.0, np.abs(up))).all(), what
    assert np.abs(w.d - (c - A.T @ w.y)).max() <= 1e-9 * max(1.0, np.abs(c).max()), what
    basic = np.zeros(n + m, dtype=bool); basic[w.basis] = True
    assert np.abs(w.d[basic[:n]]).max(initial=0.0) <= 1e-9 * max(1.0, np.abs(c).max()), what
    at_up = w.at_upper != 0
    at_lo = ~at_up & ~basic[:n]
    assert np.array_equal(w.x[at_up], up[at_up]) and np.array_equal(w.x[at_lo], lo[at_lo]), what
    dual_value = w.y @ b + (w.d[at_up] * up[at_up]).sum() + (w.d[at_lo] * lo[at_lo]).sum()
    assert abs(w.value - dual_value) <= 1e-9 * max(1.0, abs(w.value)), (what, w.value, dual_value)


@pytest.mark.parametrize("with_b", FORMS)
@pytest.mark.parametrize("name", list(W.SETS))
def test_scenarios_agree_with_their_cold_solves(name, with_b):
    (c0, A, rel, b0, upper, lower, sense), cs, rhs = K.cost_set(name)
    warm, cold = K.set_refs(name, True, with_b), K.set_cold(name, with_b)
    for i, (w, k) in enumerate(zip(warm, cold)):
        what = (name, with_b, i)
        b = rhs[i] if with_b else b0
        assert w.primal_events == sum(w.pcounts) and w.dual_events == sum(w.dcounts), what
        if not with_b:
            assert w.dual_events == 0 and w.status != K.INFEASIBLE, what
        if k.status == P.EINVAL:                        # an improving cost on a column without an upper bound: the dual start refuses
            assert k.why == "precheck" and not 1 <= i <= K.N_SPREAD, what       # never on the +-30 % vectors
            status, value = _linprog(cs[i], A, rel, b, lower, upper, sense)
            if w.status == K.UNBOUNDED and with_b and status == K.INFEASIBLE:
                continue                                # the contract: an unbounded primal phase is reported even where b_i is infeasible
            assert w.status == status, what
            if status == K.OPTIMAL:
                assert abs(w.value - value) <= 1e-9 * max(1.0, abs(value)), (what, w.value, value)
                _check_optimal(w, cs[i], A, rel, b, lower, upper, what)
            continue
        assert w.status == k.status, what               # OPTIMAL or, with b, INFEASIBLE
        if 1 <= i <= K.N_SPREAD and not with_b:
            assert k.status == P.OPTIMAL, what          # no +-30 % scenario is left out of the cold comparison
        if k.status != P.OPTIMAL:
            continue
        assert abs(w.value - k.value) <= 1e-9 * max(1.0, abs(k.value)), (what, w.value, k.value)
        _check_optimal(w, cs[i], A, rel, b, lower, upper, what)


@pytest.mark.parametrize("name", list(W.SETS))
def test_spread_costs_are_all_optimal_on_both_sides(name):
    """On the +-30 % vectors with the base's right-hand side every scenario of every set is OPTIMAL warm and cold."""
    warm, cold = K.set_refs(name, True, False), K.set_cold(name, False)
    for i in range(1, K.N_SPREAD + 1):
        assert warm[i].status == K.OPTIMAL and cold[i].status == P.OPTIMAL, (name, i)


@pytest.mark.parametrize("long_step", [True, False])
@pytest.mark.parametrize("name", list(W.SETS))
def test_the_base_costs_are_the_base_bit_for_bit(name, long_step):
    cb = K.set_base(name, long_step)
    _, cs, rhs = K.cost_set(name)
    assert np.array_equal(cs[0], cb.c0)
    w, k = K.set_refs(name, long_step, False)[0], cb.base.cold
    assert (w.status, w.primal_events, w.dual_events, w.pcounts, w.dcounts) == (K.OPTIMAL, 0, 0, (0, 0, 0), (0, 0, 0))
    for a, b in ((w.x, k.x), (w.value, k.value), (w.z, k.z), (w.y, k.y), (w.d, k.d)):
        assert np.array_equal(_u64(a), _u64(b))
    assert w.basis.tolist() == k.basis.tolist() and w.at_upper.tolist() == k.at_upper.tolist()
    T, constant, shifted = K.cost_move(cb.base, cb.c0, cb.c0)
    assert np.array_equal(_u64(T), _u64(cb.base.T)) and shifted == cb.base.shifted
    assert not shifted or _u64(constant) == _u64(cb.base.constant)
    # with b: the right-hand-side call, bit for bit
    for bi in W.scenario_set(name)[1]:
        w, r = K.solve(cb, cb.c0, bi, long_step=long_step), W.solve(cb.base, bi, long_step=long_step)
        assert (w.status, w.primal_events, w.dual_events, w.dcounts) == (r.status, 0, r.events, r.counts)
        for a, b in ((w.x, r.x), (w.value, r.value), (w.z, r.z), (w.y, r.y), (w.d, r.d)):
            assert np.array_equal(_u64(a), _u64(b))
        assert w.basis.tolist() == r.basis.tolist() and w.at_upper.tolist() == r.at_upper.tolist()


def test_fewer_events_than_the_cold_solves_on_covering_12x60():
    for with_b in FORMS:
        warm = sum(r.primal_events + r.dual_events for r in K.set_refs("covering 12x60", True, with_b)[1:])
        cold = sum(r.events for r in K.set_cold("covering 12x60", with_b)[1:])
        assert 0 < warm < cold, (with_b, warm, cold)


def test_the_unbounded_hand_model_and_the_reporting_rule():
    model, cs, rhs = K.unbounded_hand()
    cb = K.open_model(model)
    rs = K.solve_all(cb, cs)
    assert [r.status for r in rs] == [K.OPTIMAL, K.UNBOUNDED, K.OPTIMAL] and [r.value for r in rs] == [3.0, -3.0, 6.0]
    assert rs[0].primal_events == 0 and rs[2].primal_events == 0
    assert _linprog(cs[1], *[model[k] for k in (1, 2, 3, 5, 4, 6)])[0] == K.UNBOUNDED
    rb = K.solve_all(cb, cs, rhs)
    assert [r.status for r in rb] == [K.OPTIMAL, K.UNBOUNDED, K.OPTIMAL] and rb[2].value == 8.0 and rb[1].dual_events == 0


def test_inputs_that_are_not_finite_are_refused_alone():
    cb = K.set_base("mixed 12x16")
    _, cs, rhs = K.cost_set("mixed 12x16")
    cs, rhs = cs[:4].copy(), rhs[:4].copy()
    cs[1, 3] = np.nan; rhs[2, 11] = -INF
    rs = K.solve_all(cb, cs, rhs)
    want = K.set_refs("mixed 12x16", True, True)
    assert [r.status for r in rs] == [want[0].status, K.EINVAL, K.EINVAL, want[3].status]
    for r in rs[1:3]:
        assert not r.x.any() and not r.y.any() and not r.d.any() and not r.basis.any() and not r.at_upper.any()
        assert (r.value, r.primal_events, r.dual_events, r.pcounts, r.dcounts, r.z) == (0.0, 0, 0, (0, 0, 0), (0, 0, 0), 0.0)
    assert K.solve_all(cb, cs)[2].status == K.OPTIMAL   # the infinity stands in b only
    for got, wanted in zip(rs[3], want[3]):
        assert np.array_equal(got, wanted)


def test_the_iteration_limits_are_tested_first_and_apart():
    cb = K.set_base("covering 12x60")
    _, cs, rhs = K.cost_set("covering 12x60")
    full = K.solve(cb, cs[1], rhs[1])
    assert full.status == K.OPTIMAL and full.primal_events > 2 and full.dual_events > 2
    for limit in (0, 1, 2):
        r = K.solve(cb, cs[1], rhs[1], p_max_iter=limit)
        assert (r.status, r.primal_events, r.dual_events) == (K.ITER_LIMIT, limit, 0)
        r = K.solve(cb, cs[1], rhs[1], d_max_iter=limit)
        assert r.status == K.ITER_LIMIT and r.primal_events == full.primal_events and r.dual_events >= limit
    assert K.solve(cb, cb.c0, p_max_iter=0).status == K.ITER_LIMIT                 # even where nothing is left to do
    assert K.solve(cb, cb.c0, d_max_iter=0).status == K.OPTIMAL                    # without b the dual loop is not run


def test_the_sets_of_the_gpu_tests_exercise_every_edge():
    seen = {"kind0": 0, "kind1": 0, "flips": 0, "dual kind0": 0, "dual kind1": 0, "passes": 0, "infeasible": 0}
    for name in W.SETS:
        for with_b in FORMS:
            for r in K.set_refs(name, True, with_b):
                seen["kind0"] += r.pcounts[0]; seen["kind1"] += r.pcounts[1]; seen["flips"] += r.pcounts[2]
                seen["dual kind0"] += r.dcounts[0]; seen["dual kind1"] += r.dcounts[1]; seen["passes"] += r.dcounts[2]
                seen["infeasible"] += r.status == K.INFEASIBLE
    assert all(v > 0 for v in seen.values()), seen
    mixed = K.set_base("mixed 12x16").base
    assert mixed.shifted and (mixed.flip[:16] & 1).any() and not (mixed.flip[:16] & 1).all()      # K is non-zero, some g_j negated
    assert K.set_base("max, <= rows").base.cold.dualize_flips == 12                # every column flipped in front of the base's loop
    assert len(K.set_base("4x1100").base.ub) > 1024                               # the column loop of step 3 takes a second trip
