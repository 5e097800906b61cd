"""CPU checks of the restatement of lpx_packed_base_open / lpx_packed_base_solve (tests/_packed_warm_ref.py) against the cold solve
of every scenario (tests/_packed_dual_ref.py: solve from the slack basis), which shares the loop but not the start: equal statuses,
optima within the project's 1e-9 relative bar, primal feasibility, d = c - A^T y and strong duality by what they mean, a zero
delta bit-equal to the base, refused right-hand sides, and fewer events than the cold solves where the issue measured that.  The
scenario sets are those of tests/test_gpu_packed_warm.py."""
import numpy as np
import pytest

import _packed_dual_ref as P
import _packed_warm_ref as W

INF = np.inf


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.mark.parametrize("long_step", [True, False])
@pytest.mark.parametrize("name", list(W.SETS))
def test_warm_scenarios_agree_with_their_cold_solves(name, long_step):
    (c, A, rel, b0, upper, lower, sense), bs = W.scenario_set(name)
    m, n = A.shape
    warm, cold = W.set_refs(name, long_step), W.set_cold(name, long_step)
    assert [r.status for r in warm] == [r.status for r in cold]
    assert warm[0].status == P.OPTIMAL                  # the first scenario is the base's own right-hand side
    lo = np.zeros(n) if lower is None else np.broadcast_to(np.asarray(lower, dtype=np.float64), (n,))
    up = np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,))
    ge = rel == P.GE
    for i, (w, k) in enumerate(zip(warm, cold)):
        assert w.dualize_flips == 0 and w.events == sum(w.counts) and w.why == ""
        if w.status != P.OPTIMAL:
            continue
        # the project's 1e-9 relative bar; the floor of 1 because a warm optimum of -8.9e-16 meets a cold -0.0
        assert abs(w.value - k.value) <= 1e-9 * max(1.0, abs(k.value)), (i, w.value, k.value)
        # primal feasibility to the same scale: the loop stops when no basic value is more than eps = 1e-9 beyond a bound
        Ax = A @ w.x
        viol = np.where(ge, bs[i] - Ax, Ax - bs[i])
        assert (viol <= 1e-9 * np.maximum(1.0, np.abs(bs[i]))).all(), (i, viol.max())
        assert (w.x >= lo - 1e-9 * np.maximum(1.0, np.abs(lo))).all() and (w.x <= up + 1e-9 * np.maximum(1.0, np.abs(up))).all(), i
        # the duals, as tests/test_packed_dual_ref.py checks them: d = c - A^T y, +-0 on basic columns, strong duality
        assert np.abs(w.d - (c - A.T @ w.y)).max() <= 1e-9 * max(1.0, np.abs(c).max()), i
        basic = np.zeros(n + m, dtype=bool); basic[w.basis] = True
        assert not w.d[basic[:n]].any(), i
        at_up = w.at_upper != 0
        at_lo = ~at_up & ~basic[:n]
        assert np.array_equal(w.x[at_up], up[at_up]) and np.array_equal(w.x[at_lo], lo[at_lo]), i
        dual_value = w.y @ bs[i] + (w.d[at_up] * up[at_up]).sum() + (w.d[at_lo] * lo[at_lo]).sum()
        assert abs(w.value - dual_value) <= 1e-9 * max(1.0, abs(w.value)), (i, w.value, dual_value)


@pytest.mark.parametrize("long_step", [True, False])
@pytest.mark.parametrize("name", list(W.SETS))
def test_a_zero_delta_is_the_base_bit_for_bit(name, long_step):
    base, w = W.set_base(name, long_step), W.set_refs(name, long_step)[0]
    k = base.cold
    assert np.array_equal(W.scenario_set(name)[1][0], base.b0)
    assert (w.status, w.events, w.counts, w.dualize_flips) == (P.OPTIMAL, 0, (0, 0, 0), 0)
    for a, b in ((w.x, k.x), (w.value, k.value), (w.z, k.z), (w.y, k.y), (w.d, k.d)):
        assert np.array_equal(_u64(a), _u64(b))
    assert w.basis.tolist() == k.basis.tolist() and w.at_upper.tolist() == k.at_upper.tolist()


def test_fewer_events_than_the_cold_solves_on_covering_12x60():
    """+-20 % right-hand sides of covering(12, 60): the summed events of the warm runs lie below those of the cold runs (the issue
    measured 22.5 against 55.5 per scenario)."""
    for long_step in (True, False):
        warm = sum(r.events for r in W.set_refs("covering 12x60", long_step)[1:])
        cold = sum(r.events for r in W.set_cold("covering 12x60", long_step)[1:])
        assert 0 < warm < cold, (long_step, warm, cold)


def test_a_right_hand_side_that_is_not_finite_is_refused_alone():
    base = W.set_base("mixed 12x16", True)
    bs = W.scenario_set("mixed 12x16")[1][:4].copy()
    bs[1, 3] = np.nan; bs[2, 11] = -INF
    rs = W.solve_all(base, bs)
    assert [r.status for r in rs] == [P.OPTIMAL, P.EINVAL, P.EINVAL, W.set_refs("mixed 12x16", True)[3].status]
    for r in rs[1:3]:
        assert not r.x.any() and not r.y.any() and not r.d.any() and not r.basis.any() and not r.at_upper.any()
        assert (r.value, r.events, r.counts, r.dualize_flips, r.z) == (0.0, 0, (0, 0, 0), 0, 0.0)
    for got, want in zip(rs[3], W.set_refs("mixed 12x16", True)[3]):
        assert np.array_equal(got, want)


def test_a_base_that_is_not_optimal_is_not_opened():
    c, A, rel, b = P._covering(6, 12, (1,), True)[1]   # more than every variable at its upper bound can cover
    with pytest.raises(ValueError):
        W.open_base(c, A, b, rel, None, 1.0, P.MIN)
    with pytest.raises(ValueError):                     # the iteration limit
        W.open_base(*[W.scenario_set("covering 6x12")[0][k] for k in (0, 1, 3, 2)], None, 1.0, P.MIN, max_iter=1)


def test_the_iteration_limit_is_tested_first():
    base = W.set_base("covering 12x60", True)
    b = W.scenario_set("covering 12x60")[1][1]
    full = W.solve(base, b)
    assert full.status == P.OPTIMAL and full.events > 2
    for max_iter in (0, 1, 2):
        r = W.solve(base, b, max_iter=max_iter)
        assert r.status == P.ITER_LIMIT and r.events >= max_iter and (max_iter > 0 or r.events == 0)
    assert W.solve(base, base.b0, max_iter=0).status == P.ITER_LIMIT            # even where nothing is left to do


def test_the_sets_of_the_gpu_tests_exercise_every_event_kind():
    """Warm runs make kind-0 pivots, kind-1 pivots and passes and end INFEASIBLE, each at least once; the bases carry dualize
    flips, flipped columns and a lower shift; delta has zeros beside non-zeros where the zero skip matters."""
    seen = {"kind0": 0, "kind1": 0, "passes": 0, "infeasible": 0, "events in hand 2x3": 0}
    for name in W.SETS:
        for long_step in (True, False):
            for r in W.set_refs(name, long_step):
                seen["kind0"] += r.counts[0]; seen["kind1"] += r.counts[1]; seen["passes"] += r.counts[2]
                seen["infeasible"] += r.status == P.INFEASIBLE
                if name == "hand 2x3":
                    seen["events in hand 2x3"] += r.events
    assert all(v > 0 for v in seen.values()), seen
    assert W.set_base("mixed 12x16", True).cold.dualize_flips > 0 and W.set_base("mixed 12x16", True).shifted
    assert W.set_base("max, <= rows", True).cold.dualize_flips == 12              # every column flipped in front of the base's loop
    hand = W.scenario_set("hand 2x3")
    moves = hand[1] - hand[0][3]
    assert any(mv[0] != 0.0 and mv[1] == 0.0 for mv in moves) and any(mv[0] == 0.0 and mv[1] != 0.0 for mv in moves)
    assert any(mv.all() for mv in moves)
    wide = W.set_base("4x1100", True)
    assert wide.flip[1024:].any() and len(wide.ub) > 1024                         # the second trip of the copies carries data
