"""CPU checks of the restatement of lpx_solve_packed_dual (tests/_packed_dual_ref.py), against things that do not share its
arithmetic: optimum and x against HiGHS; the duals by what they mean (finite differences of the optimum in b, d = c - A^T y,
zero reduced costs on basic columns, strong duality) on models asserted non-degenerate; the order of the per-model refusals; and
the event kinds that the instances shared with tests/test_gpu_packed_dual.py exercise."""
import numpy as np
import pytest

import _bounded_dual_ref as D
import _bounded_long_ref as L
import _packed_dual_ref as P

INF = np.inf


def _models():
    """name -> (c, A, rel, b, upper, lower, sense)"""
    out = {"mixed": L.mixed_model()}
    c, A, rel, b, up = P.hand_model()
    out["hand 2x3"] = (c, A, rel, b, up, None, P.MIN)
    for s in (1, 2, 3):
        c, A, rel, b = L.covering_model(6, 12, s)
        out["covering(6, 12, %d)" % s] = (c, A, rel, b, np.ones(12), None, P.MIN)
    c, A, rel, b, up = P.max_le_model(2)
    out["max, <= rows"] = (c, A, rel, b, up, None, P.MAX)
    return out


def _highs(c, A, rel, b, lower, upper, sense):
    """(status, optimum, x) of HiGHS on the user's model: >= rows negated for linprog's A_ub."""
    from scipy.optimize import linprog
    ge = np.asarray(rel) == P.GE
    A2, b2 = np.where(ge[:, None], -A, A), np.where(ge, -b, b)
    st, value = D.highs_bounded(c, A2, b2, lower, upper, maximise=sense == P.MAX)
    x = linprog(c if sense == P.MIN else -c, A_ub=A2, b_ub=b2, bounds=list(zip(lower, upper)), method="highs").x
    return st, value, x


@pytest.mark.parametrize("name", ["mixed", "hand 2x3", "covering(6, 12, 1)", "covering(6, 12, 2)", "covering(6, 12, 3)"])
@pytest.mark.parametrize("long_step", [True, False])
def test_optimum_and_x_against_highs(name, long_step):
    c, A, rel, b, upper, lower, sense = _models()[name]
    n = len(c)
    r = P.solve(c, A, b, rel, lower, upper, sense, long_step=long_step)
    st, value, x = _highs(c, A, rel, b, np.zeros(n) if lower is None else lower, np.broadcast_to(upper, (n,)), sense)
    assert r.status == P.OPTIMAL == st
    assert abs(r.value - value) <= 1e-9 * max(1.0, abs(value))
    assert np.abs(r.x - x).max() <= 1e-9 * max(1.0, np.abs(x).max())          # the optimum is unique: the models are non-degenerate


def _non_degenerate(r, c, A, rel, b, lower, upper):
    """Every basic value more than 1e-6 from both bounds, every nonbasic reduced cost (a slack's is y_i) above 1e-6 in size."""
    m, n = A.shape
    basic = np.zeros(n + m, dtype=bool); basic[r.basis] = True
    slack = np.where(rel == P.GE, A @ r.x - b, b - A @ r.x)
    for j in range(n):
        if basic[j]:
            assert min(r.x[j] - lower[j], upper[j] - r.x[j]) > 1e-6, j
        else:
            assert abs(r.d[j]) > 1e-6, j
    for i in range(m):
        if basic[n + i]:
            assert slack[i] > 1e-6, i
        else:
            assert abs(r.y[i]) > 1e-6, i
    return basic


@pytest.mark.parametrize("name", ["max, <= rows", "covering(6, 12, 1)", "mixed"])
def test_duals_by_their_meaning(name):
    c, A, rel, b, upper, lower, sense = _models()[name]
    m, n = A.shape
    lo = np.zeros(n) if lower is None else lower
    up = np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,))
    r = P.solve(c, A, b, rel, lower, upper, sense)
    assert r.status == P.OPTIMAL
    basic = _non_degenerate(r, c, A, rel, b, lo, up)
    h = 1e-4
    for i in range(m):                                  # y_i = d value / d b_i, in the user's sense and on the user's row
        e = np.zeros(m); e[i] = h
        moved = P.solve(c, A, b + e, rel, lower, upper, sense)
        assert moved.status == P.OPTIMAL and moved.basis.tolist() == r.basis.tolist()
        assert abs((moved.value - r.value) - r.y[i] * h) <= 1e-9, (i, moved.value - r.value, r.y[i] * h)
    assert np.abs(r.d - (c - A.T @ r.y)).max() <= 1e-9              # d = c - A^T y
    assert not r.d[basic[:n]].any()                                  # +-0 on basic columns
    at_up = r.at_upper != 0
    at_lo = ~at_up & ~basic[:n]
    assert np.array_equal(r.x[at_up], up[at_up]) and np.array_equal(r.x[at_lo], lo[at_lo])
    dual_value = r.y @ b + (r.d[at_up] * up[at_up]).sum() + (r.d[at_lo] * lo[at_lo]).sum()
    assert abs(r.value - dual_value) <= 1e-9 * max(1.0, abs(r.value))                                # strong duality


def test_duals_have_the_signs_of_their_sense():
    """A Min model pays for a larger >= right-hand side and gains from a larger <= one; a Max model the other way round."""
    c, A, rel, b, upper, lower, sense = _models()["mixed"]
    r = P.solve(c, A, b, rel, lower, upper, sense)
    assert (r.y[rel == P.GE] >= 0.0).all() and (r.y[rel == P.LE] <= 0.0).all() and (r.y != 0.0).any()
    c, A, rel, b, upper, lower, sense = _models()["max, <= rows"]
    r = P.solve(c, A, b, rel, lower, upper, sense)
    assert (r.y >= 0.0).all() and (r.y != 0.0).any()
    assert (r.d[r.at_upper != 0] > 0.0).all()           # a Max model holds a variable at its upper bound because it still gains


def test_refusal_order_and_the_other_models_are_unchanged():
    c, A, rel, b, upper, lower, sense = _models()["mixed"]
    m, n = A.shape
    good = P.solve(c, A, b, rel, lower, upper, sense)
    bad_upper = upper.copy(); bad_upper[3] = lower[3] - 1.0             # below its lower bound
    bad_rel = rel.copy(); bad_rel[5] = 2                                # LPX_EQ is not accepted
    open_upper = upper.copy(); open_upper[np.flatnonzero(c < 0)[0]] = INF          # Min, c_j < 0: improving and unbounded above
    assert P.solve(c, A, b, bad_rel, lower, bad_upper, sense).why == "bound"       # every defect at once: the bound first
    assert P.solve(c, A, b, bad_rel, lower, open_upper, sense).why == "rel"        # then the row senses
    assert P.solve(c, A, b, rel, lower, open_upper, sense).why == "precheck"
    nan_lower = lower.copy(); nan_lower[0] = np.nan
    assert P.solve(c, A, b, rel, nan_lower, upper, sense).why == "bound"
    # one batch of five: the refused ones are zeroed, the good ones are what they are alone
    rels = np.stack([rel, bad_rel, rel, rel, rel])
    uppers = np.stack([upper, upper, bad_upper, open_upper, upper])
    rs = P.solve_all(c, A, b, rels, lower, uppers, sense)
    assert [r.status for r in rs] == [P.OPTIMAL, P.EINVAL, P.EINVAL, P.EINVAL, P.OPTIMAL]
    for r in (rs[0], rs[4]):
        for got, want in zip(r, good):
            assert np.array_equal(got, want)
    for r in rs[1:4]:
        assert not r.x.any() and not r.y.any() and not r.d.any() and not r.basis.any() and not r.at_upper.any()
        assert (r.value, r.events, r.counts, r.dualize_flips, r.z) == (0.0, 0, (0, 0, 0), 0, 0.0)


def test_the_instances_of_the_gpu_tests_exercise_every_event_kind():
    """kind-0 pivots, kind-1 pivots, passes and dualize flips each at least once, and INFEASIBLE at least once."""
    seen = {"kind0": 0, "kind1": 0, "passes": 0, "dualize_flips": 0, "infeasible": 0}
    for name in P.SHAPES:
        for long_step in (True, False):
            for r in P.shape_refs(name, long_step):
                seen["kind0"] += r.counts[0]; seen["kind1"] += r.counts[1]; seen["passes"] += r.counts[2]
                seen["dualize_flips"] += r.dualize_flips; seen["infeasible"] += r.status == P.INFEASIBLE
    assert all(v > 0 for v in seen.values()), seen
    wide = P.shape_refs("4x1100", True)
    assert all(r.dualize_flips > 0 and r.counts[2] > 0 for r in wide)        # the second trip of the count and of the flip list
