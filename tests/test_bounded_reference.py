"""The NumPy restatement of the bounded-variable primal simplex (tests/_bounded_ref.py) against independent answers: the
hand example event by event, the oracle's primal loop when no column is bounded, the explicit-rows form of the same models
solved by the oracle, and SciPy/HiGHS.  CPU only; the GPU tests compare the device loop against this restatement bit for bit."""
import numpy as np
import pytest

import _bounded_ref as B
from linear_programming_solver_lpr381_amd import synth

REL = 1e-9      # README "Parity bar": paths that are not bitwise agree in the objective within 1e-9 relative
FEAS = 1e-6     # IsFeasible's tolerance (Models/Branch&Bound.cs)


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_hand_example_event_by_event(oracle):
    T, basis, ub, _ = B.hand_example()
    # event 1: x2 enters (most negative cost), ratios 10/2 = 5 and 15/4 = 3.75, u2 = 3 <= 3.75 -> bound flip of column 1
    st, T1, b1, f1, tr1, k1 = B.run(T, basis, ub, max_iter=1)
    assert st == B.ITER_LIMIT and tr1.tolist() == [[-1, 1]] and k1 == (0, 0, 1)
    assert f1.tolist() == [0, 1, 0, 0, 0] and b1.tolist() == basis.tolist()
    assert T1[:, -1].tolist() == [10.0 - 3 * 2, 15.0 - 3 * 4, 0.0 - 3 * -5.0] and T1[:, 1].tolist() == [-2.0, -4.0, 5.0]
    # event 2: x1 enters, ratios 4/1 and 3/2 -> pivot (1, 0), kind 0
    st, T2, b2, f2, tr2, k2 = B.run(T, basis, ub, max_iter=2)
    assert tr2.tolist() == [[-1, 1], [1, 0]] and k2 == (1, 0, 1) and b2.tolist() == [3, 0]
    # event 3: column 1 (u2 - x2) enters with negative entries in both rows; row 1 (x1, u = 4) reaches its upper bound first
    st, T3, b3, f3, tr3, k3 = B.run(T, basis, ub)
    assert st == B.OPTIMAL
    assert tr3.tolist() == [[-1, 1], [1, 0], [-3, 1]] and k3 == (1, 1, 1)
    assert f3.tolist() == [1, 1, 0, 0, 0] and b3.tolist() == [3, 1]
    x, z, up = B.solution(T3, b3, f3, ub, 3)
    assert x.tolist() == [4.0, 1.75, 0.0] and z == 20.75 and up.tolist() == [1, 0, 0]


@pytest.mark.parametrize("m,n,seed", [(24, 40, 7), (48, 80, 3), (64, 128, 11)])
def test_all_infinite_bounds_is_the_primal_loop(oracle, m, n, seed):
    c, A, b = synth.dense_lp(m, n, seed)
    T, basis = synth.primal_tableau_from(c, A, b)
    To, bo = T.copy(), basis.copy()
    st_o, tr_o = oracle.primal_tableau(To, bo)
    for ub in (None, np.full(T.shape[1] - 1, np.inf)):
        st, Tb, bb, flip, tr, counts = B.run(T, basis, ub)
        assert st == st_o and tr.tolist() == tr_o.tolist()
        assert np.array_equal(_u64(Tb), _u64(To)) and bb.tolist() == bo.tolist()
        assert not flip.any() and counts == (len(tr_o), 0, 0)


def _check_against_rows(oracle, bounded, rows, n):
    T, basis, ub, (c, A0, b0) = bounded
    st, Tb, bb, flip, tr, counts = B.run(T, basis, ub)
    assert st == B.OPTIMAL
    assert min(counts) > 0, counts                       # all three event kinds
    assert sum(counts) == len(tr)
    Tr, br = rows
    st_r, tr_r = oracle.primal_tableau(Tr, br)
    assert st_r == B.OPTIMAL
    x, z, up = B.solution(Tb, bb, flip, ub, n)
    z_rows = Tr[-1, -1]
    rel = abs(z - z_rows) / max(1.0, abs(z_rows))
    print(f"events {len(tr)} (kind0 {counts[0]}, kind1 {counts[1]}, flips {counts[2]}) vs {len(tr_r)} pivots; rel diff {rel:.2e}")
    assert rel <= REL
    assert (A0 @ x <= b0 + FEAS).all() and (x >= -FEAS).all() and (x <= ub[:n] + FEAS).all()
    vb = Tb[:-1, -1]
    assert (vb >= -FEAS).all() and (vb <= ub[bb] + FEAS).all()      # basic values inside their bounds
    assert abs(c @ x - z) <= REL * max(1.0, abs(z))
    return z


@pytest.mark.parametrize("seed", B.BINARY_SEEDS)
@pytest.mark.parametrize("n,m", B.BINARY_SHAPES)
def test_binary_models_match_the_rows_form(oracle, n, m, seed):
    _check_against_rows(oracle, B.binary_bounded(n, m, seed), B.binary_rows(n, m, seed), n)


@pytest.mark.parametrize("m,n", B.DENSE_UNIT_SHAPES)
def test_dense_unit_bounds_match_the_rows_form(oracle, m, n):
    _check_against_rows(oracle, B.dense_unit_bounded(m, n), B.dense_unit_rows(m, n), n)


@pytest.mark.parametrize("n,m,seed", [(40, 20, 1), (128, 64, 2)])
def test_highs_agrees(oracle, n, m, seed):
    from scipy.optimize import linprog
    T, basis, ub, (c, A0, b0) = B.binary_bounded(n, m, seed)
    st, Tb, bb, flip, tr, counts = B.run(T, basis, ub)
    r = linprog(-c, A_ub=A0, b_ub=b0, bounds=[(0, 1)] * n, method="highs")
    assert r.status == 0
    assert abs(-r.fun - Tb[-1, -1]) <= REL * max(1.0, abs(r.fun))
