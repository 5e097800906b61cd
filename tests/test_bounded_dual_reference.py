"""The NumPy restatement of the bounded dual simplex and of the bound change (tests/_bounded_dual_ref.py) against independent
answers: SciPy/HiGHS on covering models (both event kinds), on infeasible ones, on the children of solved 0/1 roots and on a
four-column change, and the oracle's dual loop when no column is bounded.  CPU only; the GPU tests compare the device against
this restatement bit for bit."""
import numpy as np
import pytest

import _bounded_dual_ref as D
import _bounded_ref as B

REL = 1e-9      # README "Parity bar": paths that are not bitwise agree in the objective within 1e-9 relative
COVERING = [(6, 12, 1), (20, 40, 1), (64, 128, 2), (128, 256, 3)]


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _close(got, want):
    print("objective", got, "HiGHS", want, "relative", abs(got - want) / max(1.0, abs(want)))
    assert abs(got - want) <= REL * max(1.0, abs(want))


@pytest.mark.parametrize("m,n,seed", COVERING)
def test_covering_matches_highs_with_both_kinds(oracle, m, n, seed):
    T, basis, ub, (c, A, b) = D.covering(m, n, seed)
    st, Td, bd, flip, tr, counts = D.dual_run(T, basis, ub)
    assert st == D.OPTIMAL and counts[0] > 0 and counts[1] > 0 and counts[2] == 0 and sum(counts) == len(tr)
    x, z, _ = B.solution(Td, bd, flip, ub, n)
    assert (x >= -1e-7).all() and (x <= 1 + 1e-7).all() and (A @ x >= b - 1e-7).all()
    hst, obj = D.highs_bounded(c, -A, -b, np.zeros(n), np.ones(n), maximise=False)
    assert hst == D.OPTIMAL
    _close(-z, obj)                  # the tableau maximises -c.x
    _close(float(c @ x), obj)


@pytest.mark.parametrize("m,n,seed", COVERING)
def test_covering_with_tight_bounds_is_infeasible_on_both_sides(oracle, m, n, seed):
    T, basis, ub, (c, A, b) = D.covering(m, n, seed, u=0.1)
    st, Td, bd, flip, tr, counts = D.dual_run(T, basis, ub)
    assert st == D.INFEASIBLE
    hst, _ = D.highs_bounded(c, -A, -b, np.zeros(n), np.full(n, 0.1), maximise=False)
    assert hst == D.INFEASIBLE


def _edit_and_solve(n, m, seed, cols, lower, upper):
    T0, b0, ub, (c, A0, rhs0), Ts, bs, flip = D.root(n, m, seed)
    Tc, ubc, lo = D.change_bounds(Ts, ub, np.zeros(len(ub)), flip, cols, lower, upper)
    st, Td, bd, fd, tr, counts = D.dual_run(Tc, bs, ubc, flip)
    lw, up = np.zeros(n), np.ones(n)
    lw[cols], up[cols] = lower, upper
    return st, D.solution(Td, bd, fd, ubc, lo, n), D.highs_bounded(c, A0, rhs0, lw, up), (lw, up, A0, rhs0, c)


@pytest.mark.parametrize("seed", (1, 2))
@pytest.mark.parametrize("n,m", B.BINARY_SHAPES)
def test_children_of_binary_roots_match_highs(oracle, n, m, seed):
    kids = D.children(n, m, seed)
    assert len(kids) in (2, 4, 6) and (len(kids) == 6 or n == 12)       # the smallest root has fewer than three fractional variables
    for j, l, u in kids:
        st, (x, z, _), (hst, obj), (lw, up, A0, rhs0, c) = _edit_and_solve(n, m, seed, [j], [l], [u])
        assert st == D.OPTIMAL and hst == D.OPTIMAL
        assert abs(x[j] - l) <= 1e-7 and (x >= lw - 1e-7).all() and (x <= up + 1e-7).all() and (A0 @ x <= rhs0 + 1e-6).all()
        _close(z, obj)
        _close(float(c @ x), obj)


def test_four_column_change_matches_highs(oracle):
    cols, lower, upper = D.four_column_change()
    flip = D.root(64, 32, 1)[6]
    assert len(cols) == 4 and flip[cols].any(), "one of the four columns is flipped in the root"
    st, (x, z, _), (hst, obj), (lw, up, A0, rhs0, c) = _edit_and_solve(64, 32, 1, cols, lower, upper)
    assert st == D.OPTIMAL and hst == D.OPTIMAL
    assert np.abs(x[cols] - lower).max() <= 1e-7 and (A0 @ x <= rhs0 + 1e-6).all()
    _close(z, obj)


@pytest.mark.parametrize("m,n,seed", COVERING[:3])
def test_all_infinite_bounds_is_the_oracle_dual_loop(oracle, m, n, seed):
    T, basis, _, _ = D.covering(m, n, seed)
    To, bo = T.copy(), basis.copy()
    st_o, tr_o, nf = oracle.dual_tableau(To, bo, fdf_guard=0, cleanup=0)
    assert nf == 0 and len(tr_o) > 0
    for ub in (None, np.full(T.shape[1] - 1, np.inf)):
        st, Td, bd, flip, tr, counts = D.dual_run(T, basis, ub)
        assert st == st_o and tr.tolist() == tr_o.tolist()
        assert np.array_equal(_u64(Td), _u64(To)) and bd.tolist() == bo.tolist()
        assert not flip.any() and counts == (len(tr_o), 0, 0)


def test_change_with_zero_shift_moves_nothing(oracle):
    _, _, ub, _, Ts, bs, flip = D.root(40, 20, 1)
    j = int(np.flatnonzero(flip[:40])[0])
    Tc, ubc, lo = D.change_bounds(Ts, ub, np.zeros(len(ub)), flip, [j], [0.0], [1.0])      # flipped: s = ub - u' = 0
    assert np.array_equal(_u64(Tc), _u64(Ts)) and ubc[j] == 1.0 and lo[j] == 0.0
