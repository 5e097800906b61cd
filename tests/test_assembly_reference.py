"""CPU checks of the NumPy restatement of node and child assembly (tests/_assembly_ref.py) against something that is not the
restatement: build_node against BuildTableau of the model with the cut rows appended (synth.primal_tableau_from), bit for bit;
build_child against a cold re-solve of the LP with the bound row appended, by the oracle.  A GPU mismatch in
tests/test_gpu_node_assembly.py then points at the kernel."""
import numpy as np
import pytest

import _assembly_ref as A
from linear_programming_solver_lpr381_amd import synth


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("d", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_build_node_is_build_tableau_of_the_model_with_the_cut_rows(seed, d):
    g = np.random.default_rng(100 * seed + d)
    m, n = int(g.integers(1, 7)), int(g.integers(1, 9))
    Am = g.integers(-3, 10, size=(m, n)).astype(np.float64)
    b = g.integers(0, 30, size=m).astype(np.float64)
    c = g.integers(0, 21, size=n).astype(np.float64)             # zeros among them: -c holds -0.0
    T0, basis0 = synth.primal_tableau_from(c, Am, b)
    var, coef, zero, rhs, rows = [], [], [], [], []
    for k in range(d):
        j, ge = int(g.integers(0, n)), bool((k + seed) % 2)
        row = np.zeros(n)
        row[j] = 1.0
        bound = float(g.integers(0, 4))
        if ge:                                                   # x_j >= c written as -x_j <= -c: the zeros become -0.0
            row *= -1
            bound = -bound
        rows.append(row)
        var.append(j); coef.append(row[j]); zero.append(-0.0 if ge else 0.0); rhs.append(bound)
    want_T, want_b = synth.primal_tableau_from(c, np.vstack([Am] + rows) if d else Am, np.concatenate([b, rhs]))
    T, basis = A.build_node(T0, var, coef, zero, rhs)
    assert T.shape == (m + 1 + d, n + m + 1 + d)
    assert np.array_equal(_u64(T), _u64(want_T)) and basis.tolist() == want_b.tolist()
    if d >= 2:
        assert np.signbit(T[m:m + d, :n]).any() and not np.signbit(T[m:m + d, :n]).all()


def test_build_node_of_the_smallest_root():
    T0 = np.array([[2.0, -0.0, 1.0, 3.0], [-5.0, -0.0, 0.0, 0.0]])
    T, basis = A.build_node(T0, [1, 1], [1.0, -1.0], [0.0, -0.0], [4.0, -1.0])
    want = np.array([[2.0, -0.0, 1.0, 0.0, 0.0, 3.0],
                     [0.0, 1.0, 0.0, 1.0, 0.0, 4.0],
                     [-0.0, -1.0, 0.0, 0.0, 1.0, -1.0],
                     [-5.0, -0.0, 0.0, 0.0, 0.0, 0.0]])
    assert np.array_equal(_u64(T), _u64(want)) and basis.tolist() == [2, 3, 4]


CHILD_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10)


def test_build_child_is_the_lp_with_the_bound_row(oracle):
    """Ten integer-data LPs solved by the oracle, each with a basic fractional structural variable: the LE and the GE child,
    warm from build_child with the dual loop, and cold from the slack basis with the bound row appended, end in the same status
    and the same z to within 1e-9 * max(1, |z|), the margin the warm-started search is held to."""
    both_feasible = 0
    for seed in CHILD_SEEDS:
        c, Am, b = A.binary_relaxation(seed)
        n = len(c)
        Tp, bp = synth.primal_tableau_from(c, Am, b)
        st, _ = oracle.primal_tableau(Tp, bp)
        assert st == oracle.OPTIMAL
        pick = A.fractional_row(Tp, bp, n)
        assert pick is not None, "seed %d: the LP optimum is integral" % seed
        var, ik = pick
        v = Tp[ik, -1]
        feasible = 0
        for is_ge, bound in ((0, np.floor(v)), (1, np.ceil(v))):
            T, basis = A.build_child(Tp, bp, var, ik, is_ge, bound)
            assert T[len(bp), -1] < 0.0, "the branching row must cut the parent's optimum off"
            warm, _, _ = oracle.dual_tableau(T, basis, fdf_guard=0)
            row = np.zeros(n)
            row[var] = 1.0
            if is_ge:
                row *= -1
            Tc, bc = synth.primal_tableau_from(c, np.vstack([Am, row]), np.concatenate([b, [-bound if is_ge else bound]]))
            if is_ge:
                cold, _, _ = oracle.dual_tableau(Tc, bc, fdf_guard=10000, cleanup=1)
            else:
                cold, _ = oracle.primal_tableau(Tc, bc)
            assert warm == cold, (seed, is_ge, warm, cold)
            assert warm in (oracle.OPTIMAL, oracle.INFEASIBLE)
            if warm == oracle.OPTIMAL:
                zw, zc = T[-1, -1], Tc[-1, -1]
                assert abs(zw - zc) <= 1e-9 * max(1.0, abs(zc)), (seed, is_ge, zw, zc)
                xw, _ = A.solution(T, basis, n)
                assert abs(xw @ c - zc) <= 1e-9 * max(1.0, abs(zc))
                assert xw[var] >= bound - 1e-9 if is_ge else xw[var] <= bound + 1e-9
                feasible += 1
        both_feasible += feasible == 2
    assert both_feasible >= 8, both_feasible


def test_solution_reads_the_rhs_through_the_basis():
    T = np.array([[0.0, 0.0, 0.0, 1.5], [0.0, 0.0, 0.0, -0.0], [0.0, 0.0, 0.0, 7.0], [0.0, 0.0, 0.0, -2.25]])
    x, z = A.solution(T, np.array([2, 0, 5], dtype=np.int32), 3)
    assert _u64(x).tolist() == _u64(np.array([-0.0, 0.0, 1.5])).tolist() and z == -2.25
    x, z = A.solution(T, np.array([2, 0, 5], dtype=np.int32), 0)
    assert x.shape == (0,) and z == -2.25
