"""CPU checks of the GMI cutting-plane definitions themselves (include/lpx.h, lpx_tableau_gmi_round / lpx_solve_cuts),
through the numpy restatement in tests/_gmi_ref.py on the CPU oracle: known answers, validity of every cut on enumerated
integer points, separation of the LP point, a monotone bound, and agreement with scipy's MILP when the loop closes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gmi_ref as G                          # noqa: E402


KATS = [
    # (sense, c, A, rel, b, status, LP bound, IP value, x or None, rounds or None)
    (G.MAX, [7, 10], [[-1, 3], [7, 1]], [G.LE, G.LE], [6, 35], G.CUT_INTEGER, 66.5, 58.0, [4, 3], None),
    (G.MIN, [1, 1], [[2, 2]], [G.GE], [3], G.CUT_INTEGER, 1.5, 2.0, None, None),
    (G.MAX, [1, 1], [[2, 2]], [G.EQ], [3], G.INFEASIBLE, 1.5, None, None, None),
    (G.MAX, [1, 1], [[1, 0], [0, 1]], [G.LE, G.LE], [2, 3], G.CUT_INTEGER, 5.0, 5.0, [2, 3], 0),
]


@pytest.mark.parametrize("case", range(len(KATS)))
def test_known_answers(oracle, case):
    s, c, A, rel, b, status, lp, ip, x, rounds = KATS[case]
    r = G.gmi_solve(oracle, s, np.array(c, float), np.array(A, float), rel, np.array(b, float))
    assert r.status == status
    assert r.root_z == pytest.approx(lp, abs=1e-9)
    if ip is not None:
        assert r.z == pytest.approx(ip, abs=1e-9)
    if x is not None:
        assert np.allclose(r.x, x, atol=1e-9)
    if rounds is not None:
        assert r.rounds == rounds and r.added == 0 and len(r.cuts) == 0


def _ub(A, rel, b, n):
    ub = np.full(n, np.inf)
    for a, r, bi in zip(A, rel, b):
        if r == G.LE and np.all(a >= 0):
            for j in range(n):
                if a[j] > 0:
                    ub[j] = min(ub[j], np.floor(bi / a[j]))
    return ub


@pytest.mark.parametrize("seed", range(30))
def test_random_ips_cuts_valid_separating_and_bound(oracle, seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(2, 7))
    m = int(rng.integers(1, 4))
    s, c, A, rel, b = G.random_ip(rng, n, m, ub=int(rng.integers(2, 5)))
    r = G.gmi_solve(oracle, s, c, A, rel, b, G.CutOpts(cuts_per_round=int(rng.integers(1, 9))))
    pts = G.enumerate_points(A, rel, b, _ub(A, rel, b, n))
    assert len(pts) > 0
    # validity: every integer-feasible point satisfies every cut (x-space LE rows)
    if len(r.cuts):
        viol = pts @ r.cuts[:, :n].T - r.cuts[:, n]
        assert viol.max() <= 1e-6, viol.max()
    # separation: each round's cuts are violated by the LP point they were cut from (by 1 in exact arithmetic)
    k = 0
    for rows, xlp in zip(r.src_rows, r.lp_points):
        for _ in rows:
            assert r.cuts[k, :n] @ xlp - r.cuts[k, n] > 0.5
            k += 1
    # the bound never increases (Max model), from the root on
    bounds = [r.root_z] + r.bounds
    assert all(bounds[i + 1] <= bounds[i] + 1e-9 for i in range(len(bounds) - 1))
    best = max(c @ p for p in pts)
    assert r.z >= best - 1e-6
    if r.status == G.CUT_INTEGER:
        from scipy.optimize import Bounds, LinearConstraint, milp
        lo = np.where(np.array(rel) == G.GE, b, -np.inf)
        hi = np.where(np.array(rel) == G.GE, np.inf, b)
        sol = milp(-c, constraints=LinearConstraint(A, lo, hi), integrality=np.ones(n), bounds=Bounds(0, np.inf))
        assert sol.status == 0
        assert r.z == pytest.approx(-sol.fun, abs=1e-6)
        assert r.z == pytest.approx(best, abs=1e-6)


def test_round_shapes_purge_and_capacity(oracle):
    """One round on a solved LP: cut rows above the objective, slacks before the RHS, the spec's entries; then a purge."""
    found_purge = False
    for seed in range(40):
        s, c, A, rel, b = G.random_ip(np.random.default_rng(seed), 5, 3)
        cp, Ap, bp = G.prepare(s, c, A, rel, b)
        T, basis = G.build_tableau(cp, Ap, bp)
        if not np.all(T[:-1, -1] >= 0):
            continue
        oracle.primal_tableau(T, basis)
        R, C = T.shape
        is_int = np.ones(C - 1, np.uint8)
        o = G.CutOpts(cuts_per_round=3)
        T1, b1, src, pcol = G.gmi_round(T, basis, is_int, C - 1, C - 1, o, R + 2, C + 2)   # capacity caps K at 2
        K = len(src)
        assert K <= 2 and pcol == []
        if K == 0:
            continue
        assert T1.shape == (R + K, C + K)
        assert np.array_equal(T1[-1, :C - 1], T[-1, :C - 1]) and T1[-1, -1] == T[-1, -1]
        assert np.all(T1[R - 1:R - 1 + K, -1] == -1.0)
        assert list(b1[R - 1:]) == [C - 1 + k for k in range(K)]
        assert not np.any(np.signbit(T1[R - 1:R - 1 + K]) & (T1[R - 1:R - 1 + K] == 0))
        T1 = np.ascontiguousarray(T1)
        st, _, _ = oracle.dual_tableau(T1, b1, fdf_guard=0, cleanup=1)
        if st != G.OPTIMAL:
            continue
        T2, b2, src2, pcol2 = G.gmi_round(T1, b1, is_int, C - 1, C - 1, G.CutOpts(), R + 64, C + 64)
        if pcol2:
            found_purge = True
            P = len(pcol2)
            assert T2.shape == (T1.shape[0] - P + len(src2), T1.shape[1] - P + len(src2))
            assert all(C - 1 <= p < T1.shape[1] - 1 for p in pcol2)
            break
    assert found_purge
