"""CPU checks of the post-optimal edit definitions (include/lpx.h, lpx_tableau_rhs_update / _objective_update /
_add_column / _add_row and the lpx_session_* mapping), through the numpy restatement tests/_postopt_ref.py on the CPU
oracle: after the follow-up oracle run, each edit reaches the optimum of the edited model, as SciPy / HiGHS finds it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _postopt_ref as P                      # noqa: E402

scipy_opt = pytest.importorskip("scipy.optimize")


def highs(sense, c, A, rel, b):
    """(status, z, x) of the model by HiGHS; status uses the LPX codes."""
    c = np.asarray(c, float)
    A = np.asarray(A, float).reshape(len(b), len(c))
    rel = list(rel)
    ub = [A[i] if r == P.LE else -A[i] for i, r in enumerate(rel) if r != P.EQ]
    bu = [b[i] if r == P.LE else -b[i] for i, r in enumerate(rel) if r != P.EQ]
    eq = [A[i] for i, r in enumerate(rel) if r == P.EQ]
    be = [b[i] for i, r in enumerate(rel) if r == P.EQ]
    obj = -c if sense == P.MAX else c
    r = scipy_opt.linprog(obj, A_ub=np.array(ub) if ub else None, b_ub=np.array(bu) if bu else None,
                          A_eq=np.array(eq) if eq else None, b_eq=np.array(be) if be else None,
                          bounds=[(0, None)] * len(c), method="highs")
    if r.status == 2:
        return P.INFEASIBLE, None, None
    if r.status == 3:
        return P.UNBOUNDED, None, None
    assert r.status == 0, r.message
    return P.OPTIMAL, (-r.fun if sense == P.MAX else r.fun), r.x


def model_of(S):
    return S.sense, S.c, [list(a) for a in S.A], S.rel, S.b


def check_against_highs(S, st):
    hs, hz, hx = highs(*model_of(S))
    assert st == hs, (st, hs)
    if st == P.OPTIMAL:
        x, z = S.solution()
        assert z == pytest.approx(hz, rel=1e-9, abs=1e-9)
        A = np.asarray(S.A, float)
        # x is feasible for the edited model
        for i, r in enumerate(S.rel):
            v = A[i] @ x
            if r == P.LE:
                assert v <= S.b[i] + 1e-7
            elif r == P.GE:
                assert v >= S.b[i] - 1e-7
            else:
                assert v == pytest.approx(S.b[i], abs=1e-7)
        assert (x >= -1e-9).all()


def test_segment_order_is_the_header_rule():
    rng = np.random.default_rng(5)
    T = rng.standard_normal((5, 200))
    cols = np.arange(150)
    v = rng.standard_normal(150)
    base = T[:, -1].copy()
    out = P.col_combination(T, base, cols, v)
    exp = base.copy()
    for s0 in range(0, 150, P.SEG):
        for i in range(5):
            s = 0.0
            for k in range(s0, min(150, s0 + P.SEG)):
                s = s + float(v[k]) * float(T[i, cols[k]])
            exp[i] = exp[i] + s
    assert np.array_equal(out.view(np.uint64), exp.view(np.uint64))
    assert np.array_equal(P.col_combination(T, base, [], []).view(np.uint64), base.view(np.uint64))


EXAMPLE = (P.MAX, [3.0, 5.0], [[1, 0], [0, 2], [3, 2]], [P.LE, P.LE, P.LE], [4.0, 12.0, 18.0])


@pytest.mark.parametrize("edit,x,z,warm_pivots", [
    (("rhs", [2], [20.0]), [8 / 3, 6], 38.0, 0),
    (("rhs", [2], [30.0]), [4, 6], 42.0, None),
    (("cost", [0], [10.0]), [4, 3], 55.0, None),
    (("row", [1, 1], P.LE, 7.0), [1, 6], 33.0, None),
    (("col", 6.0, [0, 1, 1]), [2, 0, 12], 78.0, None),
])
def test_known_answers_on_the_example(oracle, edit, x, z, warm_pivots):
    S = P.Session(oracle, *EXAMPLE)
    assert S.status == P.OPTIMAL and S.solution()[1] == 36.0
    kind = edit[0]
    if kind == "rhs":
        st = S.set_rhs(edit[1], edit[2])
    elif kind == "cost":
        st = S.set_cost(edit[1], edit[2])
    elif kind == "row":
        st = S.add_constraint(edit[1], edit[2], edit[3])
    else:
        st = S.add_variable(edit[1], edit[2])
    assert st == P.OPTIMAL and S.warm == 1
    xs, zs = S.solution()
    assert np.allclose(xs, x, atol=1e-12) and zs == pytest.approx(z, abs=1e-12)
    if warm_pivots is not None:
        assert len(S.trace) == warm_pivots


def random_model(rng, n, m):
    sense = int(rng.integers(0, 2))
    A = rng.uniform(0.5, 3.0, size=(m, n))
    x0 = rng.uniform(0.5, 2.0, size=n)
    rel = [int(r) for r in rng.choice([P.LE, P.LE, P.GE, P.EQ], size=m)]
    b = A @ x0
    b = np.where(np.asarray(rel) == P.LE, b * rng.uniform(1.0, 1.3, m), np.where(np.asarray(rel) == P.GE, b * rng.uniform(0.7, 1.0, m), b))
    c = rng.uniform(0.5, 2.0, size=n) * (1 if sense == P.MAX else 1)
    if sense == P.MAX:
        # bounded: every variable sits in some <= row with positive coefficients
        rel[0] = P.LE
    return sense, c, A, rel, b


def random_edit(rng, S):
    k = int(rng.integers(0, 4))
    n, m = len(S.c), len(S.b)
    if k == 0:
        i = int(rng.integers(0, m))
        return S.set_rhs([i], [S.b[i] * float(rng.uniform(0.5, 1.6))])
    if k == 1:
        j = int(rng.integers(0, n))
        return S.set_cost([j], [S.c[j] * float(rng.uniform(0.3, 2.5))])
    if k == 2:
        return S.add_variable(float(rng.uniform(0.5, 2.5)), rng.uniform(0.2, 3.0, size=m))
    a = rng.uniform(0.2, 3.0, size=n)
    x, _ = S.solution()
    rel = [P.LE, P.GE, P.EQ][int(rng.integers(0, 3))]
    b = float(a @ x) * float(rng.uniform(0.7, 1.1))
    return S.add_constraint(a, rel, b)


@pytest.mark.parametrize("seed", range(12))
def test_random_edit_sequences_reach_the_edited_optimum(oracle, seed):
    rng = np.random.default_rng(700 + seed)
    n, m = int(rng.integers(3, 8)), int(rng.integers(2, 6))
    S = P.Session(oracle, *random_model(rng, n, m))
    check_against_highs(S, S.status)
    for _ in range(6):
        st = random_edit(rng, S)
        check_against_highs(S, st)


def test_infeasible_and_unbounded_then_cold(oracle):
    S = P.Session(oracle, *EXAMPLE)
    S.add_constraint([1.0, 1.0], P.GE, 20.0)           # x1 <= 4, x2 <= 6: x1 + x2 >= 20 is infeasible
    assert S.status == P.INFEASIBLE and S.warm == 1
    st = S.set_rhs([3], [8.0])                          # from the infeasible state: cold
    assert S.warm == 0
    check_against_highs(S, st)
    U = P.Session(oracle, P.MAX, [1.0, 1.0], [[1.0, -1.0]], [P.LE], [2.0])
    assert U.status == P.UNBOUNDED
    st = U.add_constraint([0.0, 1.0], P.LE, 3.0)        # cold, now bounded
    assert U.warm == 0 and st == P.OPTIMAL
    check_against_highs(U, st)
    st = U.set_cost([1], [-1.0])
    check_against_highs(U, st)
    st = U.set_rhs([0], [-5.0])                         # x1 - x2 <= -5 with x2 <= 3: infeasible (dual pivots)
    assert st == P.INFEASIBLE
    check_against_highs(U, st)


def test_cost_change_that_opens_a_ray(oracle):
    S = P.Session(oracle, P.MAX, [1.0, 0.0], [[1.0, 0.0]], [P.LE], [2.0])
    assert S.status == P.OPTIMAL
    st = S.set_cost([1], [0.5])                         # x2 now pays and no row bounds it
    assert st == P.UNBOUNDED and S.warm == 1
    check_against_highs(S, st)
