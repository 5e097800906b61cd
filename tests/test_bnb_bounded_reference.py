"""The NumPy restatement of branch and bound by bound changes (tests/_bnb_bounded_ref.py) against independent answers:
scipy.optimize.milp on 0/1 programs and on small general-integer, shifted, Min, mixed and infeasible models; the cycling node of
binary_bounded(64, 32, 1) with and without the flag; and flags = 0 against the bounded dual restatement.  CPU only; the GPU
tests compare the device against this restatement bit for bit."""
import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bounded_dual_ref as D

REL = 1e-9      # README "Parity bar": paths that are not bitwise agree in the objective within 1e-9 relative
BINARY = [(8, 4, 1), (16, 8, 1), (32, 16, 2), (40, 20, 3), (24, 40, 2), (96, 8, 1)]
NODE_EVENT_BOUND = 1000


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def milp(c, A, rel, b, upper, lower=None, is_int=None, sense=0):
    """(status, optimum in the user's sense) of scipy.optimize.milp; status 2 = infeasible."""
    from scipy.optimize import Bounds, LinearConstraint, milp as _milp
    n = len(c)
    lower = np.zeros(n) if lower is None else lower
    lb = np.where(np.asarray(rel) == 2, b, -np.inf)
    res = _milp(c if sense == 1 else -np.asarray(c), constraints=LinearConstraint(A, lb, b),
                integrality=np.ones(n) if is_int is None else np.asarray(is_int, dtype=float), bounds=Bounds(lower, upper))
    if res.status == 2:
        return N.INFEASIBLE, None
    assert res.status == 0, res.message
    return N.OPTIMAL, (res.fun if sense == 1 else -res.fun)


def _check(out, want_status, want):
    assert out["rc"] == 0 and out["status"] == want_status
    assert out["log"]["events"].max() < NODE_EVENT_BOUND, "a node reached 1000 events"
    assert len(out["log"]) == out["nodes"]
    if want is not None:
        print("optimum", out["value"], "milp", want, "relative", abs(out["value"] - want) / max(1.0, abs(want)))
        assert abs(out["value"] - want) <= REL * max(1.0, abs(want))


@pytest.mark.parametrize("n,m,seed", BINARY)
def test_binary_programs_match_milp(oracle, n, m, seed):
    c, A0, b0 = N.binary_model(n, m, seed)
    out = N.solve(c, A0, b0, np.ones(n))
    st, want = milp(c, A0, np.zeros(m), b0, np.ones(n))
    _check(out, st, want)
    x = out["x"]
    assert np.array_equal(x, np.rint(x)) and (x >= 0).all() and (x <= 1).all() and (A0 @ x <= b0 + 1e-9).all()
    assert abs(float(c @ x) - want) <= REL * max(1.0, abs(want))


@pytest.mark.parametrize("name", ["general", "lowers", "min", "mixed", "infeasible"])
def test_small_models_match_milp(oracle, name):
    c, A, rel, b, upper, lower, is_int, sense = N.small_models()[name]
    out = N.solve(c, A, b, upper, lower=lower, is_int=is_int, sense=sense, rel=rel)
    st, want = milp(c, A, rel, b, upper, lower, is_int, sense)
    assert (st == N.INFEASIBLE) == (name == "infeasible")
    _check(out, st, want)
    if st == N.OPTIMAL:
        x = out["x"]
        ints = np.ones(len(c), dtype=bool) if is_int is None else is_int != 0
        assert np.array_equal(x[ints], np.rint(x[ints])) and (A @ x <= b + 1e-7).all()
        assert (x >= (0 if lower is None else lower) - 1e-9).all() and (x <= upper + 1e-9).all()
        assert abs(float(c @ x) - want) <= 1e-7 * max(1.0, abs(want))
        assert out["nodes"] > 1, "the model is solved at the root: it tests nothing"
    if name == "mixed":
        assert np.abs(x[~ints] - np.rint(x[~ints])).max() > 1e-6, "no continuous variable is fractional at the optimum"
    if name == "lowers":
        assert out["constant"] == float(c @ lower) and out["constant"] != 0.0


def test_cycling_node_cycles_without_the_flag_and_ends_with_it(oracle):
    Tc, bs, ubc, flip = N.cycling_node()
    states = set()
    st, Td, bd, fd, tr, counts = N.dual_run2(Tc, bs, ubc, flip, 0, states=states)
    assert st == N.ITER_LIMIT and len(tr) == 10000 and "repeated" in states
    assert abs(Td[-1, -1] - 445.0) <= REL * 445.0                            # the objective stays there
    st_d = D.dual_run(Tc, bs, ubc, flip)[0]
    assert st_d == D.ITER_LIMIT
    states = set()
    Tz, fz, nflips, bad = N.dualize(Tc, ubc, flip)
    assert bad == 0
    st, Td, bd, fd, tr, counts = N.dual_run2(Tz, bs, ubc, fz, N.SKIP_FIXED, states=states)
    print("flagged: events", len(tr), "dual-feasibility flips", nflips)
    assert st == N.OPTIMAL and len(tr) <= 100 and "distinct" in states
    fixed = np.flatnonzero(ubc == 0.0)
    assert len(fixed) == 31 and not np.isin(tr[:, 1], fixed).any(), "a fixed column entered"
    # the answer is the LP optimum of the node
    c, A0, b0 = N.binary_model(64, 32, 1)
    lw, up = np.zeros(64), np.ones(64)
    lw[list(N.CYCLING_ONES)] = 1.0
    up[list(N.CYCLING_ZEROS)] = 0.0
    hst, obj = D.highs_bounded(c, A0, b0, lw, up)
    assert hst == D.OPTIMAL and abs(Td[-1, -1] - obj) <= REL * abs(obj)


@pytest.mark.parametrize("n,m,seed", [(12, 6, 1), (40, 20, 1), (64, 32, 2)])
def test_flags_zero_is_the_bounded_dual_restatement_bit_for_bit(oracle, n, m, seed):
    _, _, ub, _, Ts, bs, flip = D.root(n, m, seed)
    for j, l, u in D.children(n, m, seed):
        Tc, ubc, _ = D.change_bounds(Ts, ub, np.zeros(len(ub)), flip, [j], [l], [u])
        a = D.dual_run(Tc, bs, ubc, flip)
        b = N.dual_run2(Tc, bs, ubc, flip, 0)
        assert a[0] == b[0] and np.array_equal(_u64(a[1]), _u64(b[1])) and a[2].tolist() == b[2].tolist()
        assert a[3].tolist() == b[3].tolist() and a[4].tolist() == b[4].tolist() and a[5] == b[5]


def test_relaxing_a_fixed_column_needs_the_flips(oracle):
    """Finding 2: after a dive the columns fixed at 0 carry negative reduced costs; relaxing them leaves the tableau dual
    infeasible until lpx_tableau_dualize flips them."""
    out = N.solve(*[N.binary_model(16, 8, 1)[k] for k in (0, 1, 2)], np.ones(16))
    assert out["flips"] > 0 and (out["log"]["flips"] > 0).any()


def test_pick_rule(oracle):
    T = np.zeros((4, 8)); basis = np.array([0, 2, 5], dtype=np.int32)
    T[:3, 7] = [0.25, 0.75, 0.5]; T[3, 7] = 9.0
    ub = np.full(7, np.inf); ub[1] = 1.0
    flip = np.zeros(7, dtype=np.uint8)
    assert N.pick(T, basis, flip, ub, None, 5)["var"] == 0                   # 0.25 and 0.75 tie: the lowest index
    assert N.pick(T, basis, flip, ub, None, 6) == {"var": 5, "candidates": 3, "x_var": 0.5, "z": 9.0}
    assert N.pick(T, basis, flip, ub, None, 6, is_int=[1, 1, 1, 1, 1, 0])["var"] == 0
    flip[1] = 1                                                              # nonbasic at its bound: x = 1, integral
    assert N.pick(T, basis, flip, ub, None, 2)["candidates"] == 1
    assert N.pick(T, basis, flip, ub, None, 1, tol=0.25)["var"] == -1        # f exactly at tol is no candidate
