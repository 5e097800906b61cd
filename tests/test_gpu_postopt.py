"""GPU checks of the post-optimal edits (include/lpx.h, lpx_postopt.hip and lpx_session_*):
1. the four tableau operations bit for bit against the numpy restatement tests/_postopt_ref.py (ragged shapes, ld padding,
   every segment edge, handles of different capacity, untouched regions, the headline shape);
2. hand-derived known answers on integration/Input/example_input.txt, each edit alone and in sequence;
3. random mixed models under mixed edit sequences against a cold lpx_solve of the edited model and HiGHS, through
   INFEASIBLE / UNBOUNDED states and the cold path;
4. config-2 size, 20 mixed edits against cold solves;
5. session details: the open is Primal Simplex bit for bit on all-<= models, capacity exhaustion, ranging, the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _postopt_ref as P                      # noqa: E402
from test_gpu_ranging import ref_ranging      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
EXAMPLE = os.path.join(ROOT, "integration", "Input", "example_input.txt")
SEG = P.SEG


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _solved_tableau(lpx, R, C, seed, pivots=None):
    """A primal-feasible tableau of m = R-1 rows and C columns: a random all-<= model after some primal pivots."""
    from oracle import oracle as O
    g = np.random.default_rng(seed)
    m, n = R - 1, C - R
    A = g.uniform(0.0, 1.0, size=(m, n))
    b = g.uniform(0.5 * n, 0.6 * n, size=m)
    c = g.uniform(0.5, 1.5, size=n)
    T = np.zeros((R, C))
    T[:m, :n] = A
    T[np.arange(m), n + np.arange(m)] = 1.0
    T[:m, -1] = b
    T[m, :n] = -c
    basis = np.arange(n, n + m, dtype=np.int32)
    O.primal_tableau(T, basis, max_iter=pivots if pivots is not None else min(m, 40))
    return T, basis


SHAPES = [(7, 19), (33, 77), (70, 131), (130, 301)]      # C not a multiple of 16; ld padded


def _terms(g, K, lo, hi):
    idx = g.integers(lo, hi, size=K).astype(np.int32)
    return idx, g.standard_normal(K)


@pytest.mark.parametrize("R,C", SHAPES)
@pytest.mark.parametrize("cap", [(0, 0), (3, 45)])
def test_tableau_ops_bitwise(gpu, R, C, cap):
    T, basis = _solved_tableau(gpu, R, C, seed=R * 7 + C)
    m = R - 1
    g = np.random.default_rng(R + C)
    Rcap, Ccap = R + 2 + cap[0], C + 2 + cap[1]
    for K in sorted({0, 1, SEG - 1, SEG, SEG + 1, m}):
        # RHS update (terms on any non-RHS column, repeats allowed)
        cols, v = _terms(g, K, 0, C - 1)
        Tw, bw = P.rhs_update(T, basis, cols, v)
        with gpu.DeviceTableau.with_capacity(T, basis, Rcap, Ccap) as dt:
            dt.rhs_update(cols, v)
            Tg, bg = dt.download()
        assert _same(Tg, Tw) and np.array_equal(bg, bw), ("rhs", K)
        assert _same(Tg[:, :-1], T[:, :-1])                           # only the RHS column moves
        # new column
        obj = float(g.standard_normal())
        Tw, bw = P.add_column(T, basis, cols, v, obj)
        with gpu.DeviceTableau.with_capacity(T, basis, Rcap, Ccap) as dt:
            dt.add_column(cols, v, obj)
            assert (dt.R, dt.C) == (R, C + 1)
            Tg, bg = dt.download()
        assert _same(Tg, Tw) and np.array_equal(bg, bw), ("col", K)
        # objective update with sparse deltas on nonbasic columns
        rows, w = _terms(g, K, 0, m)
        nb = np.setdiff1d(np.arange(C - 1), basis)
        dcols = g.choice(nb, size=min(3, len(nb)), replace=False).astype(np.int32)
        dd = g.standard_normal(len(dcols))
        Tw, bw = P.objective_update(T, basis, rows, w, dcols, dd)
        with gpu.DeviceTableau.with_capacity(T, basis, Rcap, Ccap) as dt:
            dt.objective_update(rows, w, dcols, dd)
            Tg, bg = dt.download()
        assert _same(Tg, Tw) and np.array_equal(bg, bw), ("obj", K)
        assert _same(Tg[:m], T[:m])                                   # only the objective row moves
        # new row
        base = g.standard_normal(C + 1)
        base[C - 1] = 1.0
        Tw, bw = P.add_row(T, basis, rows, w, base)
        with gpu.DeviceTableau.with_capacity(T, basis, Rcap, Ccap) as dt:
            dt.add_row(rows, w, base)
            assert (dt.R, dt.C) == (R + 1, C + 1)
            Tg, bg = dt.download()
        assert _same(Tg, Tw) and np.array_equal(bg, bw), ("row", K)


def test_ops_leave_the_snapshot_and_fail_cleanly_without_capacity(gpu):
    T, basis = _solved_tableau(gpu, 33, 77, seed=4)
    with gpu.DeviceTableau.from_host(T, basis) as dt:          # exact capacity: no room to grow
        dt.snapshot()
        with pytest.raises(gpu.LpxError) as e:
            dt.add_column([0], [1.0], 0.0)
        assert e.value.code == gpu._lib.EINVAL
        with pytest.raises(gpu.LpxError):
            dt.add_row([0], [1.0], np.zeros(78))
        with pytest.raises(gpu.LpxError):
            dt.rhs_update([76], [1.0])                             # the RHS column itself is no term
        with pytest.raises(gpu.LpxError):
            dt.objective_update([], [], [3, 3], [1.0, 1.0])        # repeated delta column
        Tg, _ = dt.download()
        assert _same(Tg, T)
        dt.rhs_update([40], [2.0])
        dt.restore()
        Tg, _ = dt.download()
        assert _same(Tg, T)


@pytest.fixture(scope="module")
def headline(gpu):
    from linear_programming_solver_lpr381_amd import synth
    c, A, b = synth.dense_lp(4096, 8192)
    T0, basis0 = synth.primal_tableau_from(c, A, b)
    del A
    with gpu.DeviceTableau.from_host(T0, basis0) as dt:
        del T0
        status, st = dt.primal_run(max_iter=200)
        assert st["pivots"] == 200
        T, basis = dt.download()
    return T, basis


def test_headline_objective_update_all_rows(gpu, headline):
    T, basis = headline
    m = T.shape[0] - 1
    g = np.random.default_rng(11)
    rows, w = np.arange(m, dtype=np.int32), g.standard_normal(m)
    Tw, _ = P.objective_update(T, basis, rows, w)
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        dt.objective_update(rows, w)
        Tg, _ = dt.download()
    assert _same(Tg[m], Tw[m])
    assert _same(Tg[:m], T[:m])


def test_headline_rhs_update_all_slacks(gpu, headline):
    T, basis = headline
    R, C = T.shape
    m, n = R - 1, C - R
    g = np.random.default_rng(12)
    cols, v = np.arange(n, n + m, dtype=np.int32), g.standard_normal(m)
    Tw, _ = P.rhs_update(T, basis, cols, v)
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        dt.rhs_update(cols, v)
        Tg, _ = dt.download()
    assert _same(Tg[:, -1], Tw[:, -1])
    assert _same(Tg[:, :-1], T[:, :-1])


# ---- 2. known answers -----------------------------------------------------------------------------------------------
def _example(lpx):
    return lpx.ParseFromText(open(EXAMPLE).read())


KATS = [
    ("rhs", (2, 20.0), [8 / 3, 6], 38.0),
    ("rhs", (2, 30.0), [4, 6], 42.0),
    ("cost", (0, 10.0), [4, 3], 55.0),
    ("row", ([1.0, 1.0], 0, 7.0), [1, 6], 33.0),
    ("col", (6.0, [0.0, 1.0, 1.0]), [2, 0, 12], 78.0),
]


def _apply(ses, kind, args):
    if kind == "rhs":
        return ses.ChangeRHS(*args)
    if kind == "cost":
        return ses.ChangeCost(*args)
    if kind == "row":
        return ses.AddConstraint(*args)
    return ses.AddActivity(*args)


@pytest.mark.parametrize("case", range(len(KATS)))
def test_known_answers(gpu, case):
    kind, args, x, z = KATS[case]
    with gpu.LPSolver().Open(_example(gpu)) as ses:
        assert ses.Result.Status == 0 and ses.Result.OptimalValue == 36.0
        r = _apply(ses, kind, args)
        assert r.Status == 0 and r.Aux[0] == 1.0
        assert np.allclose(r.Solution, x, atol=1e-12) and r.OptimalValue == pytest.approx(z, abs=1e-12)
        if case == 0:
            assert len(r.Trace) == 0                               # b3 = 20 stays inside the range [12, 24]
        if case == 1:
            assert len(r.Trace) > 0                                # past the ranged 24: dual pivots


def test_known_answers_in_sequence(gpu):
    with gpu.LPSolver().Open(_example(gpu)) as ses:
        # each KAT from the previous state: compare with a cold solve of the model as it stands
        for kind, args, _, _ in KATS:
            if kind == "col":                                      # one coefficient per constraint, the added row's too
                args = (args[0], list(args[1]) + [0.0])
            r = _apply(ses, kind, args)
            cold = gpu.LPSolver(dual_flags=7).Solve(ses.Problem, "Dual Simplex")
            assert r.Status == cold.Status == 0
            assert r.OptimalValue == pytest.approx(cold.OptimalValue, rel=1e-12)
        # max 10x1 + 5x2 + 6x3, x1 <= 4, 2x2 + x3 <= 12, 3x1 + 2x2 + x3 <= 30, x1 + x2 <= 7
        assert r.OptimalValue == pytest.approx(112.0, abs=1e-9)
        assert np.allclose(r.Solution, [4, 0, 12], atol=1e-9)


# ---- 3. random models -----------------------------------------------------------------------------------------------
def _highs(prob):
    from test_postopt_reference import highs
    return highs(int(prob.ObjectiveSense), list(prob.C), [list(k.A) for k in prob.Constraints],
                 [int(k.Relation) for k in prob.Constraints], [k.B for k in prob.Constraints])


def _check(gpu, ses, r):
    prob = ses.Problem
    cold = gpu.LPSolver(dual_flags=7).Solve(prob, "Dual Simplex")
    hs, hz, hx = _highs(prob)
    assert r.Status == hs, (r.Status, hs)
    assert cold.Status == hs
    if hs == 0:
        assert r.OptimalValue == pytest.approx(hz, rel=1e-9, abs=1e-9)
        # lpx_solve reports the prepared (Max) model's z, as the reference's DualSimplex does: -z for a Min model
        zc = -cold.OptimalValue if int(prob.ObjectiveSense) == 1 else cold.OptimalValue
        assert r.OptimalValue == pytest.approx(zc, rel=1e-9, abs=1e-9)
        assert np.allclose(r.Solution, hx, atol=1e-7)


def _random_model(gpu, rng, n, m):
    from test_postopt_reference import random_model
    s, c, A, rel, b = random_model(rng, n, m)
    return gpu.LPProblem.from_arrays(s, c, A, rel, b)


def _random_edit(rng, ses, allow_bad=True):
    prob = ses.Problem
    n, m = prob.NumVars, len(prob.Constraints)
    k = int(rng.integers(0, 4))
    if k == 0:
        i = int(rng.integers(0, m))
        return ses.ChangeRHS(i, prob.Constraints[i].B * float(rng.uniform(0.5, 1.6)))
    if k == 1:
        j = int(rng.integers(0, n))
        return ses.ChangeCost(j, prob.C[j] * float(rng.uniform(0.3, 2.5)))
    if k == 2:
        return ses.AddActivity(float(rng.uniform(0.5, 2.5)), rng.uniform(0.2, 3.0, size=m))
    a = rng.uniform(0.2, 3.0, size=n)
    x = ses.Result.Solution if ses.Result.Status == 0 else np.ones(n)
    rel = int(rng.integers(0, 3))
    return ses.AddConstraint(a, rel, float(a @ x) * float(rng.uniform(0.7, 1.1)))


@pytest.mark.parametrize("seed", range(8))
def test_random_models_and_edit_sequences(gpu, seed):
    rng = np.random.default_rng(900 + seed)
    prob = _random_model(gpu, rng, int(rng.integers(4, 12)), int(rng.integers(3, 8)))
    with gpu.LPSolver().Open(prob, extra_rows=32, extra_cols=32) as ses:
        _check(gpu, ses, ses.Result)
        for _ in range(7):
            r = _random_edit(rng, ses)
            _check(gpu, ses, r)


def test_infeasible_and_unbounded_states_then_cold(gpu):
    with gpu.LPSolver().Open(_example(gpu)) as ses:
        r = ses.AddConstraint([1.0, 1.0], 1, 20.0)                # infeasible: the empty set
        assert r.Status == gpu._lib.INFEASIBLE and r.Aux[0] == 1.0
        _check(gpu, ses, r)
        r = ses.ChangeRHS(3, 8.0)                                  # from INFEASIBLE: rebuilt and solved cold
        assert r.Aux[0] == 0.0
        _check(gpu, ses, r)
        r = ses.ChangeRHS(3, 6.0)                                  # warm again
        assert r.Aux[0] == 1.0
        _check(gpu, ses, r)
    prob = gpu.LPProblem.from_arrays(0, [1.0, 0.0], [[1.0, 0.0]], [0], [2.0])
    with gpu.LPSolver().Open(prob) as ses:
        r = ses.ChangeCost(1, 0.5)                                 # opens a ray
        assert r.Status == gpu._lib.UNBOUNDED and r.Aux[0] == 1.0
        _check(gpu, ses, r)
        r = ses.AddConstraint([0.0, 1.0], 0, 3.0)                  # from UNBOUNDED: cold, bounded again
        assert r.Status == 0 and r.Aux[0] == 0.0
        _check(gpu, ses, r)
        assert r.OptimalValue == pytest.approx(3.5)


# ---- 4. config 2 ----------------------------------------------------------------------------------------------------
def test_config2_twenty_mixed_edits(gpu):
    from linear_programming_solver_lpr381_amd import synth
    c, A, b = synth.dense_lp(1024, 2048)
    prob = gpu.LPProblem.from_arrays(0, c, A, [0] * 1024, b)
    rng = np.random.default_rng(2)
    with gpu.LPSolver().Open(prob) as ses:
        assert ses.Result.Status == 0
        for e in range(20):
            k = e % 4
            if k == 0:
                i = int(rng.integers(0, 1024))
                r = ses.ChangeRHS(i, ses.Problem.Constraints[i].B * float(rng.uniform(0.8, 1.2)))
            elif k == 1:
                j = int(rng.integers(0, ses.Problem.NumVars))
                r = ses.ChangeCost(j, ses.Problem.C[j] * float(rng.uniform(0.5, 2.0)))
            elif k == 2:
                r = ses.AddActivity(float(rng.uniform(1.0, 2.0)), rng.random(len(ses.Problem.Constraints)))
            else:
                a = rng.random(ses.Problem.NumVars)
                r = ses.AddConstraint(a, 0, float(a @ r.Solution) * 0.98)
            assert r.Aux[0] == 1.0
            cold = gpu.LPSolver().Solve(ses.Problem, "Primal Simplex")    # all <= with b >= 0 throughout
            assert r.Status == cold.Status == 0
            assert r.OptimalValue == pytest.approx(cold.OptimalValue, rel=1e-9)


# ---- 5. session details ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 8), (30, 50), (200, 300)])
def test_open_is_primal_simplex_bit_for_bit(gpu, shape):
    from linear_programming_solver_lpr381_amd import synth
    m, n = shape
    c, A, b = synth.dense_lp(m, n, seed=m + n)
    prob = gpu.LPProblem.from_arrays(0, c, A, [0] * m, b)
    ref = gpu.LPSolver().Solve(prob, "Primal Simplex")
    with gpu.LPSolver().Open(prob, want_tableau=1) as ses:
        r = ses.Result
        assert np.array_equal(r.Trace, ref.Trace)
        assert np.array_equal(r.Basis, ref.Basis)
        assert _bits(np.array([r.OptimalValue])) == _bits(np.array([ref.OptimalValue]))
        assert _same(r.Tableau, ref.Tableau)
        assert r.Aux[0] == 1.0


def test_capacity_exhaustion_fails_cleanly(gpu):
    with gpu.LPSolver().Open(_example(gpu), extra_rows=1, extra_cols=1, want_tableau=1) as ses:
        T0 = ses.Result.Tableau.copy()
        with pytest.raises(gpu.SolverException) as e:
            ses.AddConstraint([1.0, 1.0], 2, 7.0)                  # an equality takes 2 rows
        assert e.value.code == gpu._lib.EINVAL
        r = ses.ChangeRHS(0, 4.0)                                  # unchanged session: same model, 0 pivots
        assert _same(r.Tableau, T0) and len(r.Trace) == 0
        r = ses.AddActivity(1.0, [1.0, 1.0, 1.0])                  # takes the one spare column
        with pytest.raises(gpu.SolverException) as e:
            ses.AddActivity(1.0, [1.0, 1.0, 1.0])
        assert e.value.code == gpu._lib.EINVAL
        with pytest.raises(gpu.SolverException):
            ses.AddConstraint([1.0, 1.0, 1.0], 0, 7.0)
        assert ses.Problem.NumVars == 3 and len(ses.Problem.Constraints) == 3


def test_ranging_after_edits_matches_the_reference(gpu):
    with gpu.LPSolver().Open(_example(gpu), want_tableau=1) as ses:
        ses.ChangeRHS(2, 20.0)
        ses.AddActivity(1.0, [1.0, 0.0, 1.0])
        r = ses.AddConstraint([1.0, 1.0, 0.0], 0, 7.0)
        T, basis = r.Tableau, r.Basis
        rg = ses.Ranging()
    assert rg.valid
    w = ref_ranging(T, basis)
    d = T[-1, :-1]
    slack = [2, 3, 4, 6]                                            # x1 x2 | c1 c2 c3 | x3 | c4
    var = [0, 1, 5]
    b = [4.0, 12.0, 20.0, 7.0]
    for i, s in enumerate(slack):
        assert rg.dual[i] == d[s]
        assert rg.rhs_hi[i] == b[i] + w["col_inc"][s] and rg.rhs_lo[i] == b[i] - w["col_dec"][s]
    cost = [3.0, 5.0, 1.0]
    row_of = {int(c): k for k, c in enumerate(basis)}
    for j, col in enumerate(var):
        if col in row_of:
            k = row_of[col]
            assert rg.cost_hi[j] == cost[j] + w["row_inc"][k] and rg.cost_lo[j] == cost[j] - w["row_dec"][k]
        else:
            assert rg.cost_hi[j] == cost[j] + max(d[col], 0.0) and rg.reduced_cost[j] == -d[col]


def test_cli_set_rhs_and_cost(gpu):
    out = subprocess.run([CLI, "--set-rhs", "3=20", EXAMPLE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    tail = out.stdout.split("Re-solve after --set-rhs 3=20 (warm, 0 pivots):")[1]
    assert "z = 38" in tail
    out = subprocess.run([CLI, "--set-rhs", "3=30", "--set-cost", "1=10", EXAMPLE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "z = 42" in out.stdout.split("--set-rhs 3=30")[1] and "z = 70" in out.stdout.split("--set-cost 1=10")[1]
    out = subprocess.run([CLI, "--set-rhs", "0=1", EXAMPLE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 64
