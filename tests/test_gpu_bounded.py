"""GPU tests of the bounded-variable primal simplex (lpx_bounded_run, csrc/lpx_bounded.hip): bit for bit against the NumPy
restatement of the contract (tests/_bounded_ref.py) -- trace with its encoding, final tableau, basis, flip states, counts,
status -- on the hand example, the model list of test_bounded_reference.py, the config-4 root LP, every shape edge of the
select kernel and its global-scratch path; the decision edges on small exact tableaux; equality with lpx_primal_run when no
column is bounded; independence of batching, graph replay and callbacks; snapshot / restore; the model level and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import _bounded_ref as B
from linear_programming_solver_lpr381_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
EXAMPLE = os.path.join(ROOT, "integration", "Input", "example_bounded.txt")
INF = np.inf
REL = 1e-9


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _gpu_run(lpx, T, basis, ub, cap=None, set_bounds=True, cb=None, **opts):
    dt = lpx.DeviceTableau.from_host(T, basis) if cap is None else lpx.DeviceTableau.with_capacity(T, basis, *cap)
    with dt:
        if set_bounds and ub is not None:
            dt.set_bounds(ub)
        status, st = dt.bounded_run(cb=cb, **opts)
        Tg, bg = dt.download()
        return status, Tg, bg, dt.bound_flags(), dt.trace(), dt.bounded_counts(), st


def _same(got, ref):
    status, Tg, bg, flip, tr, counts, st = got
    rstatus, Tr, br, rflip, rtr, rcounts = ref
    assert status == rstatus
    assert tr.tolist() == rtr.tolist()
    assert counts == rcounts
    assert bg.tolist() == br.tolist()
    assert flip.tolist() == rflip.tolist()
    assert np.array_equal(_u64(Tg), _u64(Tr)), "tableau bits differ from the restatement"
    assert st["pivots"] == rcounts[0] + rcounts[1]


def _check(lpx, T, basis, ub, cap=None, **opts):
    ref_opts = {k: v for k, v in opts.items() if k in ("eps", "max_iter")}
    if "ratio_tol" in opts:
        ref_opts["tol"] = opts["ratio_tol"]
    ref = B.run(T, basis, ub, **ref_opts)
    got = _gpu_run(lpx, T, basis, ub, cap=cap, **opts)
    _same(got, ref)
    return got, ref


# ---- item 4: bit-exact against the restatement -------------------------------------------------------------------------
def test_hand_example(gpu):
    T, basis, ub, _ = B.hand_example()
    got, ref = _check(gpu, T, basis, ub)
    assert got[0] == B.OPTIMAL and got[4].tolist() == [[-1, 1], [1, 0], [-3, 1]] and got[5] == (1, 1, 1)
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        dt.bounded_run()
        x, z, up = dt.bounded_solution(3)
    assert x.tolist() == [4.0, 1.75, 0.0] and z == 20.75 and up.tolist() == [1, 0, 0]


@pytest.mark.parametrize("seed", B.BINARY_SEEDS)
@pytest.mark.parametrize("n,m", B.BINARY_SHAPES)
def test_binary_models(gpu, n, m, seed):
    T, basis, ub, _ = B.binary_bounded(n, m, seed)
    got, ref = _check(gpu, T, basis, ub)
    assert got[0] == B.OPTIMAL and min(got[5]) > 0


@pytest.mark.parametrize("m,n", B.DENSE_UNIT_SHAPES)
def test_dense_unit_bounds(gpu, m, n):
    T, basis, ub, _ = B.dense_unit_bounded(m, n)
    got, ref = _check(gpu, T, basis, ub)
    assert got[0] == B.OPTIMAL and min(got[5]) > 0


def test_config4_root_lp_at_full_size(gpu):
    T, basis, ub, _ = B.binary_bounded(512, 256)
    assert T.shape == (257, 769)
    got, ref = _check(gpu, T, basis, ub)
    assert got[0] == B.OPTIMAL and min(got[5]) > 0


# m at the wave edges; m and Cm at the select kernel's lane count; C around a multiple of 16 (the padded leading dimension)
EDGE_SHAPES = [(16, 1), (16, 2), (24, 63), (24, 64), (24, 65),
               (40, 1023), (40, 1024), (40, 1025), (959, 64), (960, 64), (961, 64),
               (38, 8), (39, 8), (40, 8)]


@pytest.mark.parametrize("n,m", EDGE_SHAPES)
def test_shape_edges(gpu, n, m):
    T, basis, ub, _ = B.binary_bounded(n, m, 5)
    _check(gpu, T, basis, ub)


def test_spare_capacity(gpu):
    T, basis, ub, _ = B.binary_bounded(40, 20, 2)
    got, ref = _check(gpu, T, basis, ub, cap=(40, 100))
    assert got[0] == B.OPTIMAL and min(got[5]) > 0


def test_global_scratch_ratios(gpu):
    """More than 4096 rows: the ratios do not fit the kernel's LDS array and go through global scratch (lpx.h)."""
    T, basis, ub, _ = B.binary_bounded(12, 4100, 3)
    got, ref = _check(gpu, T, basis, ub, max_iter=6)
    assert len(got[4]) == 6 and got[0] == B.ITER_LIMIT


# ---- item 5: decision edges, small integer tableaux, every quantity exact ---------------------------------------------------
def _tab(rows, obj, basis):
    return np.array(rows + [obj], dtype=np.float64), np.array(basis, dtype=np.int32)


def test_bound_equal_to_best_ratio_flips(gpu):
    T, basis = _tab([[2, 1, 4]], [-1, 0, 0], [1])
    got, ref = _check(gpu, T, basis, np.array([2.0, INF]))
    assert got[4].tolist() == [[-1, 0]] and got[0] == B.OPTIMAL
    assert got[1].tolist() == [[-2.0, 1.0, 0.0], [1.0, 0.0, 2.0]]


@pytest.mark.parametrize("tol,second", [(1e-9, 2.0), (0.5, 1.75)])
def test_hysteresis_keeps_the_earlier_row_across_kinds(gpu, tol, second):
    # columns: x (entering, unbounded), s1 (basic row 0), s2 (basic row 1), RHS; the kind-1 row's basic variable has u = 5
    # kind 0 first (rho = 2), kind 1 second (rho = (5 - (5 - second)) / 1 = second, within tol of 2)
    T, basis = _tab([[1, 1, 0, 2], [-1, 0, 1, 5 - second]], [-1, 0, 0, 0], [1, 2])
    got, ref = _check(gpu, T, basis, np.array([INF, INF, 5.0]), ratio_tol=tol, max_iter=1)
    assert got[4].tolist() == [[0, 0]]
    # kind 1 first (rho = (5 - 3) / 1 = 2), kind 0 second (rho = second)
    T, basis = _tab([[-1, 1, 0, 3], [1, 0, 1, second]], [-1, 0, 0, 0], [1, 2])
    got, ref = _check(gpu, T, basis, np.array([INF, 5.0, INF]), ratio_tol=tol, max_iter=1)
    assert got[4].tolist() == [[-2, 0]]


def test_fixed_variable_flips_once_and_never_enters_again(gpu):
    T, basis = _tab([[1, 1, 1, 0, 4], [2, 1, 0, 1, 6]], [-5, -1, 0, 0, 0], [2, 3])
    got, ref = _check(gpu, T, basis, np.array([0.0, INF, INF, INF]))
    tr = got[4].tolist()
    assert tr[0] == [-1, 0] and [q for _, q in tr].count(0) == 1 and got[0] == B.OPTIMAL
    assert got[3].tolist() == [1, 0, 0, 0]


def test_negative_entry_of_an_unbounded_basic_variable_is_ignored(gpu):
    T, basis = _tab([[-1, 1, 0, 1], [1, 0, 1, 4]], [-1, 0, 0, 0], [1, 2])
    got, ref = _check(gpu, T, basis, np.array([INF, INF, INF]), max_iter=1)
    assert got[4].tolist() == [[1, 0]]
    got, ref = _check(gpu, T, basis, np.array([INF, 9.0, INF]), max_iter=1)      # the same row with a bound takes part: (9 - 1) / 1 = 8 > 4
    assert got[4].tolist() == [[1, 0]]
    got, ref = _check(gpu, T, basis, np.array([INF, 3.0, INF]), max_iter=1)      # (3 - 1) / 1 = 2 < 4
    assert got[4].tolist() == [[-2, 0]]


def test_unbounded_column(gpu):
    T, basis = _tab([[-1, 1, 0, 1], [0, 0, 1, 4]], [-1, 0, 0, 0], [1, 2])
    got, ref = _check(gpu, T, basis, np.array([INF, INF, INF]))
    assert got[0] == B.UNBOUNDED and len(got[4]) == 0
    got, ref = _check(gpu, T, basis, np.array([7.0, INF, INF]))                  # a finite bound on the column: it flips instead
    assert got[0] == B.OPTIMAL and got[4].tolist() == [[-1, 0]]


@pytest.mark.parametrize("max_iter,last", [(1, [-1, 1]), (2, [1, 0])])
def test_iteration_limit_on_a_flip_and_on_a_pivot(gpu, max_iter, last):
    T, basis, ub, _ = B.hand_example()
    got, ref = _check(gpu, T, basis, ub, max_iter=max_iter)
    assert got[0] == B.ITER_LIMIT and len(got[4]) == max_iter and got[4][-1].tolist() == last


# ---- item 6: no bounded column = lpx_primal_run -----------------------------------------------------------------------------
def _primal(lpx, T, basis, **opts):
    with lpx.DeviceTableau.from_host(T, basis) as dt:
        status, st = dt.primal_run(**opts)
        Tg, bg = dt.download()
        return status, Tg, bg, dt.trace()


@pytest.mark.parametrize("m,n,max_iter", [(24, 40, 10000), (48, 80, 10000), (1024, 2048, 200)])
def test_without_bounds_it_is_the_primal_loop(gpu, m, n, max_iter):
    c, A, b = synth.dense_lp(m, n) if m == 1024 else synth.dense_lp(m, n, 7)
    T, basis = synth.primal_tableau_from(c, A, b)
    ps, pT, pb, ptr = _primal(gpu, T, basis, max_iter=max_iter)
    assert len(ptr) == (200 if m == 1024 else len(ptr)) and len(ptr) > 0
    for set_bounds in (True, False):          # every ub = +inf, and a handle that never had bounds
        got = _gpu_run(gpu, T, basis, np.full(T.shape[1] - 1, INF), set_bounds=set_bounds, max_iter=max_iter)
        assert got[0] == ps and got[4].tolist() == ptr.tolist() and got[2].tolist() == pb.tolist()
        assert np.array_equal(_u64(got[1]), _u64(pT))
        assert not got[3].any() and got[5] == (len(ptr), 0, 0)


# ---- item 7: the bits do not depend on how the launches are issued ----------------------------------------------------------
@pytest.mark.parametrize("which", ["hand", "binary", "dense"])
def test_batching_graph_and_callback_do_not_change_the_result(gpu, which):
    T, basis, ub, _ = {"hand": B.hand_example, "binary": lambda: B.binary_bounded(64, 32, 1),
                       "dense": lambda: B.dense_unit_bounded(64, 128)}[which]()
    ref = B.run(T, basis, ub)
    for opts in ({"use_graph": 0}, {"batch": 1}, {"batch": 7}, {"batch": 7, "use_graph": 0}, {"profile": 1}, {}):
        _same(_gpu_run(gpu, T, basis, ub, **opts), ref)
    seen = []
    got = _gpu_run(gpu, T, basis, ub, cb=lambda it, r, q: seen.append((it, r, q)))
    _same(got, ref)
    assert seen == [(k + 1, int(r), int(q)) for k, (r, q) in enumerate(ref[4])]
    seen.clear()
    _same(_gpu_run(gpu, T, basis, ub, cb=lambda it, r, q: seen.append((it, r, q)), batch=3), ref)
    assert [(r, q) for _, r, q in seen] == [tuple(e) for e in ref[4].tolist()]


# ---- item 8: snapshot / restore, set_bounds, set_shape ----------------------------------------------------------------------
def test_snapshot_restore_and_bound_lifetime(gpu):
    T, basis, ub, _ = B.binary_bounded(40, 20, 2)
    ref = B.run(T, basis, ub)
    with gpu.DeviceTableau.with_capacity(T, basis, T.shape[0] + 2, T.shape[1] + 3) as dt:
        dt.set_bounds(ub)
        dt.snapshot()
        runs = []
        for k in range(2):
            status, st = dt.bounded_run()
            Tg, bg = dt.download()
            runs.append((status, Tg, bg, dt.bound_flags(), dt.trace(), dt.bounded_counts(), st))
            assert runs[-1][3].any()
            dt.restore()
            assert not dt.bound_flags().any()             # the snapshot's own flip states came back
            T0, b0 = dt.download()
            assert np.array_equal(_u64(T0), _u64(T)) and b0.tolist() == basis.tolist()
        _same(runs[0], ref)
        _same(runs[1], ref)
        dt.bounded_run()
        assert dt.bound_flags().any()
        dt.set_bounds(ub)                                 # new bounds: every flip cleared
        assert not dt.bound_flags().any()
        dt.set_shape(T.shape[0], T.shape[1] + 1)          # another live C: the bounds no longer belong to the tableau
        with pytest.raises(gpu.LpxError) as e:
            dt.bounded_run()
        assert e.value.code == gpu._lib.EINVAL
        with pytest.raises(gpu.LpxError) as e:
            dt.set_bounds(ub)                             # ncols is not the live C - 1
        assert e.value.code == gpu._lib.EINVAL
        dt.set_shape(*T.shape)
        with pytest.raises(gpu.LpxError) as e:
            dt.set_bounds(np.array([-1.0] + [1.0] * (T.shape[1] - 2)))
        assert e.value.code == gpu._lib.EINVAL
        with pytest.raises(gpu.LpxError) as e:
            dt.bounded_run(resident=1)
        assert e.value.code == gpu._lib.EINVAL
        dt.upload(T, basis)
        dt.set_bounds(ub)
        status, st = dt.bounded_run()
        Tg, bg = dt.download()
        _same((status, Tg, bg, dt.bound_flags(), dt.trace(), dt.bounded_counts(), st), ref)
        dt.set_bounds(None)                               # bounds removed: the plain primal loop on the same upload
        dt.upload(T, basis)
        assert not dt.bound_flags().any()
        dt.bounded_run()
        To, bo = T.copy(), basis.copy()
        from oracle import oracle as O
        st_o, tr_o = O.primal_tableau(To, bo)
        assert dt.trace().tolist() == tr_o.tolist() and np.array_equal(_u64(dt.download()[0]), _u64(To))


# ---- item 9: the model level ------------------------------------------------------------------------------------------------
def _problem(lpx, c, A, b, sense=0, rel=None):
    return lpx.LPProblem.from_arrays(sense, c, A, np.zeros(len(b), dtype=np.int32) if rel is None else rel, b)


@pytest.mark.parametrize("n,m,seed", [(12, 6, 1), (40, 20, 2), (64, 32, 3), (128, 64, 1), (256, 128, 2)])
def test_solve_bounded_matches_the_rows_model(gpu, n, m, seed):
    c, A, rel, b = synth.binary_ip(n, m, seed)
    rows = gpu.LPSolver().Solve(_problem(gpu, c, A, b), "Primal Simplex")
    res = gpu.LPSolver().SolveBounded(_problem(gpu, c, A[:m], b[:m]), upper=1.0)
    assert res.Status == gpu._lib.OPTIMAL and rows.Status == gpu._lib.OPTIMAL
    assert abs(res.OptimalValue - rows.OptimalValue) <= REL * max(1.0, abs(rows.OptimalValue))
    x = res.Solution
    assert (x >= -1e-6).all() and (x <= 1 + 1e-6).all() and (A[:m] @ x <= b[:m] + 1e-6).all()
    assert res.Tableau.shape == (m + 1, n + m + 1) and rows.Tableau.shape == (m + n + 1, 2 * n + m + 1)
    T, basis, ub, _ = B.binary_bounded(n, m, seed)
    ref = B.run(T, basis, ub)
    assert res.Trace.tolist() == ref[4].tolist() and res.BoundCounts == ref[5]
    assert np.array_equal(_u64(res.Tableau), _u64(ref[1])) and res.Flips.tolist() == ref[3].tolist()
    assert res.AtUpper.tolist() == B.solution(ref[1], ref[2], ref[3], ub, n)[2].tolist()
    assert "at upper bound:" in res.Report and "at upper bound:" in res.Summary


@pytest.mark.parametrize("m,n", B.DENSE_UNIT_SHAPES)
def test_solve_bounded_dense_unit(gpu, m, n):
    c, A, b = synth.dense_lp(m, n)
    rows = gpu.LPSolver().Solve(_problem(gpu, c, np.vstack([A, np.eye(n)]), np.concatenate([b, np.ones(n)])), "Primal Simplex")
    res = gpu.LPSolver().SolveBounded(_problem(gpu, c, A, b), upper=np.ones(n))
    assert abs(res.OptimalValue - rows.OptimalValue) <= REL * max(1.0, abs(rows.OptimalValue))
    assert (res.Solution >= -1e-6).all() and (res.Solution <= 1 + 1e-6).all()


def test_lower_bounds_against_the_model_shifted_by_hand(gpu):
    c = np.array([3.0, 5.0, 2.0]); A = np.array([[1.0, 2.0, 2.0], [2.0, 4.0, 3.0]]); b = np.array([10.0, 15.0])
    l = np.array([1.0, 0.5, 0.0]); u = np.array([4.0, 3.0, 3.0])
    res = gpu.LPSolver().SolveBounded(_problem(gpu, c, A, b), upper=u, lower=l)
    bs = b.copy()
    for j in range(3):
        if l[j] != 0.0:
            bs = bs - A[:, j] * l[j]
    hand = gpu.LPSolver().SolveBounded(_problem(gpu, c, A, bs), upper=u - l)
    assert res.Trace.tolist() == hand.Trace.tolist() and np.array_equal(_u64(res.Tableau), _u64(hand.Tableau))
    assert res.Solution.tolist() == (hand.Solution + l).tolist()
    const = 0.0
    for j in range(3):
        if l[j] != 0.0:
            const = const + c[j] * l[j]
    assert res.OptimalValue == hand.OptimalValue + const and res.Aux[3] == const
    assert (res.Solution >= l - 1e-9).all() and (res.Solution <= u + 1e-9).all() and (A @ res.Solution <= b + 1e-9).all()
    from scipy.optimize import linprog
    hs = linprog(-c, A_ub=A, b_ub=b, bounds=list(zip(l, u)), method="highs")
    assert abs(-hs.fun - res.OptimalValue) <= REL * max(1.0, abs(hs.fun))


def test_min_model_and_equality_row(gpu):
    # Min -3x1 - 5x2 - 2x3 is the hand example: the user's optimum is -20.75
    c = np.array([3.0, 5.0, 2.0]); A = np.array([[1.0, 2.0, 2.0], [2.0, 4.0, 3.0]]); b = np.array([10.0, 15.0])
    res = gpu.LPSolver().SolveBounded(_problem(gpu, -c, A, b, sense=1), upper=[4, 3, 3])
    assert res.OptimalValue == -20.75 and res.Solution.tolist() == [4.0, 1.75, 0.0] and res.AtUpper.tolist() == [1, 0, 0]
    assert res.Trace.tolist() == [[-1, 1], [1, 0], [-3, 1]]
    # an = row becomes the <= pair of the Primal Simplex preparation: x1 - x2 = 0 added to the hand example
    A2 = np.vstack([A, [[1.0, -1.0, 0.0]]]); b2 = np.concatenate([b, [0.0]])
    rel = np.array([0, 0, 2], dtype=np.int32)
    res = gpu.LPSolver().SolveBounded(_problem(gpu, c, A2, b2, rel=rel), upper=[4, 3, 3])
    assert res.Tableau.shape == (5, 8) and res.Status == gpu._lib.OPTIMAL
    from scipy.optimize import linprog
    hs = linprog(-c, A_ub=A, b_ub=b, A_eq=[[1.0, -1.0, 0.0]], b_eq=[0.0], bounds=[(0, 4), (0, 3), (0, 3)], method="highs")
    assert abs(-hs.fun - res.OptimalValue) <= REL * max(1.0, abs(hs.fun))
    assert abs(res.Solution[0] - res.Solution[1]) <= 1e-9


@pytest.mark.parametrize("m,n,seed", [(24, 40, 7), (48, 80, 3)])
def test_no_bounds_is_primal_simplex_bitwise(gpu, m, n, seed):
    c, A, b = synth.dense_lp(m, n, seed)
    p = _problem(gpu, c, A, b)
    ps = gpu.LPSolver().Solve(p, "Primal Simplex")
    for res in (gpu.LPSolver().SolveBounded(p), gpu.LPSolver().Solve(p, "Bounded Primal Simplex")):
        assert res.Status == ps.Status and res.Trace.tolist() == ps.Trace.tolist() and res.Basis.tolist() == ps.Basis.tolist()
        assert np.array_equal(_u64(res.Tableau), _u64(ps.Tableau)) and np.array_equal(_u64(res.Solution), _u64(ps.Solution))
        assert np.array_equal(_u64(np.array([res.OptimalValue])), _u64(np.array([ps.OptimalValue])))


def test_cli_bounds(gpu):
    r = subprocess.run([CLI, "--upper", "1=4", "--upper", "2=3", "--upper", "3=3", EXAMPLE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Status: OPTIMAL" in r.stdout and "z* = 20.75" in r.stdout and "x* = [4, 1.75, 0]" in r.stdout
    assert "at upper bound: x1" in r.stdout
    r = subprocess.run([CLI, "--binary", EXAMPLE], capture_output=True, text=True)          # every u = 1: x = (1, 1, 1), z = 10
    assert r.returncode == 0, r.stderr
    assert "z* = 10" in r.stdout and "x* = [1, 1, 1]" in r.stdout and "at upper bound: x1, x2, x3" in r.stdout
    r = subprocess.run([CLI, "--lower", "3=1", "--upper", "1=4", "--upper", "2=3", "--upper", "3=3", EXAMPLE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    from scipy.optimize import linprog
    hs = linprog([-3.0, -5.0, -2.0], A_ub=[[1, 2, 2], [2, 4, 3]], b_ub=[10, 15], bounds=[(0, 4), (0, 3), (1, 3)], method="highs")
    assert abs(-hs.fun - 19.0) <= 1e-9 and "z* = 19\n" in r.stdout
