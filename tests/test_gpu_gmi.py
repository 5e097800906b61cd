"""GPU checks of the GMI cutting planes: lpx_tableau_gmi_round bit for bit against the numpy restatement (tests/_gmi_ref.py)
on ragged shapes, mixed masks, purges, capacity caps and the zero-candidate case; the whole loop (lpx_solve_cuts) bit for
bit against the reference loop on the CPU oracle; and the model-level outcomes through lpx_solve, LPSolver and the CLI."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gmi_ref as G                          # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _solved_lp(oracle, n, m, seed):
    """An oracle-solved LP tableau with integer data: Max c.x, A x <= b, A >= 0 (C - 1 = n + m)."""
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 20, n).astype(float)
    A = rng.integers(0, 10, (m, n)).astype(float)
    b = rng.integers(10 * n // 4 + 5, 10 * n // 2 + 20, m).astype(float)
    T, basis = G.build_tableau(c, A, b)
    st, _ = oracle.primal_tableau(T, basis)
    assert st == G.OPTIMAL
    return T, basis


def _round_both(lpx, T, basis, is_int, first, o, Rcap, Ccap):
    ref = G.gmi_round(T.copy(), basis.copy(), is_int, len(is_int), first, o, Rcap, Ccap)
    with lpx.DeviceTableau.with_capacity(T, basis, Rcap, Ccap) as dt:
        src, pcol = dt.gmi_round(is_int, first, opts=lpx.CutOpts(**vars(o)).to_c())
        Tg, bg = dt.download()
    Tr, br, sr, pr = ref
    assert Tg.shape == Tr.shape
    assert list(src) == list(sr)
    assert list(pcol) == list(pr)
    assert np.array_equal(bg, br)
    assert np.array_equal(_bits(Tg), _bits(Tr)), "tableau differs from the reference round"
    return Tr, br, sr, pr


@pytest.mark.parametrize("n,m", [(411, 100), (412, 100), (413, 100), (823, 200), (824, 200), (825, 200), (60, 40)])
def test_round_bitwise_ragged_widths(gpu, oracle, n, m):
    T, basis = _solved_lp(oracle, n, m, seed=n * 7 + m)
    R, C = T.shape
    o = G.CutOpts()
    Tr, br, src, _ = _round_both(gpu, T, basis, np.ones(C - 1, np.uint8), C - 1, o, R + 64, C + 64)
    assert len(src) > 0


@pytest.mark.parametrize("seed", range(4))
def test_round_bitwise_mixed_masks(gpu, oracle, seed):
    T, basis = _solved_lp(oracle, 150, 60, seed=100 + seed)
    R, C = T.shape
    rng = np.random.default_rng(seed)
    is_int = (rng.random(150 + 30) < 0.6).astype(np.uint8)      # the last 30 slacks are continuous (j >= n_mask)
    o = G.CutOpts(cuts_per_round=int(rng.integers(1, 65)), coef_eps=[1e-9, 1e-6, 0.0, 1e-3][seed],
                  max_dynamism=[1e6, 10.0, 1.0, 1e3][seed], away=[1e-3, 0.05, 0.2, 0.5][seed])
    _round_both(gpu, T, basis, is_int, C - 1, o, R + 64, C + 64)


def test_round_capacity_caps_k(gpu, oracle):
    T, basis = _solved_lp(oracle, 100, 50, seed=5)
    R, C = T.shape
    _, _, src, _ = _round_both(gpu, T, basis, np.ones(C - 1, np.uint8), C - 1, G.CutOpts(cuts_per_round=8), R + 3, C + 5)
    assert len(src) == 3


def test_round_zero_candidates_leaves_the_tableau(gpu, oracle):
    T, basis = _solved_lp(oracle, 100, 50, seed=6)
    R, C = T.shape
    with gpu.DeviceTableau.with_capacity(T, basis, R + 8, C + 8) as dt:
        src, pcol = dt.gmi_round(np.zeros(0, np.uint8), C - 1)                 # every column continuous: no candidate
        Tg, bg = dt.download()
    assert len(src) == 0 and len(pcol) == 0
    assert np.array_equal(_bits(Tg), _bits(T)) and np.array_equal(bg, basis)


def test_round_purge_after_a_dual_run(gpu, oracle):
    """Round, dual re-optimisation (both sides), second round with purges: the compacting pass bit for bit."""
    done = 0
    for seed in range(30):
        T, basis = _solved_lp(oracle, 40, 25, seed=300 + seed)
        R, C = T.shape
        is_int = np.ones(C - 1, np.uint8)
        o = G.CutOpts(cuts_per_round=16)
        Rcap, Ccap = R + 64, C + 64
        with gpu.DeviceTableau.with_capacity(T, basis, Rcap, Ccap) as dt:
            T1, b1, src, _ = G.gmi_round(T.copy(), basis.copy(), is_int, C - 1, C - 1, o, Rcap, Ccap)
            s1, _ = dt.gmi_round(is_int, C - 1, opts=gpu.CutOpts(**vars(o)).to_c())
            assert list(s1) == list(src)
            if not len(src):
                continue
            T1 = np.ascontiguousarray(T1)
            st, tr, _ = oracle.dual_tableau(T1, b1, fdf_guard=0, cleanup=1)
            stg, _ = dt.dual_run(fdf_guard=0, cleanup=1)
            assert stg == st
            assert dt.trace().tolist() == tr.tolist()
            if st != G.OPTIMAL:
                continue
            T2, b2, src2, pcol2 = G.gmi_round(T1.copy(), b1.copy(), is_int, C - 1, C - 1, G.CutOpts(), Rcap, Ccap)
            s2, p2 = dt.gmi_round(is_int, C - 1)
            Tg, bg = dt.download()
        assert list(s2) == list(src2) and list(p2) == list(pcol2)
        assert np.array_equal(bg, b2) and np.array_equal(_bits(Tg), _bits(T2))
        if pcol2:
            done += 1
            if done >= 3:
                break
    assert done >= 1, "no purge reached"


def test_round_purge_beyond_max_active_fills_exactly_the_documented_buffer(gpu, oracle):
    """Two rounds of 64 cuts (max_active stays at its default of 64), then a round that purges all 128 cut columns: the round
    writes exactly C-1 - first_cut_col purged columns, the size include/lpx.h gives, and nothing past them."""
    T, basis = _solved_lp(oracle, 400, 200, seed=77)
    R, C = T.shape
    first = C - 1
    is_int = np.ones(first, np.uint8)
    Rcap, Ccap = R + 160, C + 160
    o64 = G.CutOpts(cuts_per_round=64)
    Tr, br = T.copy(), basis.copy()
    with gpu.DeviceTableau.with_capacity(T, basis, Rcap, Ccap) as dt:
        for _ in range(2):
            Tr, br, sr, pr = G.gmi_round(Tr, br, is_int, first, first, o64, Rcap, Ccap)
            s, p = dt.gmi_round(is_int, first, opts=gpu.CutOpts(**vars(o64)).to_c())
            assert list(s) == list(sr) and len(sr) == 64 and not pr and not len(p)
        ncut = dt.C - 1 - first
        opg = G.CutOpts(cuts_per_round=8, purge_tol=-2.0)
        Tr, br, sr, pr = G.gmi_round(Tr, br, is_int, first, first, opg, Rcap, Ccap)
        assert len(pr) == ncut == 128 > opg.max_active
        canary = -12345
        buf = np.full(ncut + 16, canary, np.int32)
        src = np.zeros(opg.cuts_per_round, np.int32)
        k, npg = ctypes.c_int(), ctypes.c_int()
        co = gpu.CutOpts(**vars(opg)).to_c()
        rc = gpu._lib.lib().lpx_tableau_gmi_round(dt._h, is_int.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), first, first,
                                                   ctypes.byref(co), ctypes.byref(k), src.ctypes.data_as(gpu._lib.ip),
                                                   ctypes.byref(npg), buf.ctypes.data_as(gpu._lib.ip))
        assert rc == 0
        assert npg.value == ncut and list(buf[:ncut]) == list(pr) and np.all(buf[ncut:] == canary)
        assert k.value == len(sr) and list(src[:k.value]) == list(sr)
        dt.R, dt.C = Tr.shape
        Tg, bg = dt.download()
    assert np.array_equal(bg, br) and np.array_equal(_bits(Tg), _bits(Tr))


def test_round_large_ip_tableau(gpu):
    """One round on a 1025 x 3073 tableau (m = 1024, n = 2048 integer data) after 150 primal pivots on the device."""
    rng = np.random.default_rng(11)
    n, m = 2048, 1024
    c = rng.integers(1, 20, n).astype(float)
    A = rng.integers(0, 10, (m, n)).astype(float)
    b = rng.integers(2000, 6000, m).astype(float)
    T, basis = G.build_tableau(c, A, b)
    R, C = T.shape
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        dt.primal_run(max_iter=150)
        T, basis = dt.download()
    _, _, src, _ = _round_both(gpu, T, basis, np.ones(C - 1, np.uint8), C - 1, G.CutOpts(cuts_per_round=64), R + 64, C + 64)
    assert len(src) > 0


KATS = [
    (G.MAX, [7, 10], [[-1, 3], [7, 1]], [G.LE, G.LE], [6, 35], G.CUT_INTEGER, 58.0),
    (G.MIN, [1, 1], [[2, 2]], [G.GE], [3], G.CUT_INTEGER, 2.0),
    (G.MAX, [1, 1], [[2, 2]], [G.EQ], [3], G.INFEASIBLE, None),
    (G.MAX, [1, 1], [[1, 0], [0, 1]], [G.LE, G.LE], [2, 3], G.CUT_INTEGER, 5.0),
]


def _problems():
    out = [(s, np.array(c, float), np.array(A, float), rel, np.array(b, float), G.CutOpts()) for s, c, A, rel, b, _, _ in KATS]
    for seed in range(20):
        rng = np.random.default_rng(2000 + seed)
        n = int(rng.integers(2, 7))
        s, c, A, rel, b = G.random_ip(rng, n, int(rng.integers(1, 4)), ub=int(rng.integers(2, 5)))
        out.append((s, c, A, rel, b, G.CutOpts(cuts_per_round=int(rng.integers(1, 9)))))
    for seed in range(4):             # larger ones: more rounds, purges, the round cap
        rng = np.random.default_rng(3000 + seed)
        s, c, A, rel, b = G.random_ip(rng, 12, 8, ub=9)
        out.append((s, c, A, rel, b, G.CutOpts(cuts_per_round=4, max_rounds=[50, 6, 20, 50][seed], max_active=[64, 8, 12, 6][seed])))
    return out


PROBLEMS = _problems()


def _rounds_src(res):
    log = np.asarray(res.NodeLog).reshape(-1, 3)
    out = {}
    for rd, src, _ in log:
        out.setdefault(int(rd), []).append(int(src))
    return [out[k] for k in sorted(out)]


@pytest.mark.parametrize("case", range(len(PROBLEMS)))
def test_loop_bitwise_against_reference(gpu, oracle, case):
    s, c, A, rel, b, o = PROBLEMS[case]
    ref = G.gmi_solve(oracle, s, c, A, rel, b, o)
    prob = gpu.LPProblem.from_arrays(s, c, A, rel, b)
    res = gpu.LPSolver().SolveCuts(prob, gpu.CutOpts(**vars(o)))
    assert res.Status == ref.status
    assert _rounds_src(res) == ref.src_rows
    assert res.Trace.tolist() == ref.trace.tolist()
    assert res.Tableau.shape == ref.T.shape
    assert np.array_equal(_bits(res.Tableau), _bits(ref.T))
    assert np.array_equal(res.Basis, ref.basis)
    assert np.array_equal(_bits(res.Solution), _bits(ref.x))
    assert res.OptimalValue == ref.z
    assert res.LpSolves == 1 + ref.rounds
    assert list(res.Aux) == [ref.rounds, ref.added, ref.purged, ref.root_z]
    n = len(c)
    if ref.added:
        assert res.Cuts.shape == (ref.added, n + 1)
        assert np.allclose(res.Cuts, ref.cuts, rtol=1e-9, atol=1e-9)
    assert res.VarNames[:n] == [f"x{j + 1}" for j in range(n)]


def _ub(A, rel, b, n):
    ub = np.full(n, np.inf)
    for a, r, bi in zip(A, rel, b):
        if r == G.LE and np.all(a >= 0):
            for j in range(n):
                if a[j] > 0:
                    ub[j] = min(ub[j], np.floor(bi / a[j]))
    return ub


@pytest.mark.parametrize("case", range(len(KATS)))
def test_model_level_kats(gpu, case):
    s, c, A, rel, b, status, z = KATS[case]
    prob = gpu.LPProblem.from_arrays(s, c, A, rel, b)
    for res in (gpu.LPSolver().Solve(prob, "GMI Cutting Plane"), gpu.LPSolver().Solve(prob, "gmi"),
                gpu.GmiCuttingPlane().Solve(prob), gpu.LPSolver().SolveCuts(prob)):
        assert res.Status == status
        if z is not None:
            assert res.OptimalValue == pytest.approx(z, abs=1e-9)
    if case == 0:
        assert np.allclose(res.Solution, [4, 3])
        assert res.VarNames[:4] == ["x1", "x2", "c1", "c2"]
        assert res.VarNames[4:] == [f"g{k + 1}" for k in range(len(res.VarNames) - 4)]


@pytest.mark.parametrize("case", range(4, 24))      # small enough to enumerate
def test_model_level_cuts_valid_and_bounds(gpu, case):
    s, c, A, rel, b, o = PROBLEMS[case]
    n = len(c)
    res = gpu.LPSolver().SolveCuts(gpu.LPProblem.from_arrays(s, c, A, rel, b), gpu.CutOpts(**vars(o)))
    pts = G.enumerate_points(A, rel, b, _ub(A, rel, b, n))
    best = max(c @ p for p in pts)
    if res.Cuts is not None:
        assert (pts @ res.Cuts[:, :n].T - res.Cuts[:, n]).max() <= 1e-6
    root = res.Aux[3]
    if res.Status == G.CUT_INTEGER:
        from scipy.optimize import Bounds, LinearConstraint, milp
        lo = np.where(np.array(rel) == G.GE, b, -np.inf)
        hi = np.where(np.array(rel) == G.GE, np.inf, b)
        sol = milp(-c, constraints=LinearConstraint(A, lo, hi), integrality=np.ones(n), bounds=Bounds(0, np.inf))
        assert res.OptimalValue == pytest.approx(-sol.fun, abs=1e-6)
    else:
        assert res.Status == G.CUT_INCOMPLETE
        assert best - 1e-6 <= res.OptimalValue <= root + 1e-9


def test_cli_gmi(gpu):
    path = os.path.join(ROOT, "integration", "Input", "example_gmi.txt")
    for extra in ([], ["--cuts-per-round", "2", "--cut-rounds", "30"]):
        out = subprocess.run([CLI, "--algorithm", "GMI Cutting Plane", *extra, path], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert "Status: OPTIMAL INTEGER" in out.stdout and "z = 58" in out.stdout
    out = subprocess.run([CLI, "--algorithm", "gmi", "--cut-rounds", "0", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "INCOMPLETE" in out.stdout and "z = 66.5" in out.stdout
