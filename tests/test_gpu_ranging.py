"""GPU tests of the ranging pass (csrc/lpx_ranging.hip) and of lpx_solve_ranging / LPSolver.SolveRanged.

The kernels are checked bit for bit against the numpy restatement of the definitions below (include/lpx.h); the
user-level report against a hand-derived KAT, SciPy/HiGHS marginals and the original model data rebuilt in numpy."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "integration", "Input", "example_input.txt")
CLI = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")


# ---- numpy restatement -------------------------------------------------------------------------------------------
def _masked_min(q, mask, axis):
    """Strict minimum of q over mask along axis, lowest index on ties; empty -> (+inf, -1)."""
    qm = np.where(mask, q, np.inf)
    idx = np.argmin(qm, axis=axis)
    val = np.take_along_axis(qm, np.expand_dims(idx, axis), axis).squeeze(axis)
    first = np.argmax(mask, axis=axis)              # an all-+inf candidate set still names its first member
    idx = np.where(val == np.inf, first, idx)
    idx = np.where(mask.any(axis=axis), idx, -1).astype(np.int32)
    return val, idx


def _col_test(G, bp, eps):
    neg, pos = G < -eps, G > eps
    with np.errstate(divide="ignore", invalid="ignore"):
        inc, inc_at = _masked_min(bp[:, None] / -G, neg, 0)
        dec, dec_at = _masked_min(bp[:, None] / G, pos, 0)
    return inc, inc_at, dec, dec_at


def ref_ranging(T, basis, eps=1e-9):
    R, C = T.shape
    m, Cm = R - 1, C - 1
    A, b, d = T[:m, :Cm], T[:m, Cm], T[m, :Cm]
    bp = np.where(b > 0, b, 0.0)
    dp = np.where(d > 0, d, 0.0)
    nb = np.ones(Cm, dtype=bool)
    bs = np.asarray(basis[:m])
    nb[bs[(bs >= 0) & (bs < Cm)]] = False
    ci, cia, cd, cda = _col_test(A, bp, eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        ri, ria = _masked_min(dp[None, :] / -A, (A < -eps) & nb[None, :], 1)
        rd, rda = _masked_min(dp[None, :] / A, (A > eps) & nb[None, :], 1)
    min_rhs = b[np.argmin(b)] if m > 0 else np.inf
    min_dj = d[nb][np.argmin(d[nb])] if nb.any() else np.inf
    return dict(col_inc=ci, col_inc_at=cia, col_dec=cd, col_dec_at=cda, row_inc=ri, row_inc_at=ria, row_dec=rd,
                row_dec_at=rda, min_rhs=min_rhs, min_dj=min_dj)


def ref_pairs(T, a, b, eps=1e-9):
    m = T.shape[0] - 1
    bv = T[:m, -1]
    G = T[:m, a] - T[:m, b]
    return _col_test(G, np.where(bv > 0, bv, 0.0), eps)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def assert_ranging_equal(got, want):
    for k, v in want.items():
        g = getattr(got, k)
        if k.endswith("_at"):
            assert np.array_equal(np.asarray(g), v), k
        else:
            assert np.array_equal(_bits(g), _bits(v)), (k, g, v)


def _random_tableau(g, R, C, quantized):
    if quantized:       # exact ties and exact zeros everywhere
        T = g.integers(-4, 5, size=(R, C)) / 4.0
    else:
        T = g.uniform(-1, 1, size=(R, C))
        T[g.random((R, C)) < 0.1] = 0.0
    m, Cm = R - 1, C - 1
    basis = g.choice(Cm, size=m, replace=m > Cm).astype(np.int32)
    return T, basis


# ---- 1. bitwise against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", [(2, 3), (5, 7), (33, 65), (257, 1031), (1025, 3073), (4097, 257)])
@pytest.mark.parametrize("quantized", [False, True])
def test_random_tableaux_bitwise(gpu, R, C, quantized):
    g = np.random.default_rng(R * 7919 + C + quantized)
    T, basis = _random_tableau(g, R, C, quantized)
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        got = dt.ranging()
        K = 16
        a, b = g.integers(0, C - 1, K), g.integers(0, C - 1, K)
        a[0] = b[0]                 # g = 0 everywhere: empty on both sides
        inc, inc_at, dec, dec_at = dt.ranging_pairs(a, b)
    assert_ranging_equal(got, ref_ranging(T, basis))
    w = ref_pairs(T, a, b)
    assert np.array_equal(_bits(inc), _bits(w[0])) and np.array_equal(inc_at, w[1])
    assert np.array_equal(_bits(dec), _bits(w[2])) and np.array_equal(dec_at, w[3])
    assert inc_at[0] == -1 and dec_at[0] == -1 and np.isinf(inc[0])


def test_shrunk_handle_masks_the_padding(gpu):
    g = np.random.default_rng(11)
    big = g.uniform(-1, 1, size=(70, 150))
    with gpu.DeviceTableau.from_host(big, np.arange(70, 139, dtype=np.int32)) as dt:
        assert dt.ld > 90
        gpu._lib.check(gpu._lib.lib().lpx_tableau_set_shape(dt._h, 40, 90))
        dt.R, dt.C = 40, 90
        T, basis = _random_tableau(g, 40, 90, False)
        dt.upload(T, basis)                        # the columns beyond 90 still hold the old tableau
        got = dt.ranging()
        a, b = np.array([0, 5, 88], np.int32), np.array([3, 88, 0], np.int32)
        pr = dt.ranging_pairs(a, b)
    assert_ranging_equal(got, ref_ranging(T, basis))
    w = ref_pairs(T, a, b)
    for x, y in zip(pr, w):
        assert np.array_equal(np.asarray(x).view(np.uint64) if x.dtype == np.float64 else x,
                              np.asarray(y).view(np.uint64) if y.dtype == np.float64 else y)


@pytest.mark.parametrize("pivots", [7, 40, 10000])
def test_after_primal_pivots(gpu, pivots):
    from linear_programming_solver_lpr381_amd import synth
    c, A, b = synth.dense_lp(96, 160, seed=5)
    T0, basis0 = synth.primal_tableau_from(c, A, b)
    with gpu.DeviceTableau.from_host(T0, basis0) as dt:
        dt.primal_run(max_iter=pivots)
        T, basis = dt.download()
        for eps in (1e-9, 0.0, 1e-3):
            assert_ranging_equal(dt.ranging(eps), ref_ranging(T, basis, eps))


def test_planted_cases(gpu):
    eps = 1e-9
    T = np.zeros((6, 9))
    T[:5, :8] = [[1, -2, eps, -eps, 0.5, 2, 1, 0],
                 [2, -4, 2 * eps, -2 * eps, 0.25, 1, 0, 1],
                 [4, -1, -eps, eps, -0.5, -2, 0, 0],
                 [0.5, 2, 1, 1, 1, 1, 1, 1],
                 [-1, 1, -1, 1, -1, 1, -1, 1]]
    T[:5, 8] = [2.0, 4.0, -0.0, 1.0, -3e-10]        # b_r = -0.0 and a tiny negative b
    T[5, :8] = [-0.0, 3.0, -1e-12, 0.0, 6.0, -0.0, 0.0, 2.0]     # small negative d_j, signed zeros
    T[5, 8] = 7.0
    basis = np.array([6, 7, 0, 5, 5], dtype=np.int32)      # a repeated entry is still one basic column
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        for e in (eps, 0.0):
            got = dt.ranging(e)
            want = ref_ranging(T, basis, e)
            assert_ranging_equal(got, want)
        pr = dt.ranging_pairs(np.array([0, 2, 1], np.int32), np.array([1, 3, 1], np.int32), 0.0)
    assert want["col_dec"][0] == 0.0 and want["col_dec_at"][0] == 2          # b_2 = -0.0 -> +0.0: 0 / 4 beats the 2.0 ties
    assert want["min_rhs"] == -3e-10 and want["min_dj"] == -1e-12
    w = ref_pairs(T, np.array([0, 2, 1]), np.array([1, 3, 1]), 0.0)
    assert np.array_equal(_bits(pr[0]), _bits(w[0])) and np.array_equal(pr[1], w[1])
    assert np.array_equal(_bits(pr[2]), _bits(w[2])) and np.array_equal(pr[3], w[3])


def test_scalars_flag_infeasible_tableaux(gpu):
    T = np.array([[1.0, 0.0, 1.0, 0.0, -2.0],
                  [0.0, 1.0, 0.0, 1.0, 3.0],
                  [0.0, -0.5, 0.0, 0.0, 9.0]])
    basis = np.array([0, 1], dtype=np.int32)
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        r = dt.ranging()
    assert r.min_rhs == -2.0 and r.min_dj == 0.0          # columns 2, 3 are nonbasic: d = 0, 0
    T[2, 2] = -0.25
    with gpu.DeviceTableau.from_host(T, np.array([0, 1], dtype=np.int32)) as dt:
        assert dt.ranging().min_dj == -0.25


def test_ranging_leaves_the_handle_alone(gpu):
    from linear_programming_solver_lpr381_amd import synth
    c, A, b = synth.dense_lp(64, 100, seed=9)
    T0, basis0 = synth.primal_tableau_from(c, A, b)
    with gpu.DeviceTableau.from_host(T0, basis0) as dt:
        dt.snapshot()
        dt.primal_run(max_iter=25)
        T1, b1 = dt.download()
        tr1 = dt.trace()
        dt.ranging(); dt.ranging_pairs([0, 1], [2, 3])
        T2, b2 = dt.download()
        assert np.array_equal(_bits(T1), _bits(T2)) and np.array_equal(b1, b2)
        assert np.array_equal(tr1, dt.trace())
        dt.restore()
        T3, b3 = dt.download()
        assert np.array_equal(_bits(T3), _bits(T0)) and np.array_equal(b3, basis0)


# ---- 2. headline shape --------------------------------------------------------------------------------------------
def test_headline_shape_after_200_pivots(gpu):
    from linear_programming_solver_lpr381_amd import synth
    c, A, b = synth.dense_lp(4096, 8192)
    T0, basis0 = synth.primal_tableau_from(c, A, b)
    del A
    with gpu.DeviceTableau.from_host(T0, basis0) as dt:
        del T0
        status, st = dt.primal_run(max_iter=200)
        assert st["pivots"] == 200
        T, basis = dt.download()
        got = dt.ranging()
        a = np.arange(4096, 4096 + 64, dtype=np.int32) + 8192 - 4096
        pr = dt.ranging_pairs(a, a + 1)
    assert T.shape == (4097, 12289)
    assert_ranging_equal(got, ref_ranging(T, basis))
    w = ref_pairs(T, a, a + 1)
    assert np.array_equal(_bits(pr[0]), _bits(w[0])) and np.array_equal(pr[1], w[1])
    assert np.array_equal(_bits(pr[2]), _bits(w[2])) and np.array_equal(pr[3], w[3])


# ---- 3. hand KAT -------------------------------------------------------------------------------------------------
# Max 3x1 + 5x2, x1 <= 4, 2x2 <= 12, 3x1 + 2x2 <= 18 (integration/Input/example_input.txt): x* = (2, 6), z* = 36.
# The primal loop pivots (row 1, x2) then (row 2, x1), so basis = [c1, x2, x1] = columns [2, 1, 0] and the final rows are
#   row 0 (c1): c2 coefficient  1/3, c3 -1/3, rhs 2;  row 1 (x2): c2 1/2, c3 0, rhs 6;  row 2 (x1): c2 -1/3, c3 1/3, rhs 2;
#   objective:  d = (0, 0, 0, 3/2, 1), z = 36.
# b1 (slack c1 basic in row 0): col_dec = 2/1 at row 0 -> [4-2, +inf]; c1 itself leaves at the low end (2), none above (-1).
# b2 (c2 = column 3): dec min(2/(1/3), 6/(1/2)) = 6 at row 0 (c1 leaves, 2); inc 2/(1/3) = 6 at row 2 (x1 leaves, 0).
# b3 (c3 = column 4): dec 2/(1/3) = 6 at row 2 (x1 leaves, 0); inc 2/(1/3) = 6 at row 0 (c1 leaves, 2).
# c1 (x1 basic in row 2): row_dec = 1/(1/3) = 3 via c3 (4), row_inc = (3/2)/(1/3) = 4.5 via c2 (3) -> [0, 7.5].
# c2 (x2 basic in row 1): row_dec = (3/2)/(1/2) = 3 via c2 (3), no negative entry -> [2, +inf], -1 above.
# duals = d of the slacks (0, 3/2, 1); both variables are basic, so their reduced costs are 0.
KAT = dict(cost_lo=[0, 2], cost_hi=[7.5, np.inf], cost_lo_at=[4, 3], cost_hi_at=[3, -1], reduced_cost=[0, 0],
           rhs_lo=[2, 6, 12], rhs_hi=[np.inf, 18, 24], rhs_lo_at=[2, 2, 0], rhs_hi_at=[-1, 0, 2], dual=[0, 1.5, 1])


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.array_equal(np.isinf(a), np.isinf(b)) and np.allclose(a[~np.isinf(a)], b[~np.isinf(b)], rtol=0, atol=tol)


def test_kat_example_input(gpu):
    p = gpu.ParseFromText(open(EXAMPLE).read())
    r = gpu.LPSolver().SolveRanged(p, "Primal Simplex")
    g = r.Ranging
    assert r.OptimalValue == 36.0 and r.Solution.tolist() == [2.0, 6.0] and r.Basis.tolist() == [2, 1, 0]
    assert g.valid
    for k, v in KAT.items():
        x = getattr(g, k)
        if k.endswith("_at"):
            assert x.tolist() == v, k
        else:
            assert _close(x, v), (k, x, v)


def test_cli_prints_the_kat():
    r = subprocess.run([CLI, "--ranging", EXAMPLE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    tail = r.stdout.split("Ranging:\n", 1)[1].splitlines()
    rows = {ln.split()[0]: ln.split()[1:] for ln in tail if ln.strip()}
    num = lambda s: float(s)
    assert _close([num(rows["x1"][0]), num(rows["x1"][1])], [0, 7.5]) and rows["x1"][2:4] == ["c3", "c2"]
    assert _close([num(rows["x2"][0]), num(rows["x2"][1])], [2, np.inf]) and rows["x2"][2:4] == ["c2", "-"]
    for i, (lo, hi, dual) in enumerate([(2, np.inf, 0), (6, 18, 1.5), (12, 24, 1)]):
        v = rows["b%d" % (i + 1)]
        assert _close([num(v[0]), num(v[1]), num(v[4])], [lo, hi, dual]), v
    assert "--ranging" in subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout


# ---- 4. semantics against independent data ------------------------------------------------------------------------
def _random_model(g, n, m, rels, sense):
    A = g.uniform(0.1, 1.0, size=(m, n))
    x0 = g.uniform(0.5, 2.0, size=n)
    ax = A @ x0
    b = np.where(rels == 0, ax + g.uniform(0.2, 1.0, m), np.where(rels == 1, ax - g.uniform(0.2, 1.0, m), ax))
    c = g.uniform(0.5, 2.0, size=n) if sense == 0 else g.uniform(0.5, 2.0, size=n)
    return c, A, b


def _expanded(c, A, b, rels, sense):
    """The tableau model the primal / repaired dual path builds (no D1): rows, their source constraint and sign."""
    rows, src, sgn, rhs = [], [], [], []
    for i in range(len(b)):
        if rels[i] == 2:
            rows += [A[i], -A[i]]; src += [i, i]; sgn += [1, -1]; rhs += [b[i], -b[i]]
        elif rels[i] == 1:
            rows.append(-A[i]); src.append(i); sgn.append(-1); rhs.append(-b[i])
        else:
            rows.append(A[i]); src.append(i); sgn.append(1); rhs.append(b[i])
    Ax = np.array(rows)
    M = np.hstack([Ax, np.eye(len(rows))])
    cint = np.concatenate([c if sense == 0 else -c, np.zeros(len(rows))])
    return M, np.array(rhs), np.array(src), np.array(sgn), cint


def _solve_basis(M, rhs, basis):
    return np.linalg.solve(M[:, basis], rhs)


def _reduced(M, cint, basis):
    y = np.linalg.solve(M[:, basis].T, cint[basis])
    return y @ M - cint                   # d_j = z_j - c_j (max form)


CASES = [("Primal Simplex", 0, "le"), ("Primal Simplex", 1, "le"), ("Dual Simplex", 0, "mix"), ("Dual Simplex", 1, "mix")]


@pytest.mark.parametrize("algo,sense,kind", CASES)
def test_semantics_against_scipy_and_the_model(gpu, algo, sense, kind):
    from scipy.optimize import linprog
    found = 0
    for seed in range(60):
        g = np.random.default_rng(1000 + seed)
        n, m = 6, 5
        rels = np.zeros(m, int) if kind == "le" else np.array([0, 0, 1, 2, 1])
        c, A, b = _random_model(g, n, m, rels, sense)
        if sense == 1 and kind == "le":
            c = -c                           # Min over <= rows: pull the variables away from 0
        prob = gpu.LPProblem.from_arrays(sense, c, A, rels, b)
        r = gpu.LPSolver(dual_flags=7).SolveRanged(prob, algo)
        if r.Status != 0 or not r.Ranging.valid:
            continue
        M, rhs, src, sgn, cint = _expanded(c, A, b, rels, sense)
        basis = r.Basis.astype(int) if r.Basis is not None else None
        xb = _solve_basis(M, rhs, basis)
        d = _reduced(M, cint, basis)
        nonbasic = np.setdiff1d(np.arange(M.shape[1]), basis)
        eq_slack = {n + k for k in range(len(src)) if rels[src[k]] == 2}
        deg_rows = [k for k in range(len(basis)) if basis[k] not in eq_slack and xb[k] < 1e-6]
        deg_cols = [j for j in nonbasic if j not in eq_slack and d[j] < 1e-6]
        if deg_rows or deg_cols:
            continue                          # non-degenerate models only
        found += 1
        rg = r.Ranging
        # SciPy / HiGHS marginals
        ub = [i for i in range(m) if rels[i] != 2]
        eq = [i for i in range(m) if rels[i] == 2]
        s_ub = np.where(rels[ub] == 1, -1.0, 1.0)
        kappa = -1.0 if sense == 0 else 1.0
        res = linprog(kappa * c, A_ub=A[ub] * s_ub[:, None], b_ub=b[ub] * s_ub, A_eq=A[eq] if eq else None,
                      b_eq=b[eq] if eq else None, bounds=[(0, None)] * n, method="highs")
        assert res.status == 0
        assert abs(-res.fun - r.OptimalValue) <= 1e-9 * (1 + abs(res.fun))     # OptimalValue is z of the max form
        want_dual = np.zeros(m)
        want_dual[ub] = kappa * s_ub * res.ineqlin.marginals
        if eq:
            want_dual[eq] = kappa * res.eqlin.marginals
        assert np.allclose(rg.dual, want_dual, rtol=1e-9, atol=1e-9), (rg.dual, want_dual)
        assert np.allclose(rg.reduced_cost, kappa * res.lower.marginals, rtol=1e-9, atol=1e-9)
        # every finite end of every RHS range: feasible just inside, the named basic variable goes negative just outside
        for i in range(m):
            rows = np.nonzero(src == i)[0]
            for end, at, out in ((rg.rhs_lo[i], rg.rhs_lo_at[i], -1), (rg.rhs_hi[i], rg.rhs_hi_at[i], 1)):
                if not np.isfinite(end):
                    assert at == -1
                    continue
                dl = 1e-6 * (1 + abs(end))
                for delta, inside in ((-out * dl, True), (out * dl, False)):
                    rh = rhs.copy()
                    rh[rows] = sgn[rows] * (end + delta)
                    x = _solve_basis(M, rh, basis)
                    if inside:
                        assert x.min() >= -1e-9, (i, end)
                    else:
                        assert x.min() < -1e-10 and basis[np.argmin(x)] == at, (i, end, at)
        # every finite end of every cost range: optimal just inside, the named column prices out just outside
        for j in range(n):
            for end, at, out in ((rg.cost_lo[j], rg.cost_lo_at[j], -1), (rg.cost_hi[j], rg.cost_hi_at[j], 1)):
                if not np.isfinite(end):
                    assert at == -1
                    continue
                dl = 1e-6 * (1 + abs(end))
                for delta, inside in ((-out * dl, True), (out * dl, False)):
                    cc = c.copy()
                    cc[j] = end + delta
                    dd = _reduced(M, np.concatenate([cc if sense == 0 else -cc, np.zeros(len(src))]), basis)[nonbasic]
                    if inside:
                        assert dd.min() >= -1e-10, (j, end)
                    else:
                        assert dd.min() < -1e-10 and nonbasic[np.argmin(dd)] == at, (j, end, at)
        if found == 3:
            break
    assert found >= 3, "too few non-degenerate optimal models among the seeds"


# ---- 5. no side effects, and the valid flag ------------------------------------------------------------------------
@pytest.mark.parametrize("algo,flags", [("Primal Simplex", 0), ("Dual Simplex", 7), ("Dual Simplex", 0), ("primal", 0)])
def test_solve_ranged_equals_solve(gpu, algo, flags):
    from linear_programming_solver_lpr381_amd import synth
    c, A, b = synth.dense_lp(40, 70, seed=21)
    rels = np.zeros(40, int)
    if algo.startswith("Dual"):
        rels[::7] = 1
        b[::7] *= 0.1
    p = gpu.LPProblem.from_arrays(0, c, A, rels, b)
    s = gpu.LPSolver(dual_flags=flags)
    r0 = s.Solve(p, algo)
    r1 = s.SolveRanged(p, algo)
    assert r0.Report == r1.Report and r0.Summary == r1.Summary and r0.Status == r1.Status
    assert r0.OptimalValue == r1.OptimalValue
    for k in ("Tableau", "Basis", "Solution"):
        x, y = getattr(r0, k), getattr(r1, k)
        assert (x is None) == (y is None), k
        if x is not None:
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), k
    assert np.array_equal(r0.Trace, r1.Trace)
    assert r0.Ranging is None and r1.Ranging is not None
    assert r1.Ranging.cost_lo.shape == (70,) and r1.Ranging.dual.shape == (40,)


def _assert_invalid(g):
    assert not g.valid
    for k in ("cost_lo", "cost_hi", "reduced_cost", "rhs_lo", "rhs_hi", "dual"):
        assert np.isnan(getattr(g, k)).all(), k
    for k in ("cost_lo_at", "cost_hi_at", "rhs_lo_at", "rhs_hi_at"):
        assert (getattr(g, k) == -1).all(), k


def test_invalid_for_unbounded_and_infeasible(gpu):
    P, K = gpu.LPProblem, gpu.Constraint
    unb = P(gpu.Sense.Max, [1.0, 1.0], [K([1.0, -1.0], gpu.Rel.LE, 1.0)])
    r = gpu.LPSolver().SolveRanged(unb, "Primal Simplex")
    assert r.Status == gpu._lib.UNBOUNDED
    _assert_invalid(r.Ranging)
    inf = P(gpu.Sense.Max, [1.0], [K([1.0], gpu.Rel.LE, 1.0), K([1.0], gpu.Rel.GE, 2.0)])
    r = gpu.LPSolver(dual_flags=7).SolveRanged(inf, "Dual Simplex")
    assert r.Status != gpu._lib.OPTIMAL
    _assert_invalid(r.Ranging)


def test_invalid_when_the_primal_path_ends_with_a_negative_rhs(gpu):
    hits = 0
    for seed in range(40):
        g = np.random.default_rng(500 + seed)
        n = 3
        A = g.uniform(0.1, 1.0, size=(3, n))
        b = g.uniform(1.0, 3.0, size=3)
        rels = np.array([2, 0, 0])                   # the expanded -b row of the equality starts infeasible
        p = gpu.LPProblem.from_arrays(0, g.uniform(0.5, 2.0, n), A, rels, b)
        r = gpu.LPSolver().SolveRanged(p, "Primal Simplex")
        if r.Status == gpu._lib.OPTIMAL and r.Ranging.min_rhs < -1e-9:
            _assert_invalid(r.Ranging)
            assert r.Ranging.min_rhs == r.Tableau[:-1, -1].min()
            hits += 1
    assert hits > 0, "no seeded equality model ended with a negative RHS"
