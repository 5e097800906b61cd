"""GPU checks of the post-optimal edits at every tile edge of lpx_postopt.hip (the edges come from the kernel's own
constants through tests/_exact_sums.py):
A. the four tableau operations bit for bit against tests/_postopt_ref.py with K, R and C around every term, row, column
   and combine tile, on handles of exact capacity, with C + 1 a multiple of 16, with a spare 16-column pad, and with a
   dead region holding NaN and +-inf; nothing outside the written window moves;
B. the same results against the exact sums (error-free products, math.fsum), and the entries that must be exact;
C. the loop the session runs after each edit, on the edited handle, bit for bit against the oracle: the default path, a
   graph captured on the handle before the edit, the streaming and the resident paths;
D. sessions at tile-crossing sizes against HiGHS and cold solves;
E. one handle through a GMI round, a new row, ranging, a workspace-growing cost change and a purging GMI round;
F. the new column and the new row at the headline shape."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_sums as X                                                        # noqa: E402
import _gmi_ref as G                                                           # noqa: E402
import _postopt_ref as P                                                       # noqa: E402
from test_gpu_postopt import _check, _random_model, _same, _solved_tableau, headline   # noqa: E402,F401
from test_gpu_ranging import assert_ranging_equal, ref_ranging                # noqa: E402

pytestmark = pytest.mark.gpu

TILE = X.postopt_tiling()
SEG, NT, CR, CT, RT = (TILE[k] for k in ("SEG", "NT", "CR", "CT", "RT"))
CAPS = ("exact", "pad16", "stale")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _capacity(kind, R, C, grow):
    """exact: no room beyond what the edit needs; pad16: a spare 16-column pad and more; stale: a shrunk handle."""
    if kind == "exact":
        return R + grow, C + grow
    if kind == "pad16":
        return R + grow + 2, C + grow + 17
    return R + grow + 5, C + grow + 40


def _dead(g, kind, Rcap, Ccap):
    """What the handle holds before the live tableau goes in: NaN and +-inf for a shrunk handle, finite values else."""
    S = g.uniform(-9.0, 9.0, size=(Rcap, Ccap))
    if kind == "stale":
        u = g.random(S.shape)
        S[u < 0.25] = np.nan
        S[(u >= 0.25) & (u < 0.5)] = np.inf
        S[(u >= 0.5) & (u < 0.75)] = -np.inf
    return S


def _edit(gpu, g, kind, T, basis, grow, op, want):
    """op on a handle of capacity _capacity(kind) whose dead region holds _dead(kind); the live window must equal `want`
    bit for bit, and every entry outside it must still hold what it held."""
    R, C = T.shape
    Rcap, Ccap = _capacity(kind, R, C, grow)
    S = _dead(g, kind, Rcap, Ccap)
    Tw, bw = want
    with gpu.DeviceTableau(Rcap, Ccap) as dt:
        dt.upload(S)
        dt.set_shape(R, C)
        dt.upload(T, basis)
        op(dt)
        assert (dt.R, dt.C) == Tw.shape
        Tg, bg = dt.download()
        dt.set_shape(Rcap, Ccap)
        full, _ = dt.download()
    assert np.array_equal(bg, bw)
    assert _same(Tg, Tw), np.argwhere(_bits(Tg) != _bits(Tw))[:5]
    dead = np.ones((Rcap, Ccap), dtype=bool)
    dead[: Tw.shape[0], : Tw.shape[1]] = False
    assert np.array_equal(_bits(full)[dead], _bits(S)[dead]), "an edit wrote outside its window"
    return Tg


def _sample(g, n, *tiles):
    extra = g.choice(n, size=min(n, 16), replace=False)
    return sorted(set(X.tile_edges(n, *tiles)) | set(int(i) for i in extra))


# ---- A + B. tile-edge matrix ------------------------------------------------------------------------------------------
COL_SHAPES = [(R, R + n) for R, n in zip(X.col_rows(TILE), (16, 44, 64, 144, 158))]   # C + 1 = 48, 320, 704: x16


@pytest.mark.parametrize("R,C", COL_SHAPES)
def test_column_ops_at_tile_edges(gpu, R, C):
    T, basis = _solved_tableau(gpu, R, C, seed=R * 13 + C)
    m = R - 1
    g = np.random.default_rng(R + 7 * C)
    rows = _sample(g, R, CR, NT)
    for i, K in enumerate(X.col_terms(TILE)):
        kind = CAPS[i % 3]
        cols = g.integers(0, C - 1, size=K).astype(np.int32)
        for k in range(0, K - CT, 37):
            cols[k + CT] = cols[k]                                 # the same column again one term tile later
        v = g.standard_normal(K)
        # RHS update
        Tg = _edit(gpu, g, kind, T, basis, 0, lambda dt: dt.rhs_update(cols, v), P.rhs_update(T, basis, cols, v))
        bad = X.check_col(T, [T[:, -1]], cols, v, Tg[:, -1], rows, SEG)
        assert not bad, ("rhs", K, kind, bad[:3])
        # new column: the RHS moves right unchanged
        obj = float(g.standard_normal())
        Tg = _edit(gpu, g, kind, T, basis, 1, lambda dt: dt.add_column(cols, v, obj), P.add_column(T, basis, cols, v, obj))
        base = np.zeros(R)
        base[m] = obj
        bad = X.check_col(T, [base], cols, v, Tg[:, C - 1], rows, SEG)
        assert not bad, ("col", K, kind, bad[:3])
        assert _same(Tg[:, C], T[:, C - 1])


@pytest.mark.parametrize("R,C", X.row_shapes(TILE))
def test_row_ops_at_tile_edges(gpu, R, C):
    T, basis = _solved_tableau(gpu, R, C, seed=R * 17 + C)
    m, Cm = R - 1, C - 1
    g = np.random.default_rng(R + 11 * C)
    isb = np.zeros(C, dtype=bool)
    isb[basis] = True
    nb = np.flatnonzero(~isb[:Cm])
    cols = _sample(g, C, NT, RT)
    for i, K in enumerate(X.row_terms(TILE, m)):
        kind = CAPS[i % 3]
        rows = g.integers(0, m, size=K).astype(np.int32)
        w = g.standard_normal(K)
        # cost change with sparse deltas on nonbasic columns (on every one of them once: Kd > m where C allows)
        dcols = g.choice(nb, size=len(nb) if i == 0 else min(5, len(nb)), replace=False).astype(np.int32)
        dd = g.standard_normal(len(dcols))
        Tg = _edit(gpu, g, kind, T, basis, 0, lambda dt: dt.objective_update(rows, w, dcols, dd),
                   P.objective_update(T, basis, rows, w, dcols, dd))
        d = np.zeros(C)
        d[dcols] = -dd
        live = [j for j in sorted(set(cols) | set(dcols.tolist())) if not isb[j]]
        bad = X.check_row(T, [T[m], d], rows, w, Tg[m], live, SEG)
        assert not bad, ("obj", K, kind, bad[:3])
        assert X.plus_zero(Tg[m, isb])
        # new row: basic columns +0.0, the new slack entry as given, zero slack entries in the old rows, the RHS moved
        base = g.standard_normal(C + 1)
        base[Cm] = 1.0
        Tg = _edit(gpu, g, kind, T, basis, 1, lambda dt: dt.add_row(rows, w, base), P.add_row(T, basis, rows, w, base))
        out = [j for j in cols if j < Cm and not isb[j]]
        bad = X.check_row(T, [base], rows, w, Tg[m], out + [C], SEG, src=out + [Cm])
        assert not bad, ("row", K, kind, bad[:3])
        assert _bits(Tg[m, Cm]) == _bits(base[Cm]) and X.plus_zero(Tg[m, :Cm][isb[:Cm]])
        assert X.plus_zero(Tg[:m, Cm]) and X.plus_zero(Tg[m + 1, Cm])
        assert _same(Tg[:m, C], T[:m, Cm]) and _same(Tg[m + 1, :Cm], T[m, :Cm]) and _same(Tg[m + 1, C:], T[m, Cm:])


# ---- C. the loop after the edit ---------------------------------------------------------------------------------------
LOOP_SHAPES = [(NT + 1, 2 * NT + CR + 1), (2 * NT + CR + 1, RT + NT + 1)]


def _loop_edits(T, basis, g):
    """The four edits as the session makes them on an optimal tableau, each moving the optimum: (name, dual, op, want)."""
    R, C = T.shape
    m, n = R - 1, C - R
    row_of = {int(c): r for r, c in enumerate(basis)}
    # b: the slack columns, with repeats, scaled until some RHS goes negative
    cols = (n + g.integers(0, m, size=CT + SEG + 1)).astype(np.int32)
    v = g.standard_normal(len(cols)) * (0.05 * n)
    while P.rhs_update(T, basis, cols, v)[0][:m, -1].min() >= -1e-9:
        v = v * 2.0
    out = [("rhs", True, lambda dt: dt.rhs_update(cols, v), P.rhs_update(T, basis, cols, v))]
    # c: basic variables as row weights, nonbasic ones as sparse deltas
    js = g.choice(n, size=min(n, 2 * SEG + 1), replace=False)
    delta = {int(j): float(g.uniform(0.3, 1.5)) for j in js}
    rows = np.array([row_of[j] for j in sorted(delta) if j in row_of], dtype=np.int32)
    w = np.array([delta[j] for j in sorted(delta) if j in row_of])
    dcols = np.array([j for j in sorted(delta) if j not in row_of], dtype=np.int32)
    dd = np.array([delta[j] for j in sorted(delta) if j not in row_of])
    out.append(("cost", False, lambda dt: dt.objective_update(rows, w, dcols, dd),
                P.objective_update(T, basis, rows, w, dcols, dd)))
    # a new variable over every slack column, priced to enter
    a = g.uniform(0.2, 3.0, size=m)
    scols = np.arange(n, n + m, dtype=np.int32)
    obj = -(1.5 * float(T[m, n:n + m] @ a) + 1.0)
    out.append(("col", False, lambda dt: dt.add_column(scols, a, obj), P.add_column(T, basis, scols, a, obj)))
    # a new <= row that cuts the optimum off: weights -a_j of the basic structural variables
    ar = g.uniform(0.2, 3.0, size=n)
    x = np.zeros(n)
    for r, c in enumerate(basis):
        if c < n:
            x[c] = T[r, -1]
    base = np.zeros(C + 1)
    base[:n] = ar
    base[C - 1] = 1.0
    base[C] = 0.9 * float(ar @ x)
    rr = np.array([r for r, c in enumerate(basis) if c < n], dtype=np.int32)
    wr = -ar[basis[rr]]
    out.append(("row", True, lambda dt: dt.add_row(rr, wr, base), P.add_row(T, basis, rr, wr, base)))
    return out


@pytest.mark.parametrize("R,C", LOOP_SHAPES)
def test_loop_after_each_edit_matches_the_oracle(gpu, oracle, R, C):
    T, basis = _solved_tableau(gpu, R, C, seed=R + C, pivots=10000)
    g = np.random.default_rng(R * 3 + C)
    batch = 16
    # the resident path required on the smaller shape; automatic and eager on the larger one
    resident = {"resident": 1} if (R, C) == LOOP_SHAPES[0] else {"resident": 0, "use_graph": 0}
    for name, dual, op, (Tw, bw) in _loop_edits(T, basis, g):
        Tr, br = np.ascontiguousarray(Tw).copy(), bw.copy()
        if dual:
            st_ref, tr_ref, _ = oracle.dual_tableau(Tr, br, fdf_guard=0, cleanup=1)
        else:
            st_ref, tr_ref = oracle.primal_tableau(Tr, br)
        assert len(tr_ref) > 0, name
        for how in ("default", "graph", "streaming", "resident"):
            kw = {"use_graph": 1, "batch": batch} if how == "graph" else \
                 {"resident": -1} if how == "streaming" else resident if how == "resident" else {}
            with gpu.DeviceTableau.with_capacity(T, basis, R + 2, C + 2) as dt:
                if how == "graph":                                 # graphs of both loops captured at this batch
                    assert dt.primal_run(use_graph=1, batch=batch)[0] == 0
                    assert dt.dual_run(fdf_guard=0, cleanup=1, use_graph=1, batch=batch)[0] == 0
                    T0, b0 = dt.download()
                    assert _same(T0, T) and np.array_equal(b0, basis)
                op(dt)
                if dual:
                    status, _ = dt.dual_run(fdf_guard=0, cleanup=1, **kw)
                else:
                    status, _ = dt.primal_run(**kw)
                Tg, bg = dt.download()
                tr = dt.trace()
            assert status == st_ref, (name, how)
            assert tr.tolist() == tr_ref.tolist(), (name, how)
            assert np.array_equal(bg, br), (name, how)
            assert _same(Tg, Tr), (name, how)


# ---- D. sessions at tile-crossing sizes -------------------------------------------------------------------------------
def _edit_session(rng, ses, kind):
    prob = ses.Problem
    n, m = prob.NumVars, len(prob.Constraints)
    if kind == "rhs":
        i = int(rng.integers(0, m))
        return ses.ChangeRHS(i, prob.Constraints[i].B * float(rng.uniform(0.5, 1.6)))
    if kind == "cost":
        j = int(rng.integers(0, n))
        return ses.ChangeCost(j, prob.C[j] * float(rng.uniform(0.3, 2.5)))
    if kind == "col":
        return ses.AddActivity(float(rng.uniform(0.5, 2.5)), rng.uniform(0.2, 3.0, size=m))
    a = rng.uniform(0.2, 3.0, size=n)
    x = ses.Result.Solution if ses.Result.Status == 0 else np.ones(n)
    return ses.AddConstraint(a, kind, float(a @ x) * float(rng.uniform(0.7, 1.1)))


def _session_steps(gpu, seed, n, m):
    rng = np.random.default_rng(4200 + seed)
    prob = _random_model(gpu, rng, n, m)
    kinds = ["rhs", "cost", "col", P.LE, P.GE, P.EQ, "rhs", "cost"]
    kinds = [kinds[i] for i in rng.permutation(len(kinds))]
    with gpu.LPSolver().Open(prob, extra_rows=16, extra_cols=16) as ses:
        _check(gpu, ses, ses.Result)
        for kind in kinds:
            was_optimal = ses.Result.Status == 0
            r = _edit_session(rng, ses, kind)
            if was_optimal:
                assert r.Aux[0] == 1.0, kind
            _check(gpu, ses, r)
    return int(prob.ObjectiveSense)


# Min models at 600 x 300 (prepared tableaux past 256 rows and 512 columns).  The Max models of random_model at that size run
# the reference's Dual Simplex past its iteration cap from the slack basis (the open solve or the cold check, with 10^5
# pivots as with 10^4); the Max case is the one found at 400 x 180, whose tableau crosses 512 columns but not 256 rows.
@pytest.mark.parametrize("seed,n,m,sense", [(0, 600, 300, P.MIN), (3, 600, 300, P.MIN), (19, 400, 180, P.MAX)])
def test_sessions_at_tile_crossing_sizes_against_highs(gpu, seed, n, m, sense):
    assert _session_steps(gpu, seed, n, m) == sense


# ---- E. one handle, mixed operations ----------------------------------------------------------------------------------
def test_one_handle_through_gmi_row_ranging_cost_and_purge(gpu, oracle):
    from test_gpu_gmi import _solved_lp
    T, basis = _solved_lp(oracle, 411, 300, seed=8)
    R, C = T.shape
    first = C - 1
    is_int = np.ones(first, np.uint8)
    Rcap, Ccap = R + 40, C + 40
    g = np.random.default_rng(8)

    def same(dt, Tw, bw):
        Tg, bg = dt.download()
        assert Tg.shape == Tw.shape and _same(Tg, Tw) and np.array_equal(bg, bw)

    with gpu.DeviceTableau.with_capacity(T, basis, Rcap, Ccap) as dt:
        # 1. a GMI round in place (the cut round's workspace)
        o = G.CutOpts(cuts_per_round=8)
        T1, b1, src, _ = G.gmi_round(T.copy(), basis.copy(), is_int, first, first, o, Rcap, Ccap)
        s, p = dt.gmi_round(is_int, first, opts=gpu.CutOpts(**vars(o)).to_c())
        assert list(s) == list(src) and len(src) > 0 and not len(p)
        same(dt, T1, b1)
        # 2. a new row (the post-optimal workspace)
        m1, C1 = T1.shape[0] - 1, T1.shape[1]
        rows = g.integers(0, m1, size=m1).astype(np.int32)
        w = g.standard_normal(m1)
        base = g.standard_normal(C1 + 1)
        base[C1 - 1] = 1.0
        T2, b2 = P.add_row(T1, b1, rows, w, base)
        dt.add_row(rows, w, base)
        same(dt, T2, b2)
        # 3. ranging (its own workspace layout over the same buffer); the handle is left alone
        assert_ranging_equal(dt.ranging(), ref_ranging(T2, b2))
        same(dt, T2, b2)
        # 4. a cost change with enough terms to grow the workspace past every earlier use
        m2 = T2.shape[0] - 1
        K = 48 * SEG
        rows = g.integers(0, m2, size=K).astype(np.int32)
        w = g.standard_normal(K)
        nb = np.setdiff1d(np.arange(T2.shape[1] - 1), b2)
        dcols = nb[:7].astype(np.int32)
        dd = g.standard_normal(len(dcols))
        T3, b3 = P.objective_update(T2, b2, rows, w, dcols, dd)
        dt.objective_update(rows, w, dcols, dd)
        same(dt, T3, b3)
        # 5. a GMI round that purges the cut rows, in the grown workspace
        op = G.CutOpts(cuts_per_round=8, purge_tol=-2.0)
        T4, b4, src4, pcol4 = G.gmi_round(np.ascontiguousarray(T3), b3.copy(), is_int, first, first, op, Rcap, Ccap)
        s4, p4 = dt.gmi_round(is_int, first, opts=gpu.CutOpts(**vars(op)).to_c())
        assert len(pcol4) > 0 and list(p4) == list(pcol4) and list(s4) == list(src4)
        same(dt, T4, b4)


# ---- F. headline shape ------------------------------------------------------------------------------------------------
def test_headline_add_column_and_add_row_all_rows(gpu, headline):
    T, basis = headline
    R, C = T.shape
    m, n = R - 1, C - R
    g = np.random.default_rng(13)
    cols, v = np.arange(n, n + m, dtype=np.int32), g.standard_normal(m)
    Tw, bw = P.add_column(T, basis, cols, v, -1.25)
    with gpu.DeviceTableau.with_capacity(T, basis, R + 1, C + 1) as dt:
        dt.add_column(cols, v, -1.25)
        assert (dt.R, dt.C) == (R, C + 1)
        Tg, bg = dt.download()
    assert _same(Tg, Tw) and np.array_equal(bg, bw)
    base = np.zeros(R)
    base[m] = -1.25
    assert not X.check_col(T, [base], cols, v, Tg[:, C - 1], _sample(g, R, CR, NT), SEG)
    del Tw, Tg
    rows, w = np.arange(m, dtype=np.int32), g.standard_normal(m)
    base = g.standard_normal(C + 1)
    base[C - 1] = 1.0
    Tw, bw = P.add_row(T, basis, rows, w, base)
    with gpu.DeviceTableau.with_capacity(T, basis, R + 1, C + 1) as dt:
        dt.add_row(rows, w, base)
        assert (dt.R, dt.C) == (R + 1, C + 1)
        Tg, bg = dt.download()
    assert _same(Tg, Tw) and np.array_equal(bg, bw)
    isb = np.zeros(C, dtype=bool)
    isb[basis] = True
    out = [j for j in _sample(g, C - 1, NT, RT) if not isb[j]]
    assert not X.check_row(T, [base], rows, w, Tg[m], out + [C], SEG, src=out + [C - 1])
