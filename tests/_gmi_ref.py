"""Reference restatement of the GMI cutting-plane round and loop (include/lpx.h, lpx_tableau_gmi_round / lpx_solve_cuts).

The round is restated in numpy from the header's definitions, element for element with the same IEEE operations, so that
the device result can be compared bit for bit.  The LPs run on the CPU oracle (oracle.primal_tableau / oracle.dual_tableau).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List

import numpy as np

MAX, MIN = 0, 1
LE, GE, EQ = 0, 1, 2
OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT = 0, 1, 2, 3
CUT_INTEGER, CUT_INCOMPLETE = 0, 10


@dataclass
class CutOpts:
    cuts_per_round: int = 8
    max_rounds: int = 50
    max_active: int = 64
    purge: int = 1
    away: float = 1e-3
    coef_eps: float = 1e-9
    max_dynamism: float = 1e6
    purge_tol: float = 1e-9
    int_tol: float = 1e-6


def alphas(row, isint, nb, f0, ce):
    """alpha_j of the cut of one row (row = T[r, :C-1])."""
    a = np.asarray(row, dtype=np.float64)
    with np.errstate(all="ignore"):
        fi = a - np.floor(a)
        ai = np.where((fi <= ce) | (fi >= 1.0 - ce), 0.0, np.where(fi <= f0, fi / f0, (1.0 - fi) / (1.0 - f0)))
        ac = np.where(np.abs(a) <= ce, 0.0, np.where(a > 0, a / f0, (-a) / (1.0 - f0)))
    al = np.where(isint, ai, ac)
    return np.where(nb, al, 0.0)


def gmi_round(T, basis, is_int, n_mask, first_cut_col, o: CutOpts, Rcap, Ccap):
    """One round.  Returns (T', basis', src_rows, purged_cols); T' is T itself when nothing changes."""
    T = np.asarray(T, dtype=np.float64)
    basis = np.asarray(basis, dtype=np.int32)
    R, C = T.shape
    m, Cm = R - 1, C - 1
    nint = min(n_mask, first_cut_col)
    isint = np.zeros(Cm, dtype=bool)
    isint[:nint] = np.asarray(is_int[:nint], dtype=bool)
    nb = np.ones(Cm, dtype=bool)
    nb[basis[(basis >= 0) & (basis < Cm)]] = False
    b = T[:m, Cm]
    f0 = b - np.floor(b)
    cand = isint[basis] & (f0 >= o.away) & (f0 <= 1.0 - o.away)
    passing = []
    for r in np.nonzero(cand)[0]:
        al = alphas(T[r, :Cm], isint, nb, f0[r], o.coef_eps)
        amax = al.max() if al.size else 0.0
        nz = al[al > 0]
        amin = nz.min() if nz.size else np.inf
        if not (amax > o.max_dynamism * amin):
            passing.append(int(r))
    prow = []
    if o.purge:
        for r in range(m):
            if first_cut_col <= basis[r] < Cm and b[r] > o.purge_tol:
                prow.append(r)
    pcol = sorted(int(basis[r]) for r in prow)
    P = len(prow)
    K = min(o.cuts_per_round, Rcap - (R - P), Ccap - (C - P), len(passing))
    K = max(K, 0)
    src = sorted(passing, key=lambda r: (abs(f0[r] - 0.5), r))[:K]
    if K == 0 and P == 0:
        return T, basis, [], []
    keep_r = [r for r in range(m) if r not in set(prow)]
    keep_c = [j for j in range(Cm) if j not in set(pcol)]
    R2, C2 = R - P + K, C - P + K
    T2 = np.zeros((R2, C2))
    nk = len(keep_r)
    T2[:nk, :Cm - P] = T[np.ix_(keep_r, keep_c)]
    T2[:nk, C2 - 1] = T[keep_r, Cm]
    for k, r in enumerate(src):
        al = alphas(T[r, :Cm], isint, nb, f0[r], o.coef_eps)[keep_c]
        T2[nk + k, :Cm - P] = np.where(al == 0.0, 0.0, -al)
        T2[nk + k, Cm - P + k] = 1.0
        T2[nk + k, C2 - 1] = -1.0
    T2[R2 - 1, :Cm - P] = T[m, keep_c]
    T2[R2 - 1, C2 - 1] = T[m, Cm]
    newcol = {j: i for i, j in enumerate(keep_c)}
    basis2 = np.array([newcol[int(basis[r])] for r in keep_r] + [Cm - P + k for k in range(K)], dtype=np.int32)
    return np.ascontiguousarray(T2), basis2, src, pcol


def prepare(sense, c, A, rel, b):
    """PrepareForTableauDual with defect D1 fixed: (c', A', b') of the Max model with <= rows."""
    c = np.asarray(c, dtype=np.float64)
    if sense == MIN:
        c = -c
    rows, rhs = [], []
    for a, r, bi in zip(np.asarray(A, dtype=np.float64), rel, b):
        if r == EQ:
            rows.append(a.copy()); rhs.append(float(bi))
            rows.append(a * -1); rhs.append(-float(bi))
        elif r == GE:
            rows.append(a * -1); rhs.append(float(bi) * -1)
        else:
            rows.append(a.copy()); rhs.append(float(bi))
    return c, np.array(rows).reshape(len(rows), len(c)), np.array(rhs)


def build_tableau(c, A, b):
    m, n = A.shape
    T = np.zeros((m + 1, n + m + 1))
    T[:m, :n] = A
    T[np.arange(m), n + np.arange(m)] = 1.0
    T[:m, -1] = b
    T[m, :n] = -c
    return T, (n + np.arange(m)).astype(np.int32)


@dataclass
class GmiResult:
    status: int
    z: float                   # final LP bound in the user's sense
    x: np.ndarray
    T: np.ndarray
    basis: np.ndarray
    trace: np.ndarray
    rounds: int
    added: int
    purged: int
    root_z: float
    src_rows: List[List[int]] = field(default_factory=list)
    cuts: np.ndarray = None    # x-space LE rows (A, B)
    bounds: List[float] = field(default_factory=list)
    lp_points: List[np.ndarray] = field(default_factory=list)   # x of the LP each round cut from


def gmi_solve(O, sense, c, A, rel, b, o: CutOpts = None, max_iter=10000) -> GmiResult:
    o = o or CutOpts()
    n = len(c)
    cp, Ap, bp = prepare(sense, c, A, rel, b)
    T, basis = build_tableau(cp, Ap, bp)
    R, C = T.shape
    mx, first = R - 1, C - 1
    sigma = -1.0 if sense == MIN else 1.0
    is_int = np.zeros(first, dtype=np.uint8)
    is_int[:n] = 1
    for k in range(mx):
        is_int[n + k] = 1 if (bp[k] == np.floor(bp[k]) and np.all(Ap[k] == np.floor(Ap[k]))) else 0
    rowA = [Ap[k].copy() for k in range(mx)]
    rowB = [float(bp[k]) for k in range(mx)]
    colcut: List[int] = []
    Rcap, Ccap = R + o.max_active, C + o.max_active
    traces = []
    if np.all(T[:mx, -1] >= 0):
        st, tr = O.primal_tableau(T, basis, max_iter=max_iter)
    else:
        st, tr, _ = O.dual_tableau(T, basis, fdf_guard=max_iter, max_iter=max_iter, cleanup=1)
    assert st != ITER_LIMIT
    traces.append(tr)
    res = GmiResult(st, 0.0, None, None, None, None, 0, 0, 0, sigma * T[-1, -1])
    status = st
    if st == OPTIMAL:
        status = CUT_INCOMPLETE
        while True:
            m = T.shape[0] - 1
            rhs = T[:m, -1]
            frac = [r for r in range(m) if basis[r] < first and is_int[basis[r]]
                    and abs(rhs[r] - np.rint(rhs[r])) > o.int_tol]
            if not frac:
                status = CUT_INTEGER
                break
            if res.rounds >= o.max_rounds:
                break
            xlp = np.zeros(n)
            for r in range(m):
                if basis[r] < n:
                    xlp[basis[r]] = rhs[r]
            T2, b2, src, pcol = gmi_round(T, basis, is_int, first, first, o, Rcap, Ccap)
            for p in sorted(pcol, reverse=True):
                del colcut[p - first]
            res.purged += len(pcol)
            T, basis = T2, b2
            K = len(src)
            if K == 0:
                break
            Rn, Cn = T.shape
            nold = Cn - 1 - K
            for k in range(K):
                e = T[Rn - 1 - K + k]
                a = np.zeros(n)
                cst = 0.0
                for j in range(nold):
                    if e[j] == 0.0:
                        continue
                    al = -e[j]
                    if j < n:
                        a[j] += al
                        continue
                    i = j - n if j < first else colcut[j - first]
                    a -= al * rowA[i]
                    cst += al * rowB[i]
                colcut.append(len(rowA))
                rowA.append(-a)
                rowB.append(cst - 1.0)
            res.added += K
            res.src_rows.append(list(src))
            res.lp_points.append(xlp)
            T = np.ascontiguousarray(T)
            st, tr, _ = O.dual_tableau(T, basis, fdf_guard=0, max_iter=max_iter, cleanup=1)
            assert st != ITER_LIMIT
            traces.append(tr)
            res.rounds += 1
            res.bounds.append(sigma * T[-1, -1])
            if st == INFEASIBLE:
                status = INFEASIBLE
                break
            if st != OPTIMAL:
                status = st
                break
    x = np.zeros(n)
    m = T.shape[0] - 1
    for r in range(m):
        if basis[r] < n:
            x[basis[r]] = T[r, -1]
    res.status, res.x, res.T, res.basis = status, x, T, basis
    res.z = sigma * T[-1, -1]
    res.trace = np.concatenate([t.reshape(-1, 2) for t in traces]) if traces else np.zeros((0, 2), np.int32)
    res.cuts = np.array([np.append(rowA[g], rowB[g]) for g in range(mx, len(rowA))]).reshape(-1, n + 1)
    return res


def enumerate_points(A, rel, b, ub):
    """Every integer x >= 0 with x_j <= ub[j] that satisfies the model's rows (exact integer data)."""
    import itertools
    A = np.asarray(A, dtype=np.float64)
    pts = []
    for x in itertools.product(*[range(int(u) + 1) for u in ub]):
        x = np.array(x, dtype=np.float64)
        v = A @ x
        ok = True
        for vi, r, bi in zip(v, rel, b):
            if (r == LE and vi > bi + 1e-9) or (r == GE and vi < bi - 1e-9) or (r == EQ and abs(vi - bi) > 1e-9):
                ok = False
                break
        if ok:
            pts.append(x)
    return np.array(pts).reshape(-1, A.shape[1])


def random_ip(rng, n, m, ub=6):
    """A bounded random IP with integer data: Max c.x over A x <= b (A >= 0) plus the box rows x_j <= ub, some rows >=."""
    c = rng.integers(1, 10, n).astype(float)
    A = rng.integers(0, 8, (m, n)).astype(float)
    A[A.sum(axis=1) == 0, 0] = 1.0
    b = rng.integers(5, 30, m).astype(float)
    rel = [LE] * m
    box = np.eye(n)
    A = np.vstack([A, box])
    b = np.concatenate([b, np.full(n, float(ub))])
    rel = rel + [LE] * n
    if rng.random() < 0.5:      # one >= row that the origin violates: the root LP goes through the dual path
        A = np.vstack([A, np.ones(n)])
        b = np.append(b, 1.0)
        rel = rel + [GE]
    return MAX, c, A, rel, b
