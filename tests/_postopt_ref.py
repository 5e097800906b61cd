"""Reference restatement of the post-optimal tableau edits (include/lpx.h, lpx_tableau_rhs_update / _objective_update /
_add_column / _add_row) and of the warm session built on them (lpx_session_*).

The four operations follow the header's summation order element for element with the same IEEE operations (segments of
SEG terms, each summed in term order from +0.0, added to base in ascending segment order, no FMA), so that device results
can be compared bit for bit.  The session's LPs run on the CPU oracle (oracle.primal_tableau / oracle.dual_tableau).
"""
from __future__ import annotations

import numpy as np

SEG = 64                       # LPX_POSTOPT_SEG
MAX, MIN = 0, 1
LE, GE, EQ = 0, 1, 2
OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT = 0, 1, 2, 3


def _combine(base, terms):
    """base (+) sum over terms, terms = [K, N] products already formed (one IEEE multiply each); returns [N]."""
    out = np.array(base, dtype=np.float64, copy=True)
    K = terms.shape[0]
    for s0 in range(0, K, SEG):
        seg = np.zeros(out.shape, dtype=np.float64)
        for k in range(s0, min(K, s0 + SEG)):
            seg = seg + terms[k]
        out = out + seg
    return out


def col_combination(T, base, cols, v):
    cols = np.asarray(cols, dtype=np.int64)
    v = np.asarray(v, dtype=np.float64)
    terms = v[:, None] * T[:, cols].T if len(cols) else np.zeros((0, T.shape[0]))
    return _combine(base, terms)


def rhs_update(T, basis, cols, v):
    T = np.array(T, dtype=np.float64, copy=True)
    T[:, -1] = col_combination(T, T[:, -1], cols, v)
    return T, np.array(basis, dtype=np.int32, copy=True)


def add_column(T, basis, cols, v, obj):
    R, C = T.shape
    base = np.zeros(R)
    base[R - 1] = obj
    col = col_combination(T, base, cols, v)
    T2 = np.zeros((R, C + 1))
    T2[:, : C - 1] = T[:, : C - 1]
    T2[:, C - 1] = col
    T2[:, C] = T[:, C - 1]
    return T2, np.array(basis, dtype=np.int32, copy=True)


def _basic_mask(basis, ncols):
    mask = np.zeros(ncols, dtype=bool)
    mask[np.asarray(basis, dtype=np.int64)] = True
    return mask


def objective_update(T, basis, rows, w, dcols=(), dd=()):
    T = np.array(T, dtype=np.float64, copy=True)
    R, C = T.shape
    m = R - 1
    base = T[m].copy()
    for j, d in zip(dcols, dd):
        base[j] = base[j] - d
    rows = np.asarray(rows, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64)
    terms = w[:, None] * T[rows] if len(rows) else np.zeros((0, C))
    out = _combine(base, terms)
    mask = _basic_mask(basis, C)
    out[mask] = 0.0
    T[m] = out
    return T, np.array(basis, dtype=np.int32, copy=True)


def add_row(T, basis, rows, w, base):
    """base: C + 1 entries in the new shape."""
    R, C = T.shape
    m, Cm = R - 1, C - 1
    base = np.asarray(base, dtype=np.float64)
    assert base.shape == (C + 1,)
    rows = np.asarray(rows, dtype=np.int64)
    w = np.asarray(w, dtype=np.float64)
    terms = w[:, None] * T[rows] if len(rows) else np.zeros((0, C))
    old = _combine(base[np.r_[0:Cm, C]], terms)          # over old columns: [0, Cm) and the RHS
    mask = _basic_mask(basis, C)
    old[mask] = 0.0
    row = np.zeros(C + 1)
    row[:Cm] = old[:Cm]
    row[Cm] = base[Cm]
    row[C] = old[Cm]
    T2 = np.zeros((R + 1, C + 1))
    T2[:m, :Cm] = T[:m, :Cm]
    T2[:m, C] = T[:m, Cm]
    T2[m] = row
    T2[m + 1, :Cm] = T[m, :Cm]
    T2[m + 1, C] = T[m, Cm]
    b2 = np.append(np.asarray(basis, dtype=np.int32), np.int32(Cm))
    return T2, b2


# ---- model level: the session restated on the CPU oracle -------------------------------------------------------------

def prepared_rows(rel):
    """(row_of, sign) of PreparedRows(dual = true, fix_d1 = true)."""
    row_of, sign = [], []
    for i, r in enumerate(rel):
        if r == EQ:
            row_of += [i, i]
            sign += [1, -1]
        else:
            row_of.append(i)
            sign.append(-1 if r == GE else 1)
    return row_of, sign


class Session:
    """lpx_session on the CPU: the same edits through the functions above, the same runs on the oracle."""

    def __init__(self, O, sense, c, A, rel, b):
        self.O = O
        self.sense = sense
        self.c = [float(v) for v in c]
        self.A = [list(map(float, a)) for a in np.asarray(A, dtype=np.float64)]
        self.rel = list(rel)
        self.b = [float(v) for v in b]
        self.sigma = -1.0 if sense == MIN else 1.0
        self.cold()

    # the tableau of the prepared model in the standard layout, solved as lpx_session_open solves it
    def cold(self):
        n = len(self.c)
        self.row_of, self.sign = prepared_rows(self.rel)
        mx = len(self.row_of)
        T = np.zeros((mx + 1, n + mx + 1))
        for k, (i, s) in enumerate(zip(self.row_of, self.sign)):
            a = np.asarray(self.A[i], dtype=np.float64)
            T[k, :n] = -a if s < 0 else a
            T[k, n + k] = 1.0
            T[k, -1] = -self.b[i] if s < 0 else self.b[i]
        cp = np.asarray(self.c, dtype=np.float64)
        cp = -cp if self.sigma < 0 else cp
        T[mx, :n] = -cp
        self.T, self.basis = T, np.arange(n, n + mx, dtype=np.int32)
        self.var_col = list(range(n))
        self.slack_col = [n + k for k in range(mx)]
        if np.all(T[:mx, -1] >= 0):
            self.status, self.trace = self.O.primal_tableau(self.T, self.basis)
        else:
            self.status, self.trace, _ = self.O.dual_tableau(self.T, self.basis, fdf_guard=10000, cleanup=1)
        self.warm = 0
        return self.status

    def _dual_if_needed(self):
        if self.T[:-1, -1].min() < -1e-9:
            self.status, self.trace, _ = self.O.dual_tableau(self.T, self.basis, fdf_guard=0, cleanup=1)
        else:
            self.status, self.trace = OPTIMAL, np.zeros((0, 2), np.int32)

    def _primal(self):
        self.status, self.trace = self.O.primal_tableau(self.T, self.basis)

    def set_rhs(self, cons, vals):
        warm = self.status == OPTIMAL
        delta, b0 = {}, list(self.b)
        for i, v in zip(cons, vals):
            delta[i] = float(v) - b0[i]
            self.b[i] = float(v)
        if not warm:
            return self.cold()
        cols, v = [], []
        for k, (i, s) in enumerate(zip(self.row_of, self.sign)):
            if i in delta:
                cols.append(self.slack_col[k])
                v.append(-delta[i] if s < 0 else delta[i])
        self.T, self.basis = rhs_update(self.T, self.basis, cols, v)
        self._dual_if_needed()
        self.warm = 1
        return self.status

    def set_cost(self, vars_, vals):
        warm = self.status == OPTIMAL
        delta, c0 = {}, list(self.c)
        for j, v in zip(vars_, vals):
            d = float(v) - c0[j]
            delta[j] = -d if self.sigma < 0 else d
            self.c[j] = float(v)
        if not warm:
            return self.cold()
        row_of_col = {int(c): r for r, c in enumerate(self.basis)}
        rows, w, dcols, dd = [], [], [], []
        for j in sorted(delta):
            col = self.var_col[j]
            if col in row_of_col:
                rows.append(row_of_col[col]); w.append(delta[j])
            else:
                dcols.append(col); dd.append(delta[j])
        self.T, self.basis = objective_update(self.T, self.basis, rows, w, dcols, dd)
        self.T = np.ascontiguousarray(self.T)
        self._primal()
        self.warm = 1
        return self.status

    def add_variable(self, c, a):
        warm = self.status == OPTIMAL
        self.c.append(float(c))
        for i, ai in enumerate(a):
            self.A[i].append(float(ai))
        if not warm:
            return self.cold()
        cols, v = [], []
        for k, (i, s) in enumerate(zip(self.row_of, self.sign)):
            ai = float(a[i])
            if ai == 0.0:
                continue
            cols.append(self.slack_col[k])
            v.append(-ai if s < 0 else ai)
        cp = -float(c) if self.sigma < 0 else float(c)
        C = self.T.shape[1]
        self.T, self.basis = add_column(self.T, self.basis, cols, v, -cp)
        self.var_col.append(C - 1)
        self._primal()
        self.warm = 1
        return self.status

    def add_constraint(self, a, rel, b):
        warm = self.status == OPTIMAL
        a = [float(v) for v in a]
        i_new = len(self.b)
        self.A.append(a); self.rel.append(rel); self.b.append(float(b))
        if not warm:
            return self.cold()
        signs = [1] if rel == LE else [-1] if rel == GE else [1, -1]
        for sg in signs:
            R, C = self.T.shape
            var_of_col = {c: j for j, c in enumerate(self.var_col)}
            base = np.zeros(C + 1)
            for j, col in enumerate(self.var_col):
                base[col] = -a[j] if sg < 0 else a[j]
            base[C - 1] = 1.0
            base[C] = -float(b) if sg < 0 else float(b)
            rows, w = [], []
            for r in range(R - 1):
                j = var_of_col.get(int(self.basis[r]), -1)
                if j < 0 or a[j] == 0.0:
                    continue
                ap = -a[j] if sg < 0 else a[j]
                rows.append(r); w.append(-ap)
            self.T, self.basis = add_row(self.T, self.basis, rows, w, base)
            self.row_of.append(i_new); self.sign.append(sg); self.slack_col.append(C - 1)
        self.T = np.ascontiguousarray(self.T)
        self._dual_if_needed()
        self.warm = 1
        return self.status

    def solution(self):
        n = len(self.c)
        x = np.zeros(n)
        col_var = {c: j for j, c in enumerate(self.var_col)}
        for r, col in enumerate(self.basis):
            if int(col) in col_var:
                x[col_var[int(col)]] = self.T[r, -1]
        return x, self.sigma * self.T[-1, -1]
