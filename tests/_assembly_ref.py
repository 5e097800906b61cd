"""NumPy restatement of branch-and-bound node and child assembly as include/lpx.h specifies it (lpx_tableau_build_node,
lpx_tableau_build_child, lpx_tableau_solution): plain float64, one IEEE operation per step, no kernel in the loop.  Checked on
the CPU against BuildTableau and against cold re-solves (tests/test_assembly_reference.py); the GPU tests compare the device
entry points with it bit for bit (tests/test_gpu_node_assembly.py).  A plain module, no fixtures."""
import numpy as np


def build_node(T0, var, coef, zero, rhs):
    """The root tableau T0 (R0 x C0, objective row last, RHS last) plus d unit rows: (T, basis) of shape R0 + d, C0 + d.
    Root rows keep the columns [0, n + m0) and move their RHS to the last column; branching row k has coef[k] at var[k], the
    signed zero zero[k] at every other structural column, 1.0 at its own slack n + m0 + k and rhs[k] last; the rest is +0.0."""
    T0 = np.asarray(T0, dtype=np.float64)
    R0, C0 = T0.shape
    d = len(var)
    n, m0 = C0 - R0, R0 - 1
    T = np.zeros((R0 + d, C0 + d), dtype=np.float64)
    T[:m0, :n + m0] = T0[:m0, :n + m0]
    T[:m0, -1] = T0[:m0, -1]
    T[-1, :n + m0] = T0[m0, :n + m0]
    T[-1, -1] = T0[m0, -1]
    for k in range(d):
        i = m0 + k
        T[i, :n] = zero[k]
        T[i, var[k]] = coef[k]
        T[i, n + m0 + k] = 1.0
        T[i, -1] = rhs[k]
    return T, np.arange(n, n + m0 + d, dtype=np.int32)


def build_child(Tp, basis_p, var, ik, is_ge, bound):
    """The parent's tableau Tp (Rp x Cp) plus the row of x_var <= bound (is_ge = 0) or x_var >= bound (is_ge = 1) written in
    the parent's basis, where x_var is basic in row ik: (T, basis) of shape Rp + 1, Cp + 1.  With t the parent's row ik, e the
    unit vector of var and r = bound at the RHS, the new row is (e + r) - t or (-e - r) + t: two roundings, in that order."""
    Tp = np.asarray(Tp, dtype=np.float64)
    Rp, Cp = Tp.shape
    mp = Rp - 1
    T = np.zeros((Rp + 1, Cp + 1), dtype=np.float64)
    T[:mp, :Cp - 1] = Tp[:mp, :Cp - 1]
    T[:mp, Cp] = Tp[:mp, Cp - 1]
    T[mp + 1, :Cp - 1] = Tp[mp, :Cp - 1]
    T[mp + 1, Cp] = Tp[mp, Cp - 1]
    t = Tp[ik].copy()
    e = np.zeros(Cp, dtype=np.float64)
    e[var] = 1.0
    r = np.zeros(Cp, dtype=np.float64)
    r[Cp - 1] = bound
    if is_ge:
        s = -e
        s = s - r
        row = s + t
    else:
        s = e + r
        row = s - t
    T[mp, :Cp - 1] = row[:Cp - 1]
    T[mp, Cp - 1] = 1.0
    T[mp, Cp] = row[Cp - 1]
    basis = np.concatenate([np.asarray(basis_p, dtype=np.int32)[:mp], np.array([Cp - 1], dtype=np.int32)])
    return T, basis


def solution(T, basis, nvars):
    """FinalizeReport's reads: x[basis[i]] = T[i, -1] for basis[i] < nvars in row order, the rest +0.0; z = T[m, -1]."""
    T = np.asarray(T, dtype=np.float64)
    m = T.shape[0] - 1
    x = np.zeros(nvars, dtype=np.float64)
    for i in range(m):
        if 0 <= basis[i] < nvars:
            x[basis[i]] = T[i, -1]
    return x, T[m, -1]


def binary_relaxation(seed, n=8, m=4):
    """A small integer-data LP: m knapsack rows over n columns and the rows x_j <= 1.  Returns (c, A, b) of Max c x, A x <= b."""
    g = np.random.default_rng(seed)
    A = g.integers(0, 10, size=(m, n)).astype(np.float64)
    b = np.floor(0.5 * A.sum(axis=1))
    c = g.integers(1, 21, size=n).astype(np.float64)
    return c, np.vstack([A, np.eye(n)]), np.concatenate([b, np.ones(n)])


def fractional_row(T, basis, n, tol=1e-6):
    """(var, row) of the first basic structural variable with a fractional value, or None."""
    for i, j in enumerate(basis):
        v = T[i, -1]
        if j < n and abs(v - np.round(v)) > tol:
            return int(j), i
    return None
