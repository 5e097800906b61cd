"""NumPy restatement of lpx_solve_packed (include/lpx.h), model by model: the preparation of lpx_solve_bounded and the extraction
of its result, in the operation order the header states, around the loop and the solution of tests/_bounded_ref.py.  Written
from the contract, not from the kernel.  Test infrastructure: tests/test_gpu_packed.py compares the device against it bit for bit;
tests/test_packed_ref.py pins it to hand-computed values."""
from collections import namedtuple

import numpy as np

import _bounded_ref as B

EINVAL, E_NEG_RHS = -1, -11
MAX, MIN = 0, 1

Prepared = namedtuple("Prepared", "status T basis ub constant shifted")
Solved = namedtuple("Solved", "status x value events counts z basis at_upper")


def prepare(c, A, b, lower=None, upper=None, sense=MAX):
    """The tableau of one model as the loop sees it.  status 0, or the error and nothing else."""
    c = np.asarray(c, dtype=np.float64); A = np.asarray(A, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    m, n = A.shape
    lo = None if lower is None else np.broadcast_to(np.asarray(lower, dtype=np.float64), (n,))      # a scalar: every variable
    up = None if upper is None else np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,))
    for j in range(n):                                  # the bounds first
        l = 0.0 if lo is None else lo[j]
        u = np.inf if up is None else up[j]
        if not np.isfinite(l) or not (u >= l):
            return Prepared(EINVAL, None, None, None, 0.0, False)
    cm = -c if sense == MIN else c.copy()               # Min negates c
    bp = b.copy()
    if lo is not None:                                  # b' = b - A l: j ascending, one multiply and one subtract per non-zero l_j
        for j in range(n):
            if lo[j] != 0.0:
                prod = A[:, j] * lo[j]
                bp = bp - prod
    if (bp < -1e-9).any():
        return Prepared(E_NEG_RHS, None, None, None, 0.0, False)
    constant, shifted = np.float64(0.0), False          # c.l over the user's c
    if lo is not None:
        for j in range(n):
            if lo[j] != 0.0:
                prod = c[j] * lo[j]
                constant = constant + prod
                shifted = True
    T = np.zeros((m + 1, n + m + 1))
    T[:m, :n] = A
    T[np.arange(m), n + np.arange(m)] = 1.0
    T[:m, n + m] = bp
    T[m, :n] = -cm                                      # a negation: a zero cost gives -0.0
    basis = np.arange(n, n + m, dtype=np.int32)
    ub = np.full(n + m, np.inf)
    if up is not None:
        for j in range(n):
            ub[j] = up[j] if np.isinf(up[j]) else up[j] - (0.0 if lo is None else lo[j])
    return Prepared(0, T, basis, ub, float(constant), shifted)


def solve(c, A, b, lower=None, upper=None, sense=MAX, max_iter=10000, eps=1e-9, tol=1e-9):
    """One model of a packed call: what status[i], x, value, rec, basis and at_upper hold."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    P = prepare(c, A, b, lower, upper, sense)
    if P.status != 0:
        return Solved(P.status, np.zeros(n), 0.0, 0, (0, 0, 0), 0.0, np.zeros(m, dtype=np.int32), np.zeros(n, dtype=np.uint8))
    status, T, basis, flip, trace, counts = B.run(P.T, P.basis, P.ub, eps=eps, tol=tol, max_iter=max_iter)
    x, z, at_upper = B.solution(T, basis, flip, P.ub, n)
    x = x.copy()
    if lower is not None:                               # every j, a zero lower bound too: -0.0 becomes +0.0
        x = x + np.broadcast_to(np.asarray(lower, dtype=np.float64), (n,))
    value = z
    if P.shifted or sense == MIN:
        value = -z if sense == MIN else z
        if P.shifted:
            value = value + P.constant
    return Solved(status, x, float(value), len(trace), counts, float(z), basis, at_upper)


def solve_all(c, A, b, lower=None, upper=None, sense=MAX, **kw):
    """A packed batch: arrays with or without the batch axis, as LPSolver.SolvePacked takes them."""
    c, A, b = (np.asarray(v, dtype=np.float64) for v in (c, A, b))
    lower = None if lower is None else np.asarray(lower, dtype=np.float64)
    upper = None if upper is None else np.asarray(upper, dtype=np.float64)
    sizes = [v.shape[0] for v, nd in ((c, 2), (A, 3), (b, 2), (lower, 2), (upper, 2)) if v is not None and v.ndim == nd]
    count = sizes[0] if sizes else 1

    def pick(v, nd, i):
        return None if v is None else (v[i] if v.ndim == nd else v)
    return [solve(pick(c, 2, i), pick(A, 3, i), pick(b, 2, i), pick(lower, 2, i), pick(upper, 2, i), sense, **kw)
            for i in range(count)]


def hand_model():
    """Min -2 x1 + 0 x2 - 3 x3;  x1 + x2 + x3 <= 10,  x1 + 2 x3 <= 8;  1 <= x1, 0 <= x2 <= 2, 0.5 <= x3 <= 2."""
    c = np.array([-2.0, 0.0, -3.0]); A = np.array([[1.0, 1.0, 1.0], [1.0, 0.0, 2.0]]); b = np.array([10.0, 8.0])
    lower = np.array([1.0, 0.0, 0.5]); upper = np.array([np.inf, 2.0, 2.0])
    return c, A, b, lower, upper
