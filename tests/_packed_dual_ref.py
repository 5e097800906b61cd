"""NumPy restatement of lpx_solve_packed_dual (include/lpx.h), model by model: the per-model refusals in their order, the
preparation and the loop of lpx_solve_bounded_dual (tests/_bounded_long_ref.py: prepare_dual, the dualize flips, dual_run3), the
extraction of tests/_packed_ref.py and the duals.  Written from the contract, not from the kernel.  Test infrastructure:
tests/test_gpu_packed_dual.py compares the device against it bit for bit; tests/test_packed_dual_ref.py checks it against HiGHS and
checks the duals by what they mean."""
from collections import namedtuple

import numpy as np

import _bnb_bounded_ref as N
import _bounded_long_ref as L
import _bounded_ref as B

OPTIMAL, INFEASIBLE, ITER_LIMIT, EINVAL = L.OPTIMAL, L.INFEASIBLE, L.ITER_LIMIT, -1
MAX, MIN = 0, 1
LE, GE = 0, 1

# counts = (kind-0 pivots, kind-1 pivots, passes); why: "" or which check refused the model ("bound", "rel", "precheck")
Solved = namedtuple("Solved", "status x value events counts dualize_flips z basis at_upper y d why")


def _refused(m, n, why):
    return Solved(EINVAL, np.zeros(n), 0.0, 0, (0, 0, 0), 0, 0.0, np.zeros(m, dtype=np.int32), np.zeros(n, dtype=np.uint8),
                  np.zeros(m), np.zeros(n), why)


def solve(c, A, b, rel=None, lower=None, upper=None, sense=MAX, long_step=True, max_iter=10000, eps=1e-9, tol=1e-12):
    """One model of a packed dual call: what status[i], x, value, rec, basis, at_upper, y and d hold."""
    c = np.asarray(c, dtype=np.float64); A = np.asarray(A, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    m, n = A.shape
    lo = None if lower is None else np.broadcast_to(np.asarray(lower, dtype=np.float64), (n,))      # a scalar: every variable
    up = np.full(n, np.inf) if upper is None else np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,))
    rel = np.zeros(m, dtype=np.int32) if rel is None else np.asarray(rel, dtype=np.int32)
    for j in range(n):                                  # the bounds first
        l = 0.0 if lo is None else lo[j]
        if not np.isfinite(l) or not (up[j] >= l):
            return _refused(m, n, "bound")
    if not np.isin(rel, (LE, GE)).all():                # then the row senses
        return _refused(m, n, "rel")
    try:                                                # then the precheck: an improving column without an upper bound
        T0, basis0, ub, _, is_min, shifted, constant = L.prepare_dual(c, A, rel, b, lo, up, sense)
    except ValueError:
        return _refused(m, n, "precheck")
    T1, flip, flips, unrepairable = N.dualize(T0, ub, np.zeros(len(ub), dtype=np.uint8))            # eps 1e-9, whatever the loop's is
    assert unrepairable == 0
    status, T, basis, flip, trace, counts = L.dual_run3(T1, basis0, ub, flip, L.LONG_STEP if long_step else 0, eps=eps, tol=tol,
                                                         max_iter=max_iter)
    x, z, at_upper = B.solution(T, basis, flip, ub, n)
    x = x.copy()
    if lo is not None:                                  # every j, a zero lower bound too: -0.0 becomes +0.0
        x = x + lo
    value = z
    if shifted or is_min:
        value = -z if is_min else z
        if shifted:
            value = value + constant
    # the duals: objective-row bits with exact sign changes
    y = T[m, n:n + m].copy()
    neg = (rel == GE) != bool(is_min)                   # exactly one of (row i was >=, the sense is Min)
    y[neg] = -y[neg]
    d = T[m, :n].copy()
    neg = (flip[:n] != 0) == bool(is_min)
    d[neg] = -d[neg]
    return Solved(status, x, float(value), len(trace), counts, flips, float(z), basis, at_upper, y, d, "")


def solve_all(c, A, b, rel=None, lower=None, upper=None, sense=MAX, **kw):
    """A packed batch: arrays with or without the batch axis, as LPSolver.SolvePackedDual takes them."""
    c, A, b = (np.asarray(v, dtype=np.float64) for v in (c, A, b))
    rel = None if rel is None else np.asarray(rel, dtype=np.int32)
    lower = None if lower is None else np.asarray(lower, dtype=np.float64)
    upper = None if upper is None else np.asarray(upper, dtype=np.float64)
    sizes = [v.shape[0] for v, nd in ((c, 2), (A, 3), (b, 2), (rel, 2), (lower, 2), (upper, 2)) if v is not None and v.ndim == nd]
    count = sizes[0] if sizes else 1

    def pick(v, nd, i):
        return None if v is None else (v[i] if v.ndim == nd else v)
    return [solve(pick(c, 2, i), pick(A, 3, i), pick(b, 2, i), pick(rel, 2, i), pick(lower, 2, i), pick(upper, 2, i), sense, **kw)
            for i in range(count)]


# ---- the instances the CPU and the GPU tests share ---------------------------------------------------------------------
def hand_model():
    """Min 2 x1 + 3 x2 + x3;  x1 + x2 + x3 >= 4,  x1 - x2 + 2 x3 <= 3;  0 <= x <= (3, 3, 2): (c, A, rel, b, upper)."""
    c = np.array([2.0, 3.0, 1.0]); A = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, 2.0]]); b = np.array([4.0, 3.0])
    return c, A, np.array([GE, LE], dtype=np.int32), b, np.array([3.0, 3.0, 2.0])


def max_le_model(seed):
    """binary_bounded(12, 6, seed) as a user model: Max c.x, A x <= b, 0 <= x <= 1 -- every column needs a dualize flip."""
    c, A, b = B.binary_bounded(12, 6, seed)[3]
    return c, A, np.zeros(6, dtype=np.int32), b, np.ones(12)


def wide_model(seed):
    """4 x 1100, unit bounds, costs of both signs, rows of both senses, Max: Cm = 1104 > 1024, so the count and the flip list of
    the kernel take a second trip.  (c, A, rel, b, upper)."""
    g = np.random.default_rng(seed)
    A = g.integers(1, 9, size=(4, 1100)).astype(np.float64)
    c = g.integers(1, 12, size=1100).astype(np.float64) * np.where(g.uniform(size=1100) < 0.5, -1.0, 1.0)
    rel = np.array([LE, GE, LE, GE], dtype=np.int32)
    b = np.floor(A.sum(axis=1) * np.where(rel == GE, 0.45, 0.4)) + 0.5
    return c, A, rel, b, np.ones(1100)


def tall_model(m, n, seed):
    """m rows over n columns, Min with positive costs, rows alternating >= and <=, 0 <= x <= 3: (c, A, rel, b, upper)."""
    g = np.random.default_rng(seed)
    A = g.integers(1, 9, size=(m, n)).astype(np.float64)
    c = g.integers(1, 12, size=n).astype(np.float64)
    rel = (np.arange(m) % 2 == 0).astype(np.int32)
    b = np.where(rel == GE, np.floor(0.5 * A.sum(axis=1)), np.floor(2.5 * A.sum(axis=1)) + 0.5)
    return c, A, rel, b, np.full(n, 3.0)


def _one_by_one():
    """1 x 1 in both row senses and both cost signs, 2 x <> 3 with x <= 4, and 2 x >= 9, which no x <= 4 satisfies."""
    return [(np.array([cc]), np.array([[2.0]]), np.array([r], dtype=np.int32), np.array([bb]))
            for cc, r, bb in ((1.0, LE, 3.0), (-1.0, GE, 3.0), (1.0, GE, 3.0), (-1.0, LE, 3.0), (1.0, GE, 9.0))]


def _hand_variants():
    c, A, rel, b, _ = hand_model()
    return [(c, A, rel, b + np.array(d)) for d in ((0.0, 0.0), (1.0, 0.0), (-1.0, 1.0))]


def _mixed_variants():
    c, A, rel, b = L.mixed_model()[:4]
    return [(c, A, rel, b), (c, A, rel, b + 1.0), (-c, A, 1 - rel, b)]


def _covering(m, n, seeds, infeasible=False):
    out = [L.covering_model(m, n, s) for s in seeds]
    if infeasible:                                      # more than every variable at its upper bound can cover
        c, A, rel, b = out[0]
        out.append((c, A, rel, 1.5 * A.sum(axis=1)))
    return out


# name -> (the models (c, A, rel, b) of one batch, upper, lower, sense)
SHAPES = {
    "1x1 max": (_one_by_one, np.array([4.0]), None, MAX),
    "1x1 min": (_one_by_one, np.array([4.0]), None, MIN),
    "hand 2x3": (_hand_variants, hand_model()[4], None, MIN),
    "mixed 12x16": (_mixed_variants, L.mixed_model()[4], L.mixed_model()[5], MIN),      # dualize flips, a non-zero lower bound
    "covering 6x12": (lambda: _covering(6, 12, (1, 2, 3), True), 1.0, None, MIN),
    "covering 12x60": (lambda: _covering(12, 60, (1, 2, 3)), 1.0, None, MIN),
    "65x20": (lambda: [tall_model(65, 20, s)[:4] for s in (1, 2)], 3.0, None, MIN),       # more rows than one wave
    "139x1": (lambda: [tall_model(139, 1, s)[:4] for s in (1, 2)], 3.0, None, MIN),       # the last m that fits
    "4x1100": (lambda: [wide_model(s)[:4] for s in (1, 2)], 1.0, None, MAX),              # Cm = 1104 > 1024 lanes
}

_CACHE = {}


def shape(name):
    """The stacked arrays of a shape: (c, A, rel, b, upper, lower, sense)."""
    if name not in _CACHE:
        build, upper, lower, sense = SHAPES[name]
        models = build()
        c, A, rel, b = (np.stack([mdl[k] for mdl in models]) for k in range(4))
        _CACHE[name] = (c, A, rel, b, upper, lower, sense)
    return _CACHE[name]


def shape_refs(name, long_step):
    """The restatement's answers for a shape, computed once and shared (nothing writes them)."""
    key = (name, bool(long_step))
    if key not in _CACHE:
        c, A, rel, b, upper, lower, sense = shape(name)
        _CACHE[key] = solve_all(c, A, b, rel, lower, upper, sense, long_step=long_step)
    return _CACHE[key]
