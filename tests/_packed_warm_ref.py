"""NumPy restatement of lpx_packed_base_open / lpx_packed_base_solve (include/lpx.h), written from the contract and not from the
kernel: the base is lpx_solve_bounded_dual (tests/_bounded_long_ref.py: solve_bounded_dual); a scenario moves the RHS column of
the base's solved tableau by the slack block times delta (step 3, literally: k ascending over the non-zero delta_k, one multiply
and one add each), continues with dual_run3 from the base's basis and flip bytes, and is extracted as tests/_packed_dual_ref.py
extracts a model.  Test infrastructure: tests/test_gpu_packed_warm.py compares the device against it bit for bit;
tests/test_packed_warm_ref.py pins it to the cold solve of every scenario (_packed_dual_ref.solve)."""
from collections import namedtuple

import numpy as np

import _bounded_long_ref as L
import _bounded_ref as B
import _packed_dual_ref as P

OPTIMAL, INFEASIBLE, ITER_LIMIT, EINVAL = P.OPTIMAL, P.INFEASIBLE, P.ITER_LIMIT, P.EINVAL
MAX, MIN, LE, GE = P.MAX, P.MIN, P.LE, P.GE

# cold: what base_out holds (_packed_dual_ref.Solved); T, basis, flip, ub: the solved tableau as the loop left it
Base = namedtuple("Base", "cold T basis flip ub b0 rel lower is_min shifted constant m n")


def open_base(c, A, b, rel=None, lower=None, upper=None, sense=MAX, long_step=True, max_iter=10000):
    """lpx_packed_base_open: the base solved by lpx_solve_bounded_dual.  Returns a Base; raises ValueError unless it is OPTIMAL."""
    c = np.asarray(c, dtype=np.float64); A = np.asarray(A, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    m, n = A.shape
    rel = np.zeros(m, dtype=np.int32) if rel is None else np.asarray(rel, dtype=np.int32)
    lo = None if lower is None else np.broadcast_to(np.asarray(lower, dtype=np.float64), (n,)).copy()
    up = np.full(n, np.inf) if upper is None else np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,))
    cold = P.solve(c, A, b, rel, lo, up, sense, long_step=long_step, max_iter=max_iter)
    if cold.status != OPTIMAL:
        raise ValueError("the base ends with status %d" % cold.status)
    s = L.solve_bounded_dual(c, A, rel, b, up, lo, sense, flags=L.LONG_STEP if long_step else 0, max_iter=max_iter)
    assert s["status"] == OPTIMAL and np.array_equal(s["basis"], cold.basis)
    shifted = lo is not None and bool(np.any(lo != 0.0))
    return Base(cold, s["T"], s["basis"], s["flip"], s["ub"], b.copy(), rel, lo, sense == MIN, shifted, s["constant"], m, n)


def solve(base, b, long_step=True, max_iter=10000, eps=1e-9, tol=1e-12):
    """One scenario of lpx_packed_base_solve: a _packed_dual_ref.Solved with dualize_flips = 0 and this loop's events."""
    m, n = base.m, base.n
    b = np.asarray(b, dtype=np.float64)
    if not np.isfinite(b).all():                        # step 2: refused, every output zeroed
        return P._refused(m, n, "rhs")
    delta = b - base.b0
    ge = base.rel == GE
    delta[ge] = -delta[ge]
    T = base.T.copy()
    Cm = T.shape[1] - 1
    for k in range(m):                                  # step 3: every row r = 0 .. m at once, k ascending, zeros skipped
        if delta[k] != 0.0:
            prod = T[:, n + k] * delta[k]
            T[:, Cm] = T[:, Cm] + prod
    status, T, basis, flip, trace, counts = L.dual_run3(T, base.basis, base.ub, base.flip, L.LONG_STEP if long_step else 0, eps=eps,
                                                         tol=tol, max_iter=max_iter)
    x, z, at_upper = B.solution(T, basis, flip, base.ub, n)
    x = x.copy()
    if base.lower is not None:
        x = x + base.lower
    value = z
    if base.shifted or base.is_min:
        value = -z if base.is_min else z
        if base.shifted:
            value = value + base.constant
    y = T[m, n:n + m].copy()
    neg = ge != bool(base.is_min)
    y[neg] = -y[neg]
    d = T[m, :n].copy()
    neg = (flip[:n] != 0) == bool(base.is_min)
    d[neg] = -d[neg]
    return P.Solved(status, x, float(value), len(trace), counts, 0, float(z), basis, at_upper, y, d, "")


def solve_all(base, b, **kw):
    return [solve(base, bi, **kw) for bi in np.atleast_2d(np.asarray(b, dtype=np.float64))]


# ---- the instances the CPU and the GPU tests share: name -> (c, A, rel, b0, upper, lower, sense) and the scenarios [K][m] -------
def _spread(b0, K, seed, first_is_base=True):
    """K right-hand sides within +-20 % of b0; the first one is b0 itself."""
    g = np.random.default_rng(seed)
    out = b0 * (1.0 + g.uniform(-0.2, 0.2, size=(K, len(b0))))
    if first_is_base:
        out[0] = b0
    return out


def _one_by_one(sense):
    """2 x >= 3, x <= 4; b in {3, 5, -1, 9}: the base, a move inside the bound, a row that stops binding, no x <= 4 can do it."""
    return (np.array([1.0]), np.array([[2.0]]), np.array([GE], dtype=np.int32), np.array([3.0]), np.array([4.0]), None, sense), \
        np.array([[3.0], [5.0], [-1.0], [9.0]])


def _hand():
    c, A, rel, b, up = P.hand_model()
    moves = np.array([[0.0, 0.0], [3.0, 0.0], [0.0, -4.0], [-2.0, 2.0], [2.0, -3.0]])       # delta in one row only: the zero skip
    return (c, A, rel, b, up, None, MIN), b + moves


def _mixed():
    c, A, rel, b, up, lo, sense = L.mixed_model()
    g = np.random.default_rng(5)
    moves = g.integers(-25, 25, size=(10, 12)).astype(np.float64)
    moves[0] = 0.0
    return (c, A, rel, b, up, lo, sense), b + moves


def _max_le():
    c, A, rel, b, up = P.max_le_model(2)
    return (c, A, rel, b, up, None, MAX), _spread(b, 6, 21)


def _tall(m, n, K):
    def build():
        c, A, rel, b, up = P.tall_model(m, n, 1)
        return (c, A, rel, b, up, None, MIN), _spread(b, K, 100 + m)
    return build


def _wide():
    c, A, rel, b, up = P.wide_model(1)
    return (c, A, rel, b, up, None, MAX), _spread(b, 3, 31)


def _covering(m, n, K):
    def build():
        c, A, rel, b = L.covering_model(m, n, 1)
        return (c, A, rel, b, np.ones(n), None, MIN), _spread(b, K, 41)
    return build


SETS = {
    "1x1 max": lambda: _one_by_one(MAX),
    "1x1 min": lambda: _one_by_one(MIN),
    "hand 2x3": _hand,
    "mixed 12x16": _mixed,                              # a non-zero lower bound, dualize flips in the base, rows of both senses, Min
    "max, <= rows": _max_le,                            # Max, every column flipped in the base
    "63x8": _tall(63, 8, 4), "64x8": _tall(64, 8, 4), "65x8": _tall(65, 8, 4),       # R = 64, 65, 66: either side of a wave
    "139x1": _tall(139, 1, 4),                          # the last m that fits; the objective row in the third wave
    "4x1100": _wide,                                    # Cm = 1104 > 1024 lanes: the ub and flip copies take a second trip
    "covering 6x12": _covering(6, 12, 8),
    "covering 12x60": _covering(12, 60, 8),
}

_CACHE = {}


def scenario_set(name):
    """((c, A, rel, b0, upper, lower, sense), scenarios [K][m]) of a set, built once."""
    if name not in _CACHE:
        _CACHE[name] = SETS[name]()
    return _CACHE[name]


def set_base(name, long_step):
    key = (name, "base", bool(long_step))
    if key not in _CACHE:
        (c, A, rel, b0, upper, lower, sense), _ = scenario_set(name)
        _CACHE[key] = open_base(c, A, b0, rel, lower, upper, sense, long_step=long_step)
    return _CACHE[key]


def set_refs(name, long_step):
    """The restatement's answers for a set, computed once and shared (nothing writes them)."""
    key = (name, "refs", bool(long_step))
    if key not in _CACHE:
        _CACHE[key] = solve_all(set_base(name, long_step), scenario_set(name)[1], long_step=long_step)
    return _CACHE[key]


def set_cold(name, long_step):
    """_packed_dual_ref.solve of every scenario of a set from the slack basis."""
    key = (name, "cold", bool(long_step))
    if key not in _CACHE:
        (c, A, rel, b0, upper, lower, sense), bs = scenario_set(name)
        _CACHE[key] = [P.solve(c, A, bi, rel, lower, upper, sense, long_step=long_step) for bi in bs]
    return _CACHE[key]
