"""NumPy restatement of lpx_packed_base_solve_costs (include/lpx.h), written from the contract and not from the kernel: the base is
tests/_packed_warm_ref.open_base; step 3 (the cost move) is restated literally, every product and every sum separately rounded in
the stated order; the primal loop is the arithmetic of tests/_bounded_ref.run started from the base's flip bytes; step 5 is the RHS
move of _packed_warm_ref.solve followed by _bounded_long_ref.dual_run3; the extraction is _packed_warm_ref's with the constant
re-summed from c_i.  Test infrastructure: tests/test_gpu_packed_cost.py compares the device against it bit for bit;
tests/test_packed_cost_ref.py pins it to the cold solve of every scenario."""
from collections import namedtuple

import numpy as np

import _bounded_long_ref as L
import _bounded_ref as B
import _packed_dual_ref as P
import _packed_warm_ref as W
from oracle import oracle as O

OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT, EINVAL = P.OPTIMAL, B.UNBOUNDED, P.INFEASIBLE, P.ITER_LIMIT, P.EINVAL
MAX, MIN, LE, GE = P.MAX, P.MIN, P.LE, P.GE
INF = np.inf

CostBase = namedtuple("CostBase", "base c0")            # base: a _packed_warm_ref.Base; c0: the costs it was opened with
# pcounts = (kind-0 pivots, kind-1 pivots, bound flips) of the primal loop; dcounts = (kind 0, kind 1, passes) of the dual loop
Solved = namedtuple("Solved", "status x value primal_events dual_events pcounts dcounts z basis at_upper y d")


def open_base(c, A, b, rel=None, lower=None, upper=None, sense=MAX, long_step=True, max_iter=10000):
    return CostBase(W.open_base(c, A, b, rel, lower, upper, sense, long_step=long_step, max_iter=max_iter),
                    np.asarray(c, dtype=np.float64).copy())


def _refused(m, n):
    return Solved(EINVAL, np.zeros(n), 0.0, 0, 0, (0, 0, 0), (0, 0, 0), 0.0, np.zeros(m, dtype=np.int32), np.zeros(n, dtype=np.uint8),
                  np.zeros(m), np.zeros(n))


def cost_move(base, c0, c):
    """Step 3 on a copy of the base's tile: returns (T, constant, shifted)."""
    m, n = base.m, base.n
    T = base.T.copy()
    C = T.shape[1]
    Cm = C - 1
    delta = c - c0
    if base.is_min:
        delta = -delta
    g = np.zeros(Cm)
    for j in range(n):
        g[j] = -delta[j] if base.flip[j] & 1 else delta[j]
    K = 0.0
    for j in range(n):
        if base.flip[j] & 1 and delta[j] != 0.0:
            prod = delta[j] * base.ub[j]
            K = K + prod
    acc = T[m].copy()                                   # every column j at once, i ascending, zeros skipped
    for i in range(m):
        gi = g[base.basis[i]]
        if gi != 0.0:
            prod = gi * T[i]
            acc = acc + prod
    nz = np.flatnonzero(g[:n] != 0.0)
    acc[nz] = acc[nz] - g[nz]
    acc[Cm] = acc[Cm] + K
    T[m] = acc
    constant, shifted = 0.0, False
    if base.lower is not None:
        for j in range(n):
            if base.lower[j] != 0.0:
                prod = c[j] * base.lower[j]
                constant = constant + prod
                shifted = True
    return T, constant, shifted


def primal_run(T, basis, ub, flip, eps=1e-9, tol=1e-9, max_iter=10000):
    """_bounded_ref.run with an initial flip vector, on copies.  Returns (status, T, basis, flip, events, counts)."""
    T = np.ascontiguousarray(T, dtype=np.float64).copy()
    basis = np.asarray(basis, dtype=np.int32).copy()
    flip = np.asarray(flip, dtype=np.uint8).copy()
    Cm = T.shape[1] - 1
    events, counts = 0, [0, 0, 0]
    while True:
        if events >= max_iter:
            status = ITER_LIMIT
            break
        q = O.choose_entering(T, eps)
        if q < 0:
            status = OPTIMAL
            break
        best, r, kind = B.ratio_scan(T, basis, ub, q, eps, tol)
        uq = ub[q]
        if uq < INF and uq <= best:
            prod = uq * T[:, q]
            T[:, Cm] = T[:, Cm] - prod
            T[:, q] = -T[:, q]
            flip[q] ^= 1
            events += 1; counts[2] += 1
            continue
        if r < 0:
            status = UNBOUNDED
            break
        if kind == 1:
            p = int(basis[r])
            keep = T[r, p]
            T[r, :Cm] = -T[r, :Cm]
            T[r, p] = keep
            T[r, Cm] = ub[p] - T[r, Cm]
            flip[p] ^= 1
            counts[1] += 1
        else:
            counts[0] += 1
        events += 1
        O.pivot(T, r, q)
        basis[r] = q
    return status, T, basis, flip, events, tuple(counts)


def solve(cb, c, b=None, long_step=True, p_max_iter=10000, d_max_iter=10000, p_eps=1e-9, p_tol=1e-9, d_eps=1e-9, d_tol=1e-12):
    """One scenario of lpx_packed_base_solve_costs."""
    base, c0 = cb
    m, n = base.m, base.n
    c = np.asarray(c, dtype=np.float64)
    if b is not None:
        b = np.asarray(b, dtype=np.float64)
    if not np.isfinite(c).all() or (b is not None and not np.isfinite(b).all()):      # step 2
        return _refused(m, n)
    T, constant, shifted = cost_move(base, c0, c)                                      # step 3
    status, T, basis, flip, p_events, pcounts = primal_run(T, base.basis, base.ub, base.flip, p_eps, p_tol, p_max_iter)   # step 4
    d_events, dcounts = 0, (0, 0, 0)
    ge = base.rel == GE
    if b is not None and status == OPTIMAL:                                            # step 5
        delta = b - base.b0
        delta[ge] = -delta[ge]
        Cm = T.shape[1] - 1
        for k in range(m):
            if delta[k] != 0.0:
                prod = T[:, n + k] * delta[k]
                T[:, Cm] = T[:, Cm] + prod
        status, T, basis, flip, trace, dcounts = L.dual_run3(T, basis, base.ub, flip, L.LONG_STEP if long_step else 0, eps=d_eps,
                                                             tol=d_tol, max_iter=d_max_iter)
        d_events = len(trace)
    x, z, at_upper = B.solution(T, basis, flip, base.ub, n)                            # step 6
    x = x.copy()
    if base.lower is not None:
        x = x + base.lower
    value = z
    if shifted or base.is_min:
        value = -z if base.is_min else z
        if shifted:
            value = value + constant
    y = T[m, n:n + m].copy()
    neg = ge != bool(base.is_min)
    y[neg] = -y[neg]
    d = T[m, :n].copy()
    neg = (flip[:n] != 0) == bool(base.is_min)
    d[neg] = -d[neg]
    return Solved(int(status), x, float(value), p_events, d_events, pcounts, tuple(dcounts), float(z), basis, at_upper, y, d)


def solve_all(cb, c, b=None, **kw):
    c = np.atleast_2d(np.asarray(c, dtype=np.float64))
    if b is None:
        return [solve(cb, ci, None, **kw) for ci in c]
    b = np.atleast_2d(np.asarray(b, dtype=np.float64))
    K = max(len(c), len(b))
    c = np.broadcast_to(c, (K, c.shape[1])); b = np.broadcast_to(b, (K, b.shape[1]))
    return [solve(cb, ci, bi.copy(), **kw) for ci, bi in zip(c, b)]


# ---- the scenario sets: the models of _packed_warm_ref.SETS; per set the cost vectors are c0 itself, vectors within +-30 % of c0,
# one vector with a single entry moved (the zero skip), one moved by integers in [-3, 3] (sign changes).  The combined form pairs
# the same vectors with the set's own right-hand sides, cycled ----------------------------------------------------------------
N_SPREAD = 5                                            # rows 1 .. N_SPREAD of a set's costs are the +-30 % vectors

_CACHE = {}


def cost_set(name):
    """((c, A, rel, b0, upper, lower, sense), costs [K][n], rhs [K][m]) of a set, built once."""
    if name not in _CACHE:
        model, bs = W.scenario_set(name)
        c0 = np.asarray(model[0], dtype=np.float64)
        n = len(c0)
        g = np.random.default_rng(1000 + sum(ord(ch) for ch in name))
        spread = c0 * (1.0 + g.uniform(-0.3, 0.3, size=(N_SPREAD, n)))
        single = c0.copy(); single[n // 2] = single[n // 2] + 0.75
        ints = c0 + g.integers(-3, 4, size=n).astype(np.float64)
        cs = np.vstack([c0[None, :], spread, single[None, :], ints[None, :]])
        rhs = np.stack([bs[k % len(bs)] for k in range(len(cs))])
        _CACHE[name] = (model, cs, rhs)
    return _CACHE[name]


def set_base(name, long_step=True):
    key = (name, "base", bool(long_step))
    if key not in _CACHE:
        _CACHE[key] = CostBase(W.set_base(name, long_step), np.asarray(W.scenario_set(name)[0][0], dtype=np.float64).copy())
    return _CACHE[key]


def set_refs(name, long_step=True, with_b=False):
    """The restatement's answers for a set, computed once and shared (nothing writes them)."""
    key = (name, "refs", bool(long_step), bool(with_b))
    if key not in _CACHE:
        _, cs, rhs = cost_set(name)
        _CACHE[key] = solve_all(set_base(name, long_step), cs, rhs if with_b else None, long_step=long_step)
    return _CACHE[key]


def set_cold(name, with_b=False, long_step=True):
    """_packed_dual_ref.solve of every scenario of a set from the slack basis (EINVAL where the dual start refuses the costs)."""
    key = (name, "cold", bool(long_step), bool(with_b))
    if key not in _CACHE:
        (c, A, rel, b0, upper, lower, sense), cs, rhs = cost_set(name)
        _CACHE[key] = [P.solve(ci, A, rhs[k] if with_b else b0, rel, lower, upper, sense, long_step=long_step) for k, ci in enumerate(cs)]
    return _CACHE[key]


# ---- hand models ---------------------------------------------------------------------------------------------------------------
def unbounded_hand():
    """Min x, x >= 3, no upper bound; the scenario c = -1 is UNBOUNDED (c = 1 is the base, c = 2 keeps the vertex)."""
    model = (np.array([1.0]), np.array([[1.0]]), np.array([GE], dtype=np.int32), np.array([3.0]), None, None, MIN)
    return model, np.array([[1.0], [-1.0], [2.0]]), np.array([[3.0], [5.0], [4.0]])


def batch_model():
    """The mixed 12 x 16 model with a 17th column that no <= row holds and that has no upper bound: a scenario that gives it a
    negative cost is UNBOUNDED, whatever its right-hand side."""
    c, A, rel, b, up, lo, sense = L.mixed_model()
    col = np.where(rel == GE, 2.0, 0.0)
    return (np.append(c, 5.0), np.hstack([A, col[:, None]]), rel, b, np.append(up, INF), np.append(lo, 0.0), sense)


def open_model(model, long_step=True):
    c, A, rel, b0, upper, lower, sense = model
    return open_base(c, A, b0, rel, lower, upper, sense, long_step=long_step)
