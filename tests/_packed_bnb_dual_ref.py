"""NumPy restatement of lpx_solve_packed_bnb_dual (include/lpx.h), model by model: the per-model refusals in their order, the root
of lpx_solve_bounded_dual from the pieces tests/_packed_dual_ref.py is made of (prepare_dual, the dualize flips, dual_run3), then the
search and the end of lpx_solve_packed_bnb restated on a tests/_bounded_long_ref.Handle: one path array indexed by depth, the three
budgets, the stop codes.  Written from the contract, not from the kernel.  The same dict is what lpx_solve_bnb_bounded_dual gives
where max_events and max_depth do not bind.  Test infrastructure: tests/test_gpu_packed_bnb_dual.py compares the device against it
bit for bit; tests/test_packed_bnb_dual_ref.py pins it to scipy.optimize.milp, to _packed_dual_ref.solve at the root and to a driver
that carries a path per node."""
import numpy as np

import _bnb_bounded_ref as N
import _bounded_long_ref as L
import _bounded_ref as B

OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT, CUTOFF = 0, 1, 2, 3, 5
EINVAL = -1
DONE, ROOT, NODES, NODE_ITER, EVENTS, DEPTH, REFUSED = range(7)
MAX, MIN = 0, 1
LE, GE, EQ = 0, 1, 2
INF = np.inf
EPS = N.EPS
COUNTERS = ("nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K")


def _record(n, status, stop, constant=0.0, root_events=0, why=""):
    return {"status": status, "stop": stop, "x": np.zeros(n), "value": 0.0, "nodes": 0, "events": 0, "flips": 0, "incumbents": 0,
            "pruned_bound": 0, "pruned_infeasible": 0, "max_K": 0, "deepest": 0, "root_events": root_events, "logged": 0,
            "best": -INF, "constant": constant, "log": np.zeros(0, dtype=N.LOG_DTYPE),
            "why": why, "root_status": None, "root_z": None, "root_flips": 0}      # the last four are not part of the device record


def solve(c, A, b, rel=None, upper=None, lower=None, is_int=None, sense=MAX, search_flags=0, max_iter=10000, max_nodes=100000,
          max_events=2000000, max_depth=0, log_cap=None):
    """One model of a packed call: a dict with status, stop, x, value, every counter of lpx_packed_bnb_record and log (every
    record, or the first log_cap)."""
    assert not search_flags & ~(L.LONG_STEP | L.CUTOFF_FLAG) and max_nodes >= 1 and max_events >= 1 and max_iter >= 0
    c = np.asarray(c, dtype=np.float64); A = np.asarray(A, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    m, n = A.shape
    max_depth = max_depth if max_depth > 0 else n
    lo = None if lower is None else np.broadcast_to(np.asarray(lower, dtype=np.float64), (n,))
    up = np.full(n, INF) if upper is None else np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,))
    rel = np.zeros(m, dtype=np.int32) if rel is None else np.asarray(rel, dtype=np.int32)
    mask = None if is_int is None else np.asarray(is_int, dtype=np.uint8)
    for j in range(n):                                  # the bounds first ...
        l = 0.0 if lo is None else lo[j]
        if not np.isfinite(l) or not (up[j] >= l):
            return _record(n, EINVAL, ROOT, why="bound")
    for j in range(n):                                  # ... then the integer variables: a finite upper bound, integral bounds
        if mask is not None and not mask[j]:
            continue
        l = 0.0 if lo is None else lo[j]
        if not np.isfinite(up[j]) or np.floor(l) != l or np.floor(up[j]) != up[j]:
            return _record(n, EINVAL, ROOT, why="integer")
    if not np.isin(rel, (LE, GE)).all():                # ... then the row senses
        return _record(n, EINVAL, ROOT, why="rel")
    try:                                                # ... then the precheck: an improving column without an upper bound
        T0, basis0, ub, _, is_min, shifted, constant = L.prepare_dual(c, A, rel, b, lo, up, sense)
    except ValueError:
        return _record(n, EINVAL, ROOT, why="precheck")
    T1, flip, root_flips, unrepairable = N.dualize(T0, ub, np.zeros(len(ub), dtype=np.uint8))      # eps 1e-9
    assert unrepairable == 0
    st, Ts, bs, flip, trace, _ = L.dual_run3(T1, basis0, ub, flip, search_flags & L.LONG_STEP, eps=1e-9, tol=1e-12, max_iter=max_iter)
    if st != OPTIMAL:
        out = _record(n, st, ROOT, constant, len(trace))
        out.update(root_status=st, root_z=float(Ts[-1, -1]), root_flips=root_flips)
        if st != INFEASIBLE:                            # the iteration limit: x and value as lpx_solve_packed_dual extracts them
            x = B.solution(Ts, bs, flip, ub, n)[0].copy()
            if lo is not None:
                x = x + lo
            z = Ts[-1, -1]
            value = z
            if shifted or is_min:
                value = -z if is_min else z
                if shifted:
                    value = value + constant
            out.update(x=x, value=float(value))
        return out

    out = _record(n, ITER_LIMIT, DONE, constant, len(trace))
    out.update(root_status=st, root_z=float(Ts[-1, -1]), root_flips=root_flips)
    h = L.Handle(Ts, bs, ub, flip)
    root_ub = ub[:n].copy()
    cur_lo, cur_ub = np.zeros(n), root_ub.copy()
    best, best_x = -INF, None
    stack = [(0, -1, 0.0, 0.0)]                         # (depth, var, lower, upper); the root has no override
    path = [None] * (max_depth + 1)
    log = []
    while True:
        if not stack:
            out["stop"] = DONE
            break
        if out["nodes"] >= max_nodes:                   # the limits first, in this order
            out["stop"] = NODES
            break
        if out["events"] >= max_events:
            out["stop"] = EVENTS
            break
        depth, var, l, u = stack.pop()
        if depth > 0:
            path[depth - 1] = (var, l, u)               # the shallower entries stay valid
        out["nodes"] += 1
        nb_lo, nb_ub = np.zeros(n), root_ub.copy()
        for k in range(depth):
            v, l, u = path[k]
            nb_lo[v], nb_ub[v] = l, u
        cols = np.flatnonzero((nb_lo != cur_lo) | (nb_ub != cur_ub)).astype(np.int32)      # ascending
        cutoff = best + EPS if search_flags & L.CUTOFF_FLAG else -INF
        if any(nb_ub[j] == INF and h.flip[j] for j in cols):
            out["stop"] = REFUSED
            break
        rec = h.node2(cols, nb_lo[cols], nb_ub[cols], n, mask, EPS, L.SKIP_FIXED | search_flags, cutoff, max_iter=max_iter)
        if rec["status"] is None:                       # a column no flip can repair
            out["stop"] = REFUSED
            break
        cur_lo, cur_ub = nb_lo, nb_ub
        K = len(cols)
        out["events"] += rec["events"]; out["flips"] += rec["flips"]
        out["max_K"] = max(out["max_K"], K); out["deepest"] = max(out["deepest"], depth)
        log.append((depth, K, rec["status"], rec["events"], rec["flips"], rec["var"], rec["z"]))
        if rec["status"] == ITER_LIMIT:
            out["stop"] = NODE_ITER
            break
        if rec["status"] == INFEASIBLE:
            out["pruned_infeasible"] += 1
            continue
        z = rec["z"]
        if rec["status"] == CUTOFF or z <= best + EPS:
            out["pruned_bound"] += 1
            continue
        if rec["var"] < 0:
            x = N.values(h.T, h.basis, h.flip, h.ub, h.lo, n).copy()
            ints = np.ones(n, dtype=bool) if mask is None else mask != 0
            x[ints] = np.rint(x[ints])                  # half to even
            best, best_x = z, x
            out["incumbents"] += 1
            continue
        if depth + 1 > max_depth:
            out["stop"] = DEPTH
            break
        v, xv = rec["var"], rec["x_var"]
        stack.append((depth + 1, v, nb_lo[v], np.floor(xv)))
        stack.append((depth + 1, v, np.ceil(xv), nb_ub[v]))                # explored first
        assert len(stack) <= max_depth + 1
    out["log"] = np.array(log if log_cap is None else log[:log_cap], dtype=N.LOG_DTYPE)
    out["logged"] = len(out["log"])
    out["best"] = float(best)
    if out["stop"] == DONE:
        out["status"] = OPTIMAL if best_x is not None else INFEASIBLE
    elif out["stop"] == REFUSED:
        out["status"] = EINVAL
    if best_x is not None:
        x = best_x + lo if lo is not None else best_x
        value = -best if is_min else best
        if shifted:
            value = value + constant
        out.update(x=x, value=float(value))
    return out


def solve_all(c, A, b, rel=None, upper=None, lower=None, is_int=None, sense=MAX, **kw):
    """A packed batch: arrays with or without the batch axis, as LPSolver.SolvePackedBnbDual takes them."""
    c, A, b = (np.asarray(v, dtype=np.float64) for v in (c, A, b))
    n = A.shape[-1]
    rel = None if rel is None else np.asarray(rel, dtype=np.int32)
    lower = None if lower is None else np.asarray(lower, dtype=np.float64)
    upper = None if upper is None else np.asarray(upper, dtype=np.float64)
    sizes = [v.shape[0] for v, nd in ((c, 2), (A, 3), (b, 2), (rel, 2), (lower, 2), (upper, 2)) if v is not None and v.ndim == nd]
    count = sizes[0] if sizes else 1

    def pick(v, nd, i):
        if v is None:
            return None
        if v.ndim == 0:
            return np.full(n, float(v))
        return v[i] if v.ndim == nd else v
    return [solve(pick(c, 2, i), pick(A, 3, i), pick(b, 2, i), pick(rel, 2, i), pick(upper, 2, i), pick(lower, 2, i), is_int, sense, **kw)
            for i in range(count)]


# ---- the instances the CPU and the GPU tests share: (c, A, rel, b, upper, lower, is_int, sense) -------------------------------
def _draw(m, n, seed, signs=False):
    g = np.random.default_rng(seed)
    A = g.integers(1, 9, (m, n)).astype(np.float64)     # A first, then the costs
    c = g.integers(1, 12, n).astype(np.float64)
    if signs:
        c = c * np.where(g.uniform(size=n) < 0.3, -1.0, 1.0)
    return c, A


def cover(m, n, seed, f=0.4, u=1.0):
    """Min c.x, A x >= floor(f rowsum), 0 <= x <= u, every variable integer."""
    c, A = _draw(m, n, seed)
    return c, A, np.full(m, GE, dtype=np.int32), np.floor(f * A.sum(axis=1)), np.full(n, float(u)), None, None, MIN


def mixed_rows(seed):
    """Max c.x with costs of both signs over three <= and three >= rows, binaries."""
    c, A = _draw(6, 10, seed, True)
    rel = np.array([LE, GE] * 3, dtype=np.int32)
    s = A.sum(axis=1)
    b = np.where(rel == GE, np.floor(0.45 * s), np.floor(0.55 * s) + 0.5)
    return c, A, rel, b, np.ones(10), None, None, MAX


def mixed_general(seed):
    """The same A, rel and c, Min: two non-zero lower bounds, ranges of 3, columns 1, 4 and 7 continuous."""
    c, A = _draw(6, 10, seed, True)
    rel = np.array([LE, GE] * 3, dtype=np.int32)
    lower = np.zeros(10); lower[0] = 1.0; lower[3] = 2.0
    is_int = np.ones(10, dtype=np.uint8); is_int[[1, 4, 7]] = 0
    s = A.sum(axis=1)
    b = np.where(rel == GE, np.floor(1.4 * s), np.floor(1.7 * s) + 0.5)
    return c, A, rel, b, lower + 3.0, lower, is_int, MIN


def eq_pair():
    """2 x1 + 2 x2 + 2 x3 = 3 as its pair of rows over binaries: no integer point, found by the search."""
    A = np.array([[2.0, 2.0, 2.0], [2.0, 2.0, 2.0]])
    return np.ones(3), A, np.array([LE, GE], dtype=np.int32), np.array([3.0, 3.0]), np.ones(3), None, None, MAX


def root_infeasible():
    """x1 + x2 >= 3 over binaries: the root LP has no point."""
    return np.ones(2), np.array([[1.0, 1.0]]), np.array([GE], dtype=np.int32), np.array([3.0]), np.ones(2), None, None, MIN


SWEEP_F = (0.2, 0.5, 0.8, 0.95, 1.0, 1.05)


def sweep():
    """cover(5, 9, 5) with b = floor(f rowsum) for f in SWEEP_F: a list of instances sharing c, A and rel."""
    return [cover(5, 9, 5, f) for f in SWEEP_F]


# name -> (instance, the budgets that differ from the defaults)
def _instances():
    out = {}
    for m, n, s in ((4, 8, 1), (6, 12, 1), (8, 16, 3), (10, 24, 1)):
        out["cover %dx%d s%d" % (m, n, s)] = (cover(m, n, s), {})
    for s in (1, 2, 3):
        out["mixed_rows s%d" % s] = (mixed_rows(s), {})
        out["mixed_general s%d" % s] = (mixed_general(s), {})
    out["eq_pair"] = (eq_pair(), {})
    out["root_infeasible"] = (root_infeasible(), {})
    for f, inst in zip(SWEEP_F, sweep()):
        out["sweep f=%g" % f] = (inst, {})
    return out


def _edges():
    out = {}
    for m, n, s in ((1, 1, 1), (1, 3, 1), (2, 64, 1), (3, 65, 1), (65, 5, 1), (3, 65, 2)):
        out["edge %dx%d s%d" % (m, n, s)] = (cover(m, n, s), {})
    # general integers branch on one variable more than once: the tree is 8 deep, deeper than max_depth = 0 (= n = 5) allows
    out["edge 65x5 s2 general"] = (cover(65, 5, 2, 1.2, 3.0), {"max_depth": 64})
    out["edge 9x130 s1"] = (cover(9, 130, 1), {"max_nodes": 200})       # n > 128; it ends NODES by design
    return out


INSTANCES = _instances()
EDGES = _edges()
_CACHE = {}


def ref(name, flags):
    """The restatement's answer for a named instance, computed once and shared (nothing writes it)."""
    key = (name, flags)
    if key not in _CACHE:
        inst, kw = (INSTANCES.get(name) or EDGES[name])
        c, A, rel, b, upper, lower, is_int, sense = inst
        _CACHE[key] = solve(c, A, b, rel, upper, lower, is_int, sense, search_flags=flags, **kw)
    return _CACHE[key]
