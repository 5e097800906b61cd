"""NumPy restatement of lpx_solve_packed_bnb (include/lpx.h), model by model: the preparation and the root of tests/_packed_ref.py,
then the search of lpx_solve_bnb_bounded3 on a tests/_bounded_long_ref.Handle with the three budgets and the stop codes of the
packed call.  Written from the contract, not from the kernel -- but it keeps the search's books the way the contract says the
kernel may: a stack entry is (depth, var, lower, upper) and ONE path array indexed by depth serves every entry, so checking it
against _bounded_long_ref.solve2 (a path per node) also checks that claim.  Test infrastructure: tests/test_gpu_packed_bnb.py
compares the device against it bit for bit; tests/test_packed_bnb_ref.py pins it to solve2 and to scipy.optimize.milp."""
import numpy as np

import _bnb_bounded_ref as N
import _bounded_long_ref as L
import _bounded_ref as B
import _packed_ref as PK

OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT, CUTOFF = 0, 1, 2, 3, 5
EINVAL, E_NEG_RHS = PK.EINVAL, PK.E_NEG_RHS
DONE, ROOT, NODES, NODE_ITER, EVENTS, DEPTH, REFUSED = range(7)
INF = np.inf
EPS = N.EPS
COUNTERS = ("nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K")


def _record(n, status, stop, constant=0.0, root_events=0):
    return {"status": status, "stop": stop, "x": np.zeros(n), "value": 0.0, "nodes": 0, "events": 0, "flips": 0, "incumbents": 0,
            "pruned_bound": 0, "pruned_infeasible": 0, "max_K": 0, "deepest": 0, "root_events": root_events, "logged": 0,
            "best": -INF, "constant": constant, "log": np.zeros(0, dtype=N.LOG_DTYPE)}


def solve(c, A, b, upper, lower=None, is_int=None, sense=PK.MAX, search_flags=0, max_iter=10000, max_nodes=100000,
          max_events=2000000, max_depth=0, log_cap=None):
    """One model of a packed call: a dict with status, stop, x, value, every counter of lpx_packed_bnb_record and log (every
    record, or the first log_cap)."""
    assert not search_flags & ~(L.LONG_STEP | L.CUTOFF_FLAG) and max_nodes >= 1 and max_events >= 1 and max_iter >= 0
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    max_depth = max_depth if max_depth > 0 else n
    lo = None if lower is None else np.broadcast_to(np.asarray(lower, dtype=np.float64), (n,))
    up = None if upper is None else np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,))
    mask = None if is_int is None else np.asarray(is_int, dtype=np.uint8)
    P = PK.prepare(c, A, b, lo, up, sense)
    if P.status == EINVAL:                              # the bounds first ...
        return _record(n, EINVAL, ROOT)
    for j in range(n):                                  # ... then the integer variables: a finite upper bound, integral bounds
        if mask is not None and not mask[j]:
            continue
        l = 0.0 if lo is None else lo[j]
        u = INF if up is None else up[j]
        if not np.isfinite(u) or np.floor(l) != l or np.floor(u) != u:
            return _record(n, EINVAL, ROOT)
    if P.status != 0:                                   # ... then the sign of the shifted right-hand sides
        return _record(n, P.status, ROOT)

    st, Ts, bs, flip, trace, _ = B.run(P.T, P.basis, P.ub, eps=1e-9, tol=1e-9, max_iter=max_iter)
    if st != OPTIMAL:                                   # the root's status, x and value as lpx_solve_packed gives them
        out = _record(n, st, ROOT, P.constant, len(trace))
        x = B.solution(Ts, bs, flip, P.ub, n)[0].copy()
        if lo is not None:
            x = x + lo
        z = Ts[-1, -1]
        value = z
        if P.shifted or sense == PK.MIN:
            value = -z if sense == PK.MIN else z
            if P.shifted:
                value = value + P.constant
        out.update(x=x, value=float(value))
        return out

    out = _record(n, ITER_LIMIT, DONE, P.constant, len(trace))
    h = L.Handle(Ts, bs, P.ub, flip)
    root_ub = P.ub[:n].copy()
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
        value = -best if sense == PK.MIN else best
        if P.shifted:
            value = value + P.constant
        out.update(x=x, value=float(value))
    return out


def solve_all(c, A, b, upper, lower=None, is_int=None, sense=PK.MAX, **kw):
    """A packed batch: arrays with or without the batch axis, as LPSolver.SolvePackedBnb takes them."""
    c, A, b = (np.asarray(v, dtype=np.float64) for v in (c, A, b))
    n = A.shape[-1]
    lower = None if lower is None else np.asarray(lower, dtype=np.float64)
    upper = None if upper is None else np.asarray(upper, dtype=np.float64)
    sizes = [v.shape[0] for v, nd in ((c, 2), (A, 3), (b, 2), (lower, 2), (upper, 2)) if v is not None and v.ndim == nd]
    count = sizes[0] if sizes else 1

    def pick(v, nd, i):
        if v is None:
            return None
        if v.ndim == 0:
            return np.full(n, float(v))
        return v[i] if v.ndim == nd else v
    return [solve(pick(c, 2, i), pick(A, 3, i), pick(b, 2, i), pick(upper, 2, i), pick(lower, 2, i), is_int, sense, **kw)
            for i in range(count)]


# ---- the instances the CPU and the GPU tests share ---------------------------------------------------------------------
BINARY = ((8, 3, 1), (10, 4, 2), (12, 4, 3), (16, 6, 4), (20, 8, 5), (24, 6, 6))


def binary(n, m, seed):
    """binary_model(n, m, seed) as the arguments of solve: (c, A, b, upper)."""
    c, A0, b0 = N.binary_model(n, m, seed)
    return c, A0, b0, np.ones(n)


def small(name):
    """small_models()[name] with every row <=: (c, A, b, upper, lower, is_int, sense).  The = row of "infeasible" becomes its pair
    of <= rows, whose second right-hand side is negative: a packed call refuses it with LPX_E_NEG_RHS, as lpx_solve_packed does."""
    c, A, rel, b, upper, lower, is_int, sense = N.small_models()[name]
    rows, rhs = [], []
    for i, r in enumerate(rel):
        rows.append(A[i]); rhs.append(b[i])
        if r == 2:
            rows.append(A[i] * -1.0); rhs.append(b[i] * -1.0)
    return c, np.array(rows), np.array(rhs), upper, lower, is_int, sense
