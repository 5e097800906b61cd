"""NumPy restatement of the flagged bounded dual loop (lpx_bounded_dual_run3: long-step ratio test, objective cutoff), of
lpx_bounded_node2, of the flagged driver lpx_solve_bnb_bounded2 and of the dual start lpx_solve_bounded_dual, written from the
arithmetic contract in include/lpx.h ("long-step ratio test, objective cutoff and dual start"), not from the kernels.  Test
infrastructure: the GPU tests compare the device against it bit for bit.  The bound change, the dualize flips, the pick, the
preparation and the ordinary pivot are those of _bounded_dual_ref / _bnb_bounded_ref / the oracle, imported unchanged;
everything new is spelled out here with separately rounded IEEE double operations."""
import numpy as np

import _bnb_bounded_ref as N
import _bounded_dual_ref as D
import _bounded_ref as B
from oracle import oracle as O

OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT, CUTOFF = 0, 1, 2, 3, 5
INF = np.inf
SKIP_FIXED, LONG_STEP, CUTOFF_FLAG = 1, 2, 4
EPS = N.EPS
FLAG_SETS = (0, LONG_STEP, CUTOFF_FLAG, LONG_STEP | CUTOFF_FLAG)


def dual_run3(T, basis, ub=None, flip=None, flags=0, cutoff=-INF, eps=1e-9, tol=1e-12, max_iter=10000):
    """lpx_bounded_dual_run3 on copies.  Returns (status, T, basis, flip, trace[k,2], counts(kind 0, kind 1, passes)); a pass is
    the trace entry (-1, q)."""
    assert not flags & ~(SKIP_FIXED | LONG_STEP | CUTOFF_FLAG) and cutoff == cutoff
    T = np.ascontiguousarray(T, dtype=np.float64).copy()
    basis = np.asarray(basis, dtype=np.int32).copy()
    m, Cm = T.shape[0] - 1, T.shape[1] - 1
    ub = np.full(Cm, INF) if ub is None else np.asarray(ub, dtype=np.float64)
    flip = np.zeros(Cm, dtype=np.uint8) if flip is None else np.asarray(flip, dtype=np.uint8).copy()
    open_col = ub > 0.0
    trace, counts = [], [0, 0, 0]
    while True:
        if len(trace) >= max_iter:                         # step 1: passes and pivots alike
            status = ITER_LIMIT
            break
        if flags & CUTOFF_FLAG and T[m, Cm] <= cutoff:     # step 1b
            status = CUTOFF
            break
        b = T[:m, Cm]
        u = ub[basis[:m]]
        w = np.full(m, INF)
        k0 = b < -eps
        k1 = ~k0 & (u < INF)
        w[k0] = b[k0]
        w[k1] = u[k1] - b[k1]
        r = int(np.argmin(w))                              # first index of the strict minimum
        if not w[r] < -eps:
            status = OPTIMAL
            break
        kind = 0 if k0[r] else 1
        p = int(basis[r])
        if kind == 1:                                      # step 3: the complement, in front of every pass
            keep = T[r, p]
            T[r, :Cm] = -T[r, :Cm]
            T[r, p] = keep
            T[r, Cm] = ub[p] - T[r, Cm]
            flip[p] ^= 1
        a = T[r, :Cm]
        part = a < -eps
        if flags & SKIP_FIXED:
            part = part & open_col
        rho = np.full(Cm, INF)
        with np.errstate(all="ignore"):
            rho[part] = T[m, :Cm][part] / (-a[part])      # formed once
        while True:
            q = D._hysteresis(rho, tol)
            if q < 0 or not flags & LONG_STEP or not ub[q] < INF:
                break
            prod = ub[q] * T[r, q]                         # one multiply ...
            nb = T[r, Cm] - prod                           # ... one subtract
            if not nb < -eps:
                break
            prod = ub[q] * T[:, q]                         # the pass: the BOUND FLIP of lpx_bounded_run on column q
            T[:, Cm] = T[:, Cm] - prod
            T[:, q] = -T[:, q]
            flip[q] ^= 1
            trace.append((-1, q)); counts[2] += 1
            rho[q] = INF
        if q < 0:
            status = INFEASIBLE
            break
        trace.append((-2 - r if kind else r, q))
        counts[kind] += 1
        O.pivot(T, r, q)
        basis[r] = q
    return status, T, basis, flip, np.asarray(trace, dtype=np.int32).reshape(-1, 2), tuple(counts)


def least_reduced_cost(T, basis, ub):
    """The least T[m,j] over the nonbasic columns with ub[j] > 0 (+inf when there is none)."""
    m, Cm = T.shape[0] - 1, T.shape[1] - 1
    nonbasic = np.ones(Cm, dtype=bool)
    nonbasic[basis[:m]] = False
    d = T[m, :Cm][nonbasic & (np.asarray(ub) > 0.0)]
    return float(d.min()) if d.size else INF


class Handle(N.Handle):
    """The state a device handle carries between lpx_bounded_node2 calls."""

    def node2(self, cols, lower, upper, nint, is_int=None, tol=EPS, flags=SKIP_FIXED, cutoff=-INF, eps=1e-9, ratio_tol=1e-12,
              max_iter=10000):
        """lpx_bounded_node2: lpx_bounded_node with the loop's flags and cutoff.  A cut-off node has no pick."""
        T, ub, lo = D.change_bounds(self.T, self.ub, self.lo, self.flip, cols, lower, upper)
        T, flip, flips, bad = N.dualize(T, ub, self.flip, eps)
        rec = {"status": None, "events": 0, "kind0": 0, "kind1": 0, "flips": flips, "unrepairable": bad,
               "var": -1, "candidates": 0, "x_var": 0.0, "z": 0.0}
        if bad:
            rec["flips"] = 0
            return rec
        st, T, basis, flip, tr, counts = dual_run3(T, self.basis, ub, flip, flags, cutoff, eps, ratio_tol, max_iter)
        self.T, self.basis, self.ub, self.lo, self.flip, self.trace = T, basis, ub, lo, flip, tr
        rec.update(status=st, events=len(tr), kind0=counts[0], kind1=counts[1], z=float(T[-1, -1]))
        if st == OPTIMAL:
            rec.update(N.pick(T, basis, flip, ub, lo, nint, is_int, tol))
            if flags & LONG_STEP:               # not part of the device record: what the tests assert after every such node
                rec["least_rc"] = least_reduced_cost(T, basis, ub)
        return rec


def solve2(c, A, b, upper, lower=None, is_int=None, sense=0, max_nodes=0, max_iter=10000, rel=None, search_flags=0):
    """lpx_solve_bnb_bounded2: the driver of _bnb_bounded_ref.solve with every node an lpx_bounded_node2 call carrying
    LPX_BDUAL_SKIP_FIXED | search_flags and, with CUTOFF, cutoff = best + 1e-6.  Same dict, plus pivots and passes."""
    assert not search_flags & ~(LONG_STEP | CUTOFF_FLAG)
    T0, basis0, ub0, lower, is_min, shifted, constant = N.prepare(c, A, b, lower, upper, sense, rel)
    n = len(c)
    mask = None if is_int is None else np.asarray(is_int, dtype=np.uint8)
    st, Ts, bs, flip, _, _ = B.run(T0, basis0, ub0, max_iter=max_iter)
    out = {"rc": 0, "status": st, "x": None, "value": 0.0, "nodes": 0, "events": 0, "flips": 0, "incumbents": 0,
           "pruned_bound": 0, "pruned_infeasible": 0, "max_K": 0, "constant": constant, "pivots": 0, "passes": 0,
           "least_rc": INF, "long_optimal_nodes": 0,
           "log": np.zeros(0, dtype=N.LOG_DTYPE)}
    if st != OPTIMAL:
        return out
    h = Handle(Ts, bs, ub0, flip)
    root_lo, root_ub = np.zeros(n), ub0[:n].copy()
    cur_lo, cur_ub = root_lo.copy(), root_ub.copy()
    best, best_x = -INF, None
    stack = [(0, [])]
    log = []
    while stack:
        if max_nodes > 0 and out["nodes"] >= max_nodes:
            out["rc"] = ITER_LIMIT
            break
        depth, path = stack.pop()
        out["nodes"] += 1
        nb_lo, nb_ub = root_lo.copy(), root_ub.copy()
        for var, l, u in path:
            nb_lo[var], nb_ub[var] = l, u
        cols = np.flatnonzero((nb_lo != cur_lo) | (nb_ub != cur_ub)).astype(np.int32)      # ascending
        cutoff = best + EPS if search_flags & CUTOFF_FLAG else -INF                        # the driver's own addition
        rec = h.node2(cols, nb_lo[cols], nb_ub[cols], n, mask, EPS, SKIP_FIXED | search_flags, cutoff, max_iter=max_iter)
        assert rec["status"] is not None, "unrepairable column"
        cur_lo, cur_ub = nb_lo, nb_ub
        K = len(cols)
        out["events"] += rec["events"]; out["flips"] += rec["flips"]; out["max_K"] = max(out["max_K"], K)
        out["pivots"] += rec["kind0"] + rec["kind1"]; out["passes"] += rec["events"] - rec["kind0"] - rec["kind1"]
        if "least_rc" in rec:                    # the least reduced cost any OPTIMAL long-step node left on a movable nonbasic column
            out["least_rc"] = min(out["least_rc"], rec["least_rc"]); out["long_optimal_nodes"] += 1
        log.append((depth, K, rec["status"], rec["events"], rec["flips"], rec["var"], rec["z"]))
        if rec["status"] == ITER_LIMIT:
            out["rc"] = ITER_LIMIT
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
            x[ints] = np.rint(x[ints])           # Math.Round: half to even
            best, best_x = z, x
            out["incumbents"] += 1
            continue
        v, xv = rec["var"], rec["x_var"]
        stack.append((depth + 1, path + [(v, nb_lo[v], np.floor(xv))]))
        stack.append((depth + 1, path + [(v, np.ceil(xv), nb_ub[v])]))     # explored first
    out["log"] = np.array(log, dtype=N.LOG_DTYPE)
    if best_x is None:
        out["status"] = INFEASIBLE
        return out
    x = best_x + lower if np.any(lower != 0.0) else best_x
    value = -best if is_min else best
    if shifted:
        value = value + constant
    out.update(status=OPTIMAL, x=x, value=float(value))
    return out


def prepare_dual(c, A, rel, b, lower, upper, sense=0):
    """The preparation of lpx_solve_bounded_dual: a >= row negated into a <= row (exact), then _bnb_bounded_ref.prepare, which
    accepts a negative shifted RHS.  Returns prepare's tuple; raises ValueError naming the first variable whose internal
    objective-row entry is below -1e-9 while its upper bound is +inf."""
    A = np.array(A, dtype=np.float64); b = np.array(b, dtype=np.float64); rel = np.array(rel, dtype=np.int32)
    ge = rel == 1
    A[ge] = -A[ge]
    b[ge] = -b[ge]
    rel[ge] = 0
    out = N.prepare(c, A, b, lower, upper, sense, rel)
    T, ub = out[0], out[2]
    for j in range(len(c)):
        if T[-1, j] < -1e-9 and ub[j] == INF:
            raise ValueError("x%d" % (j + 1))
    return out


def solve_bounded_dual(c, A, rel, b, upper, lower=None, sense=0, flags=LONG_STEP, max_iter=10000):
    """lpx_solve_bounded_dual.  Returns a dict: status, x, value, T, basis, flip, ub, trace, counts, dualize_flips, constant."""
    T0, basis0, ub, lower, is_min, shifted, constant = prepare_dual(c, A, rel, b, lower, upper, sense)
    n = len(c)
    T1, flip, flips, bad = N.dualize(T0, ub, np.zeros(len(ub), dtype=np.uint8))
    assert bad == 0
    st, T, basis, flip, tr, counts = dual_run3(T1, basis0, ub, flip, flags, max_iter=max_iter)
    x = B.solution(T, basis, flip, ub, n)[0]
    if np.any(lower != 0.0):
        x = x + lower
    z = T[-1, -1]
    value = z
    if shifted or is_min:
        value = -z if is_min else z
        if shifted:
            value = value + constant
    return {"status": st, "x": x, "value": float(value), "T": T, "basis": basis, "flip": flip, "ub": ub, "trace": tr,
            "counts": counts, "dualize_flips": flips, "constant": constant}


# ---- the instances the CPU and the GPU tests share ---------------------------------------------------------------------
def covering_model(m, n, seed):
    """covering(m, n, seed) as a user model: (c, A, rel, b) of Min c.x, A x >= b."""
    _, _, _, (c, A, b) = D.covering(m, n, seed)
    return c, A, np.ones(m, dtype=np.int32), b


def mixed_model():
    """Min c.x with costs of both signs (the negative ones need a dualize flip) over six <= rows and six >= rows,
    0.5 <= x_1, x <= 2: (c, A, rel, b, upper, lower, sense)."""
    g = np.random.default_rng(11)
    A = g.integers(1, 9, size=(12, 16)).astype(np.float64)
    c = g.integers(1, 12, size=16).astype(np.float64) * np.where(g.uniform(size=16) < 0.3, -1.0, 1.0)
    rel = np.array([0, 1] * 6, dtype=np.int32)
    b = np.where(rel == 1, np.floor(0.9 * A.sum(axis=1)), np.floor(1.1 * A.sum(axis=1)) + 0.5)
    lower = np.zeros(16); lower[0] = 0.5
    return c, A, rel, b, np.full(16, 2.0), lower, 1
