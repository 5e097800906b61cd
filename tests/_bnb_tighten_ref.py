"""NumPy restatement of reduced-cost bound tightening (include/lpx.h, "reduced-cost tightening"): the rule itself, lpx_bounded_node5
and the search lpx_solve_bnb_bounded10(tighten = 1), written from the contract in include/lpx.h, not from the kernel.  Test
infrastructure: the GPU tests compare the device against it bit for bit.  The node is the guard restatement's
(_bounded_guard_ref.Handle.node4) and the search is _bounded_guard_ref.solve_guard -- which with stall_events = 0 is
_bnb_divers_ref.solve_divers -- with its steps 3 and 5 changed as the contract says; the helper modules are imported unchanged."""
import functools

import numpy as np

import _bnb_bounded_ref as N
import _bounded_guard_ref as G
import _bounded_long_ref as L
import _bounded_ref as B

OPTIMAL, INFEASIBLE, ITER_LIMIT, CUTOFF = L.OPTIMAL, L.INFEASIBLE, L.ITER_LIMIT, L.CUTOFF
SKIP_FIXED, LONG_STEP, CUTOFF_FLAG = L.SKIP_FIXED, L.LONG_STEP, L.CUTOFF_FLAG
INF = np.inf
EPS = N.EPS


def tighten(handle, nint, is_int, z, fix_bound, eps=1e-9):
    """The rule on a handle whose node ended OPTIMAL with objective z: every column j < nint that the mask admits, that is not
    basic and whose reduced cost d = T[m,j] exceeds eps gets t = floor((z - fix_bound) / d) -- one subtract, one divide, each
    rounded on its own -- and is tightened iff t < ub[j].  Edits handle.ub and handle.lo in place, nothing else.  Returns the
    reported triples (cols int32, lower, upper), ascending in j."""
    T, ub, lo, flip = handle.T, handle.ub, handle.lo, handle.flip
    m = T.shape[0] - 1
    basic = np.zeros(len(ub), dtype=bool)
    stored = (handle.basis >= 0) & (handle.basis < len(ub))
    basic[handle.basis[stored]] = True                     # marked through the basis, never inferred from a zero
    cols, lower, upper = [], [], []
    if not (z > fix_bound and fix_bound > -INF):
        return np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0)
    gap = np.float64(z) - np.float64(fix_bound)            # one subtract
    for j in range(nint):
        if is_int is not None and not is_int[j]:
            continue
        if basic[j]:
            continue
        d = T[m, j]
        if not d > eps:
            continue
        g = gap / d                                        # one IEEE divide
        t = np.floor(g)
        if not t < ub[j]:
            continue
        if flip[j]:
            up = lo[j] + ub[j]
            lw = up - t
            lo[j] = lw
        else:
            lw = lo[j]
            up = lo[j] + t
        ub[j] = t
        cols.append(j); lower.append(lw); upper.append(up)
    return np.array(cols, dtype=np.int32), np.array(lower, dtype=np.float64), np.array(upper, dtype=np.float64)


class Handle(G.Handle):
    """The state a device handle carries between node calls, with lpx_bounded_node5."""

    def clone(self):
        return Handle(self.T.copy(), self.basis.copy(), self.ub.copy(), self.flip.copy(), self.lo.copy())

    def node5(self, cols, lower, upper, nint, is_int=None, tol=EPS, flags=SKIP_FIXED, cutoff=-INF, stall_events=0, fix_bound=-INF,
              eps=1e-9, ratio_tol=1e-12, max_iter=10000):
        """lpx_bounded_node5 in its on-chip form: the record of node4 plus fixed = (cols, lower, upper).  The rule runs behind the
        pick, only on a node that ended OPTIMAL with z > fix_bound."""
        assert fix_bound == fix_bound
        rec = self.node4(cols, lower, upper, nint, is_int, tol, flags, cutoff, stall_events, eps, ratio_tol, max_iter)
        rec["fixed"] = (np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0))
        if rec["status"] == OPTIMAL:
            self.ub, self.lo = self.ub.copy(), self.lo.copy()
            rec["fixed"] = tighten(self, nint, is_int, rec["z"], fix_bound, eps)
        return rec


def solve_tighten(c, A, b, upper, W, stall_events=0, lower=None, is_int=None, sense=0, max_nodes=0, max_iter=10000, rel=None,
                  search_flags=0, tighten_on=True, on_node=None, on_done=None):
    """lpx_solve_bnb_bounded10: the search of _bounded_guard_ref.solve_guard step for step, every node a node5 call.  With
    tighten_on, step 3 gives every entry fix_bound = best + EPS of the start of the round (-inf without an incumbent), and step 5
    applies a record's triples to the bounds held for the diver's handle and, where the node branches, appends them to both
    children's paths in front of the branching override.  The dict of solve_guard plus tightened_nodes, tightened_cols and
    max_per_node.  on_node(index, diver, handle, cols, lower, upper, cutoff, fix_bound) is called in front of every evaluation
    with the handle as it stands, on_done(index, diver, handle, rec) behind it."""
    assert W >= 1 and not search_flags & ~(LONG_STEP | CUTOFF_FLAG)
    T0, basis0, ub0, lower, is_min, shifted, constant = N.prepare(c, A, b, lower, upper, sense, rel)
    n = len(c)
    mask = None if is_int is None else np.asarray(is_int, dtype=np.uint8)
    st, Ts, bs, flip, _, _ = B.run(T0, basis0, ub0, max_iter=max_iter)
    out = {"rc": 0, "status": st, "x": None, "value": 0.0, "nodes": 0, "events": 0, "flips": 0, "incumbents": 0,
           "pruned_bound": 0, "pruned_infeasible": 0, "max_K": 0, "constant": constant, "rounds": 0, "steals": 0,
           "largest_batch": 0, "guarded_nodes": 0, "bland_events": 0, "max_events": 0, "tightened_nodes": 0, "tightened_cols": 0,
           "max_per_node": 0, "log": np.zeros(0, dtype=N.LOG_DTYPE), "round": np.zeros(0, dtype=np.int32),
           "diver": np.zeros(0, dtype=np.int32), "root": None}
    if st != OPTIMAL:
        return out
    out["root"] = (Ts.copy(), bs.copy(), ub0.copy(), flip.copy())
    hs = [Handle(Ts, bs, ub0, flip) for _ in range(W)]
    root_lo, root_ub = np.zeros(n), ub0[:n].copy()
    cur = [(root_lo.copy(), root_ub.copy()) for _ in range(W)]
    stacks = [[] for _ in range(W)]
    stacks[0].append((0, []))
    best, best_x = -INF, None
    log, rounds, divers = [], [], []
    stop = False
    while not stop and any(stacks):
        # 1. limit
        if max_nodes > 0 and out["nodes"] >= max_nodes:
            out["rc"] = ITER_LIMIT
            break
        # 2. steal: the oldest entry of the longest stack (ties to the lowest index), lengths as they stand now
        for d in range(W):
            if stacks[d]:
                continue
            v = max(range(W), key=lambda i: (len(stacks[i]), -i))
            if len(stacks[v]) >= 2:
                stacks[d].append(stacks[v].pop(0))
                out["steals"] += 1
        # 3. pop, 4. evaluate (every entry with the cutoff and the fix_bound of the start of the round)
        cutoff = best + EPS if search_flags & CUTOFF_FLAG else -INF
        fix_bound = best + EPS if tighten_on else -INF             # -inf + EPS = -inf: off while there is no incumbent
        recs = []
        for d in range(W):
            if not stacks[d]:
                continue
            if max_nodes > 0 and out["nodes"] + len(recs) >= max_nodes:
                break
            depth, path = stacks[d].pop()
            nb_lo, nb_ub = root_lo.copy(), root_ub.copy()
            for var, l, u in path:
                nb_lo[var], nb_ub[var] = l, u
            cols = np.flatnonzero((nb_lo != cur[d][0]) | (nb_ub != cur[d][1])).astype(np.int32)      # ascending
            index = out["nodes"] + len(recs)
            if on_node is not None:
                on_node(index, d, hs[d], cols, nb_lo[cols], nb_ub[cols], cutoff, fix_bound)
            rec = hs[d].node5(cols, nb_lo[cols], nb_ub[cols], n, mask, EPS, SKIP_FIXED | search_flags, cutoff, stall_events,
                              fix_bound, max_iter=max_iter)
            assert rec["status"] is not None, "unrepairable column"
            if on_done is not None:
                on_done(index, d, hs[d], rec)
            recs.append((d, depth, path, nb_lo, nb_ub, len(cols), rec))
        rnd = out["rounds"]
        out["rounds"] += 1
        out["largest_batch"] = max(out["largest_batch"], len(recs))
        # 5. decide, in diver order
        for d, depth, path, nb_lo, nb_ub, K, rec in recs:
            out["nodes"] += 1
            fc, fl, fu = rec["fixed"]
            nb_lo, nb_ub = nb_lo.copy(), nb_ub.copy()              # copies: the handle holds the tightened bounds already
            nb_lo[fc], nb_ub[fc] = fl, fu
            if len(fc):
                out["tightened_nodes"] += 1
                out["tightened_cols"] += len(fc)
                out["max_per_node"] = max(out["max_per_node"], len(fc))
            cur[d] = (nb_lo, nb_ub)
            out["events"] += rec["events"]; out["flips"] += rec["flips"]; out["max_K"] = max(out["max_K"], K)
            log.append((depth, K, rec["status"], rec["events"], rec["flips"], rec["var"], rec["z"]))
            rounds.append(rnd); divers.append(d)
            if rec["bland_events"] > 0:
                out["guarded_nodes"] += 1
                out["bland_events"] += rec["bland_events"]
            out["max_events"] = max(out["max_events"], rec["events"])
            if rec["status"] == ITER_LIMIT:
                out["rc"] = ITER_LIMIT
                stop = True
                break
            if rec["status"] == INFEASIBLE:
                out["pruned_infeasible"] += 1
                continue
            z = rec["z"]
            if rec["status"] == CUTOFF or z <= best + EPS:
                out["pruned_bound"] += 1
                continue
            if rec["var"] < 0:
                h = hs[d]
                x = N.values(h.T, h.basis, h.flip, h.ub, h.lo, n).copy()
                ints = np.ones(n, dtype=bool) if mask is None else mask != 0
                x[ints] = np.rint(x[ints])
                best, best_x = z, x
                out["incumbents"] += 1
                continue
            v, xv = rec["var"], rec["x_var"]
            down = path + [(int(j), float(l), float(u)) for j, l, u in zip(fc, fl, fu)]       # in front of the branching override
            stacks[d].append((depth + 1, down + [(v, nb_lo[v], np.floor(xv))]))
            stacks[d].append((depth + 1, down + [(v, np.ceil(xv), nb_ub[v])]))     # explored first
    out["log"] = np.array(log, dtype=N.LOG_DTYPE)
    out["round"] = np.array(rounds, dtype=np.int32)
    out["diver"] = np.array(divers, dtype=np.int32)
    if best_x is None:
        out["status"] = INFEASIBLE
        return out
    x = best_x + lower if np.any(lower != 0.0) else best_x
    value = -best if is_min else best
    if shifted:
        value = value + constant
    out.update(status=OPTIMAL, x=x, value=float(value), best=float(best))
    return out


# ---- the instances the CPU and the GPU tests share, each computed once ---------------------------------------------------
IP_MODELS = ((16, 4), (24, 6), (32, 8))


@functools.lru_cache(maxsize=None)
def ip_model(n, m):
    """binary_ip(n, m) with its rows [:m] and upper = 1: (c, A, b, upper)."""
    from linear_programming_solver_lpr381_amd import synth
    c, A, _, b = synth.binary_ip(n, m)
    return c, A[:m], b[:m], np.ones(n)


@functools.lru_cache(maxsize=None)
def ip_search(n, m, W, flags, tighten_on=True):
    """solve_tighten of ip_model(n, m) by W divers with the search flags `flags`."""
    c, A, b, up = ip_model(n, m)
    return solve_tighten(c, A, b, up, W, search_flags=flags, tighten_on=tighten_on)
