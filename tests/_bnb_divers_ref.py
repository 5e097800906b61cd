"""NumPy restatement of the search by W divers (lpx_solve_bnb_bounded4, include/lpx.h): W copies of the solved root, each a
_bounded_long_ref.Handle with its own current bounds and its own depth-first stack; a round steals for the idle divers, pops
one node per diver, evaluates them with Handle.node2 and decides the records in diver order.  The order of the steps is the
contract's: limit, steal, pop, evaluate, decide.  Built on the existing helper modules, which it does not edit."""
import numpy as np

import _bnb_bounded_ref as N
import _bounded_long_ref as L
import _bounded_ref as B

INF = np.inf
EPS = N.EPS


def solve_divers(c, A, b, upper, W, lower=None, is_int=None, sense=0, max_nodes=0, max_iter=10000, rel=None, search_flags=0):
    """The dict of _bounded_long_ref.solve2 (without its pivot / pass statistics), plus rounds, steals, largest_batch, the
    per-record arrays round and diver, and critical_events: the sum over the rounds of the largest event count of the round."""
    assert W >= 1 and not search_flags & ~(L.LONG_STEP | L.CUTOFF_FLAG)
    T0, basis0, ub0, lower, is_min, shifted, constant = N.prepare(c, A, b, lower, upper, sense, rel)
    n = len(c)
    mask = None if is_int is None else np.asarray(is_int, dtype=np.uint8)
    st, Ts, bs, flip, _, _ = B.run(T0, basis0, ub0, max_iter=max_iter)
    out = {"rc": 0, "status": st, "x": None, "value": 0.0, "nodes": 0, "events": 0, "flips": 0, "incumbents": 0,
           "pruned_bound": 0, "pruned_infeasible": 0, "max_K": 0, "constant": constant, "rounds": 0, "steals": 0,
           "largest_batch": 0, "critical_events": 0, "log": np.zeros(0, dtype=N.LOG_DTYPE),
           "round": np.zeros(0, dtype=np.int32), "diver": np.zeros(0, dtype=np.int32)}
    if st != L.OPTIMAL:
        return out
    hs = [L.Handle(Ts, bs, ub0, flip) for _ in range(W)]
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
            out["rc"] = L.ITER_LIMIT
            break
        # 2. steal: the oldest entry of the longest stack (ties to the lowest index), lengths as they stand now
        for d in range(W):
            if stacks[d]:
                continue
            v = max(range(W), key=lambda i: (len(stacks[i]), -i))
            if len(stacks[v]) >= 2:
                stacks[d].append(stacks[v].pop(0))
                out["steals"] += 1
        # 3. pop, 4. evaluate (every entry with the cutoff of the start of the round)
        cutoff = best + EPS if search_flags & L.CUTOFF_FLAG else -INF
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
            rec = hs[d].node2(cols, nb_lo[cols], nb_ub[cols], n, mask, EPS, L.SKIP_FIXED | search_flags, cutoff, max_iter=max_iter)
            assert rec["status"] is not None, "unrepairable column"
            recs.append((d, depth, path, nb_lo, nb_ub, len(cols), rec))
        rnd = out["rounds"]
        out["rounds"] += 1
        out["largest_batch"] = max(out["largest_batch"], len(recs))
        out["critical_events"] += max(r[6]["events"] for r in recs)
        # 5. decide, in diver order
        for d, depth, path, nb_lo, nb_ub, K, rec in recs:
            out["nodes"] += 1
            cur[d] = (nb_lo, nb_ub)
            out["events"] += rec["events"]; out["flips"] += rec["flips"]; out["max_K"] = max(out["max_K"], K)
            log.append((depth, K, rec["status"], rec["events"], rec["flips"], rec["var"], rec["z"]))
            rounds.append(rnd); divers.append(d)
            if rec["status"] == L.ITER_LIMIT:
                out["rc"] = L.ITER_LIMIT
                stop = True
                break
            if rec["status"] == L.INFEASIBLE:
                out["pruned_infeasible"] += 1
                continue
            z = rec["z"]
            if rec["status"] == L.CUTOFF or z <= best + EPS:
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
            stacks[d].append((depth + 1, path + [(v, nb_lo[v], np.floor(xv))]))
            stacks[d].append((depth + 1, path + [(v, np.ceil(xv), nb_ub[v])]))     # explored first
    out["log"] = np.array(log, dtype=N.LOG_DTYPE)
    out["round"] = np.array(rounds, dtype=np.int32)
    out["diver"] = np.array(divers, dtype=np.int32)
    if best_x is None:
        out["status"] = L.INFEASIBLE
        return out
    x = best_x + lower if np.any(lower != 0.0) else best_x
    value = -best if is_min else best
    if shifted:
        value = value + constant
    out.update(status=L.OPTIMAL, x=x, value=float(value))
    return out
