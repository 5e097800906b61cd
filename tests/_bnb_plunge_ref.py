"""NumPy restatement of the plunge (lpx_node_batch_plunge and lpx_solve_bnb_bounded5, include/lpx.h): a chain is a sequence of
_bounded_long_ref.Handle.node2 calls on one handle -- the entry's triples, then the ceil child of every node that branches -- and
the search is that of _bnb_divers_ref.solve_divers with a chain per diver and round.  The order of the steps is the contract's:
limit, steal, pop with the caps, evaluate, decide in diver and chain order.  Built on the existing helper modules, which it does
not edit."""
import numpy as np

import _bnb_bounded_ref as N
import _bounded_long_ref as L
import _bounded_ref as B

INF = np.inf
EPS = N.EPS


def chain(h, nd, nint, depth, prune=-INF, is_int=None, flags=L.SKIP_FIXED, cutoff=-INF, **kw):
    """The chain of one entry on the handle h: the records in order.  A refused node (status None) ends it and leaves the handle
    as the node before left it; its record is the last of the list."""
    cols, lower, upper = nd
    recs = []
    for s in range(depth):
        rec = h.node2(np.asarray(cols, dtype=np.int32), np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64),
                      nint, is_int, flags=flags, cutoff=cutoff, **kw)
        recs.append(rec)
        if rec["status"] is None:
            break
        if not (rec["status"] == L.OPTIMAL and rec["var"] >= 0 and not rec["z"] <= prune):
            break
        v = rec["var"]
        cols, lower, upper = [v], [np.ceil(rec["x_var"])], [h.lo[v] + h.ub[v]]     # in the handle's own terms
    return recs


def solve_plunge(c, A, b, upper, W, D, lower=None, is_int=None, sense=0, max_nodes=0, max_iter=10000, rel=None, search_flags=0):
    """The dict of _bnb_divers_ref.solve_divers plus step (per record), launched, dropped, longest_chain and chains: the
    (round, diver, records written, records kept, cap) of every chain."""
    assert W >= 1 and 1 <= D <= 64 and not search_flags & ~(L.LONG_STEP | L.CUTOFF_FLAG)
    T0, basis0, ub0, lower, is_min, shifted, constant = N.prepare(c, A, b, lower, upper, sense, rel)
    n = len(c)
    mask = None if is_int is None else np.asarray(is_int, dtype=np.uint8)
    st, Ts, bs, flip, _, _ = B.run(T0, basis0, ub0, max_iter=max_iter)
    out = {"rc": 0, "status": st, "x": None, "value": 0.0, "nodes": 0, "events": 0, "flips": 0, "incumbents": 0,
           "pruned_bound": 0, "pruned_infeasible": 0, "max_K": 0, "constant": constant, "rounds": 0, "steals": 0,
           "largest_batch": 0, "launched": 0, "dropped": 0, "longest_chain": 0, "chains": [], "refusals": 0,
           "log": np.zeros(0, dtype=N.LOG_DTYPE), "round": np.zeros(0, dtype=np.int32), "diver": np.zeros(0, dtype=np.int32),
           "step": np.zeros(0, dtype=np.int32)}
    if st != L.OPTIMAL:
        return out
    hs = [L.Handle(Ts, bs, ub0, flip) for _ in range(W)]
    root_lo, root_ub = np.zeros(n), ub0[:n].copy()
    cur = [(root_lo.copy(), root_ub.copy()) for _ in range(W)]
    stacks = [[] for _ in range(W)]
    stacks[0].append((0, []))
    best, best_x = -INF, None
    log, rounds, divers, steps = [], [], [], []
    stop = False
    while not stop and any(stacks):
        # 1. limit
        if max_nodes > 0 and out["nodes"] >= max_nodes:
            out["rc"] = L.ITER_LIMIT
            break
        # 2. steal
        for d in range(W):
            if stacks[d]:
                continue
            v = max(range(W), key=lambda i: (len(stacks[i]), -i))
            if len(stacks[v]) >= 2:
                stacks[d].append(stacks[v].pop(0))
                out["steals"] += 1
        # 3. pop with the caps, 4. evaluate (every entry against the best of the start of the round)
        prune = best + EPS
        cutoff = prune if search_flags & L.CUTOFF_FLAG else -INF
        ent, handed = [], 0
        for d in range(W):
            if not stacks[d]:
                continue
            cap = D
            if max_nodes > 0:
                left = max_nodes - out["nodes"] - handed
                if left <= 0:
                    break
                cap = min(cap, left)
            handed += cap
            depth, path = stacks[d].pop()
            nb_lo, nb_ub = root_lo.copy(), root_ub.copy()
            for var, l, u in path:
                nb_lo[var], nb_ub[var] = l, u
            cols = np.flatnonzero((nb_lo != cur[d][0]) | (nb_ub != cur[d][1])).astype(np.int32)      # ascending
            recs = chain(hs[d], (cols, nb_lo[cols], nb_ub[cols]), n, cap, prune, mask, L.SKIP_FIXED | search_flags, cutoff,
                         max_iter=max_iter)
            if recs[-1]["status"] is None:
                out["refusals"] += 1
                assert len(recs) > 1, "unrepairable column at the first node of a chain"
                raise AssertionError("a refusal inside a chain: the driver raises here")
            ent.append((d, depth, path, nb_lo, nb_ub, len(cols), recs, cap))
        rnd = out["rounds"]
        out["rounds"] += 1
        out["largest_batch"] = max(out["largest_batch"], len(ent))
        for e in ent:
            out["launched"] += len(e[6])
            out["longest_chain"] = max(out["longest_chain"], len(e[6]))
        # 5. decide: divers ascending, each diver's records in chain order
        for d, depth, path, nb_lo, nb_ub, K0, recs, cap in ent:
            if stop:
                break
            kept = 0
            for s, rec in enumerate(recs):
                has_next = s + 1 < len(recs)
                K = K0 if s == 0 else 1
                out["nodes"] += 1
                kept += 1
                out["events"] += rec["events"]; out["flips"] += rec["flips"]; out["max_K"] = max(out["max_K"], K)
                log.append((depth, K, rec["status"], rec["events"], rec["flips"], rec["var"], rec["z"]))
                rounds.append(rnd); divers.append(d); steps.append(s)
                if rec["status"] == L.ITER_LIMIT:
                    out["rc"] = L.ITER_LIMIT
                    stop = True
                    break
                if rec["status"] == L.INFEASIBLE:
                    out["pruned_infeasible"] += 1
                    break
                z = rec["z"]
                if rec["status"] == L.CUTOFF or z <= best + EPS:
                    out["pruned_bound"] += 1
                    out["dropped"] += len(recs) - 1 - s
                    for rk in recs[s:-1]:               # the handle holds the bounds of the last node evaluated
                        nb_lo[rk["var"]] = np.ceil(rk["x_var"])
                    break
                if rec["var"] < 0:
                    assert not has_next
                    h = hs[d]
                    x = N.values(h.T, h.basis, h.flip, h.ub, h.lo, n).copy()
                    ints = np.ones(n, dtype=bool) if mask is None else mask != 0
                    x[ints] = np.rint(x[ints])
                    best, best_x = z, x
                    out["incumbents"] += 1
                    break
                v, xv = rec["var"], rec["x_var"]
                stacks[d].append((depth + 1, path + [(v, nb_lo[v], np.floor(xv))]))
                ce = (depth + 1, path + [(v, np.ceil(xv), nb_ub[v])])
                if has_next:                            # the ceil child is the next record
                    depth, path = ce
                    nb_lo[v] = np.ceil(xv)
                else:
                    stacks[d].append(ce)
            cur[d] = (nb_lo, nb_ub)
            out["chains"].append((rnd, d, len(recs), kept, cap))
    out["log"] = np.array(log, dtype=N.LOG_DTYPE)
    out["round"] = np.array(rounds, dtype=np.int32)
    out["diver"] = np.array(divers, dtype=np.int32)
    out["step"] = np.array(steps, dtype=np.int32)
    if best_x is None:
        out["status"] = L.INFEASIBLE
        return out
    x = best_x + lower if np.any(lower != 0.0) else best_x
    value = -best if is_min else best
    if shifted:
        value = value + constant
    out.update(status=L.OPTIMAL, x=x, value=float(value))
    return out
