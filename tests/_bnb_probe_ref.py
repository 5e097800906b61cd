"""NumPy restatement of the strong-branching probes (lpx_bounded_probe, lpx_node_batch_run_probe) and of the search that uses
them (lpx_solve_bnb_bounded6), written from the contract in include/lpx.h ("strong branching by on-chip probes"), not from the
kernel.  A probe is Handle.node2 of _bounded_long_ref on a copy of the handle with K = 1; the search is the round of
_bnb_divers_ref.solve_divers with the two changed steps.  Built on the existing helper modules, which it does not edit."""
import numpy as np

import _bnb_bounded_ref as N
import _bounded_long_ref as L
import _bounded_ref as B

INF = np.inf
EPS = N.EPS
PROBE_NONE = -2
GAIN_MIN, GAIN_MAX = 1e-6, 1e12
SINFO_KEYS = ("probe_launches", "probes", "probe_events", "probe_limit", "pruned_by_probe", "changed_picks")


def clone(h):
    c = L.Handle(h.T, h.basis, h.ub, h.flip, h.lo)
    c.trace = h.trace.copy()
    return c


def candidates(h, nint, is_int=None, tol=EPS):
    """(columns in probe order, x of every column j < nint): the fractional integer columns by (|f - 0.5|, j) ascending."""
    x = N.values(h.T, h.basis, h.flip, h.ub, h.lo, nint)
    f = x - np.floor(x)
    with np.errstate(invalid="ignore"):
        cand = (f > tol) & ((1.0 - f) > tol)
    if is_int is not None:
        cand &= np.asarray(is_int)[:nint] != 0
    J = np.flatnonzero(cand)
    d = np.abs(f[J] - 0.5)
    return J[np.lexsort((J, d))], x


def probe(h, nint, cand_max, probe_iter, last_status=L.OPTIMAL, is_int=None, tol=EPS, flags=L.SKIP_FIXED, cutoff=-INF, prune=-INF,
          eps=1e-9, ratio_tol=1e-12):
    """lpx_bounded_probe on the restatement's handle h, which is only read.  Returns {count, candidates, z, records}; a record
    is {status (None: refused), events, kind0, kind1, flips, var, dir, x_var, lower, upper, z}."""
    z = float(h.T[-1, -1])
    out = {"count": 0, "candidates": 0, "z": z, "records": []}
    if last_status != L.OPTIMAL or z <= prune:
        return out
    order, x = candidates(h, nint, is_int, tol)
    out["candidates"] = len(order)
    out["count"] = min(len(order), cand_max)
    for j in order[:out["count"]]:
        j = int(j)
        xv = x[j]
        lj, uj = h.lo[j], h.ub[j]
        for d, (lw, up) in enumerate(((lj, np.floor(xv)), (np.ceil(xv), lj + uj))):
            if up < lw:                 # an empty interval (a bound that is not integral): the node call refuses it
                out["records"].append({"status": None, "events": 0, "kind0": 0, "kind1": 0, "flips": 0, "var": j, "dir": d,
                                       "x_var": float(xv), "lower": float(lw), "upper": float(up), "z": 0.0})
                continue
            r = clone(h).node2(np.array([j], dtype=np.int32), np.array([lw]), np.array([up]), nint, is_int, tol, flags, cutoff, eps,
                               ratio_tol, max_iter=probe_iter)
            rec = {"status": r["status"], "events": r["events"], "kind0": r["kind0"], "kind1": r["kind1"], "flips": r["flips"],
                   "var": j, "dir": d, "x_var": float(xv), "lower": float(lw), "upper": float(up), "z": r["z"]}
            if r["status"] is None:
                rec.update(events=0, kind0=0, kind1=0, flips=0, z=0.0)
            out["records"].append(rec)
    return out


def gain(rec, z):
    if rec["status"] in (L.INFEASIBLE, L.CUTOFF):
        return GAIN_MAX
    if rec["status"] is None:
        return GAIN_MIN
    return min(max(z - rec["z"], GAIN_MIN), GAIN_MAX)


def dead(rec, best):
    return rec["status"] in (L.INFEASIBLE, L.CUTOFF) or (rec["status"] == L.OPTIMAL and rec["z"] <= best + EPS)


def choose(pr, z):
    """The candidate of the first maximum of gain_floor * gain_ceil, in candidate order."""
    pick, top = 0, -1.0
    for c in range(pr["count"]):
        score = gain(pr["records"][2 * c], z) * gain(pr["records"][2 * c + 1], z)
        if score > top:
            pick, top = c, score
    return pick


def solve_strong(c, A, b, upper, W, lower=None, is_int=None, sense=0, max_nodes=0, max_iter=10000, rel=None, search_flags=0,
                 branching=1, cand_max=4, probe_iter=None):
    """lpx_solve_bnb_bounded6.  The dict of _bnb_divers_ref.solve_divers plus the counters of lpx_bnb_strong_info and
    probe_critical_events: the sum over the rounds of the largest event count of a probe of the round."""
    assert W >= 1 and not search_flags & ~(L.LONG_STEP | L.CUTOFF_FLAG) and branching in (0, 1) and 1 <= cand_max <= 32
    probe_iter = max_iter if probe_iter is None else probe_iter
    T0, basis0, ub0, lower, is_min, shifted, constant = N.prepare(c, A, b, lower, upper, sense, rel)
    n = len(c)
    mask = None if is_int is None else np.asarray(is_int, dtype=np.uint8)
    st, Ts, bs, flip, _, _ = B.run(T0, basis0, ub0, max_iter=max_iter)
    out = {"rc": 0, "status": st, "x": None, "value": 0.0, "nodes": 0, "events": 0, "flips": 0, "incumbents": 0,
           "pruned_bound": 0, "pruned_infeasible": 0, "max_K": 0, "constant": constant, "rounds": 0, "steals": 0,
           "largest_batch": 0, "critical_events": 0, "probe_critical_events": 0, "log": np.zeros(0, dtype=N.LOG_DTYPE),
           "round": np.zeros(0, dtype=np.int32), "diver": np.zeros(0, dtype=np.int32)}
    out.update({k: 0 for k in SINFO_KEYS})
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
        # 2. steal
        for d in range(W):
            if stacks[d]:
                continue
            v = max(range(W), key=lambda i: (len(stacks[i]), -i))
            if len(stacks[v]) >= 2:
                stacks[d].append(stacks[v].pop(0))
                out["steals"] += 1
        # 3. pop, 4. evaluate: the node, then the probes of the handle as the node left it, both against the start of the round
        cutoff = best + EPS if search_flags & L.CUTOFF_FLAG else -INF
        prune = best + EPS
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
            pr = None
            if branching:
                pr = probe(hs[d], n, cand_max, probe_iter, rec["status"], mask, EPS, L.SKIP_FIXED | search_flags, cutoff, prune)
            recs.append((d, depth, path, nb_lo, nb_ub, len(cols), rec, pr))
        rnd = out["rounds"]
        out["rounds"] += 1
        out["largest_batch"] = max(out["largest_batch"], len(recs))
        out["critical_events"] += max(r[6]["events"] for r in recs)
        if branching:
            out["probe_launches"] += 1
            ran = [q for r in recs for q in r[7]["records"]]
            out["probes"] += len(ran)
            out["probe_events"] += sum(q["events"] for q in ran)
            out["probe_limit"] += sum(1 for q in ran if q["status"] == L.ITER_LIMIT)
            out["probe_critical_events"] += max([q["events"] for q in ran], default=0)
        # 5. decide, in diver order
        for d, depth, path, nb_lo, nb_ub, K, rec, pr in recs:
            out["nodes"] += 1
            cur[d] = (nb_lo, nb_ub)
            out["events"] += rec["events"]; out["flips"] += rec["flips"]; out["max_K"] = max(out["max_K"], K)
            log.append([depth, K, rec["status"], rec["events"], rec["flips"], rec["var"], rec["z"]])
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
            push = [True, True]
            if branching and pr["count"] >= 1:
                pick = choose(pr, z)
                fl, ce = pr["records"][2 * pick], pr["records"][2 * pick + 1]
                v, xv = fl["var"], fl["x_var"]
                out["changed_picks"] += pick != 0
                push = [not dead(fl, best), not dead(ce, best)]
                out["pruned_by_probe"] += 2 - sum(push)
                log[-1][5] = v
            if push[0]:
                stacks[d].append((depth + 1, path + [(v, nb_lo[v], np.floor(xv))]))
            if push[1]:
                stacks[d].append((depth + 1, path + [(v, np.ceil(xv), nb_ub[v])]))     # explored first
    out["log"] = np.array([tuple(r) for r in log], dtype=N.LOG_DTYPE)
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
