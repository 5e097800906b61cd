"""NumPy restatement of lpx_solve_bnb_bounded10 with its switches combined (root_cuts, stall_events and tighten together), written
from the contract in include/lpx.h.  Test infrastructure: the GPU tests compare the device against it bit for bit.  Nothing here
is new arithmetic: the preparation and the pick are _bnb_bounded_ref's, the root solve _bounded_ref.run, the spare capacity, the
slack mask and the cut loop _bnb_cuts_ref's, the node _bnb_tighten_ref.Handle.node5 and the round loop that of
_bnb_tighten_ref.solve_tighten (its own copy: that one starts from the model, this one from the handle the cut loop leaves).  The
helper modules are imported unchanged."""
import functools

import numpy as np

import _bnb_bounded_ref as N
import _bnb_cuts_ref as X
import _bnb_tighten_ref as R
import _bounded_ref as B

OPTIMAL, INFEASIBLE, ITER_LIMIT, CUTOFF = R.OPTIMAL, R.INFEASIBLE, R.ITER_LIMIT, R.CUTOFF
SKIP_FIXED, LONG_STEP, CUTOFF_FLAG = R.SKIP_FIXED, R.LONG_STEP, R.CUTOFF_FLAG
INF = np.inf
EPS = N.EPS


def solve_combined(c, A, b, upper, W, root_cuts=None, stall_events=0, tighten_on=True, search_flags=0, lower=None, is_int=None,
                   sense=0, rel=None, max_nodes=0, max_iter=10000, on_node=None, on_done=None):
    """lpx_solve_bnb_bounded10.  root_cuts: a _gmi_ref.CutOpts or None.  The dict of _bnb_tighten_ref.solve_tighten plus cut: the
    cut loop's record with spare and ran, as _bnb_cuts_ref.solve_cuts returns it (None without root_cuts).  on_node / on_done as
    in solve_tighten."""
    assert W >= 1 and not search_flags & ~(LONG_STEP | CUTOFF_FLAG)
    T0, basis0, ub0, lower, is_min, shifted, constant = N.prepare(c, A, b, lower, upper, sense, rel)
    n = len(c)
    mask = None if is_int is None else np.asarray(is_int, dtype=np.uint8)
    st, Ts, bs, flip, _, _ = B.run(T0, basis0, ub0, max_iter=max_iter)
    out = {"rc": 0, "status": st, "x": None, "value": 0.0, "nodes": 0, "events": 0, "flips": 0, "incumbents": 0,
           "pruned_bound": 0, "pruned_infeasible": 0, "max_K": 0, "constant": constant, "rounds": 0, "steals": 0,
           "largest_batch": 0, "guarded_nodes": 0, "bland_events": 0, "max_events": 0, "tightened_nodes": 0, "tightened_cols": 0,
           "max_per_node": 0, "log": np.zeros(0, dtype=N.LOG_DTYPE), "round": np.zeros(0, dtype=np.int32),
           "diver": np.zeros(0, dtype=np.int32), "root": None, "cut": None}
    if st != OPTIMAL:
        return out
    out["root"] = (Ts.copy(), bs.copy(), ub0.copy(), flip.copy())
    h = R.Handle(Ts, bs, ub0, flip)
    if root_cuts is not None:
        Rr, Cc = Ts.shape
        a = X.spare(Rr, Cc, root_cuts.max_active)
        cut = {"spare": a, "ran": 0}
        if a > 0:
            cut.update(X.cut_loop(h, X.slack_mask(T0, n, is_int), Cc - 1, Cc - 1, n, mask, root_cuts, search_flags, Rr + a, Cc + a,
                                  max_iter))
            cut["ran"] = 1
        out["cut"] = cut
        # "status" ends the search here as the device does (SolveBnbDivers in csrc/host/bnb_bounded.cpp returns on
        # LPX_CUTLOOP_STATUS); _bnb_cuts_ref.solve_cuts goes on to search in that case.  With the loop's cutoff at -inf no
        # re-optimisation ends CUTOFF, so the stop does not occur and the two restatements agree on every model.
        if cut["ran"] and cut["stop"] in ("infeasible", "status"):             # no node is searched
            out["status"] = INFEASIBLE
            return out
        if cut["ran"] and cut["stop"] == "iter_limit":
            out["rc"] = ITER_LIMIT
            out["status"] = INFEASIBLE
            return out
    hs = [h] + [h.clone() for _ in range(W - 1)]                              # the clones are made after the loop
    root_lo, root_ub = np.zeros(n), ub0[:n].copy()                            # the root bounds are the model's
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
                g = hs[d]
                x = N.values(g.T, g.basis, g.flip, g.ub, g.lo, n).copy()
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
def model(name):
    """name -> (c, A, rel, b, upper, lower, is_int, sense): ("ip", n, m) is _bnb_tighten_ref.ip_model, ("bm", n, m, seed) is
    _bnb_bounded_ref.binary_model with upper = 1, a string a model of _bnb_bounded_ref.small_models."""
    if isinstance(name, str):
        return N.small_models()[name]
    if name[0] == "ip":
        c, A, b, up = R.ip_model(name[1], name[2])
    else:
        c, A, b = N.binary_model(*name[1:])
        up = np.ones(len(c))
    return c, A, np.zeros(len(b), dtype=np.int32), b, up, None, None, 0


def is_binary(name):
    return not isinstance(name, str)


@functools.lru_cache(maxsize=None)
def search(name, W, flags, S, rounds=4, K=8, tighten_on=True, max_nodes=0):
    """solve_combined of model(name) by W divers with the search flags `flags`, stall_events = S and, with rounds > 0, root cuts
    CutOpts(cuts_per_round=K, max_rounds=rounds).  Cached: the result is shared and must not be edited."""
    import _gmi_ref as G
    c, A, rel, b, upper, lower, is_int, sense = model(name)
    o = G.CutOpts(cuts_per_round=K, max_rounds=rounds) if rounds else None
    return solve_combined(c, A, b, upper, W, o, S, tighten_on, flags, lower=lower, is_int=is_int, sense=sense, rel=rel,
                          max_nodes=max_nodes)
