"""NumPy restatement of GMI cuts on a bounded handle (lpx_tableau_gmi_round_bounded), of the cut loop at a bounded root
(lpx_bounded_cut_loop) and of the search by W divers that starts from the handle the loop leaves (lpx_solve_bnb_bounded9), written
from include/lpx.h.  Test infrastructure: the GPU tests compare the device against it bit for bit.  The round's arithmetic is
_gmi_ref.gmi_round, the re-optimisation _bounded_long_ref.Handle.node2, the pick and the preparation _bnb_bounded_ref's, the root
solve _bounded_ref.run -- all imported unchanged; what is new (the integer notion under bounds, the bounds carried across the
reshape, the loop, the slack mask, the capacity rule and the diver loop from a given handle) is spelled out here."""
import numpy as np

import _bnb_bounded_ref as N
import _bounded_long_ref as L
import _bounded_ref as B
import _gmi_ref as G

INF = np.inf
EPS = N.EPS
STOPS = ("integral", "stalled", "rounds", "infeasible", "iter_limit", "status")


def node_fits(R, C):
    """lpx_bounded_node_fits: the formula of include/lpx.h."""
    return R >= 2 and C >= 1 and 8 * (R * (C | 1) + C + max(R, C)) <= 160 * 1024 - 2 * 1024


def integer_columns(is_int, n_mask, first_cut_col, lo, ub, Cm):
    """The round's integer array [Cm]: flagged, in front of min(n_mask, first_cut_col), and both bounds whole."""
    nint = min(n_mask, first_cut_col)
    out = np.zeros(Cm, dtype=np.uint8)
    flag = np.asarray(is_int[:nint]) != 0
    if lo is None:
        out[:nint] = flag
        return out
    lo = np.asarray(lo, dtype=np.float64)[:nint]
    ub = np.asarray(ub, dtype=np.float64)[:nint]
    with np.errstate(invalid="ignore"):
        whole = (lo == np.floor(lo)) & ((ub == INF) | (ub == np.floor(ub)))
    out[:nint] = flag & whole
    return out


def round_bounded(T, basis, ub, lo, flip, is_int, n_mask, first_cut_col, o, Rcap, Ccap):
    """lpx_tableau_gmi_round_bounded on copies.  Returns (T, basis, ub, lo, flip, src_rows, purged_cols); o.cuts_per_round may be 0."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    Cm = T.shape[1] - 1
    eff = integer_columns(is_int, n_mask, first_cut_col, lo, ub, Cm)
    T2, b2, src, pcol = G.gmi_round(T.copy(), np.asarray(basis, dtype=np.int32).copy(), eff, Cm, first_cut_col, o, Rcap, Ccap)
    K, P = len(src), len(pcol)
    if K == 0 and P == 0:
        return T2, b2, np.array(ub, dtype=np.float64), np.array(lo, dtype=np.float64), np.array(flip, dtype=np.uint8), [], []
    keep = [j for j in range(Cm) if j not in set(pcol)]
    ub2 = np.concatenate([np.asarray(ub, dtype=np.float64)[keep], np.full(K, INF)])
    lo2 = np.concatenate([np.asarray(lo, dtype=np.float64)[keep], np.zeros(K)])
    flip2 = np.concatenate([np.asarray(flip, dtype=np.uint8)[keep], np.zeros(K, dtype=np.uint8)])
    return T2, b2, ub2, lo2, flip2, list(src), list(pcol)


def handle_round(h, is_int, n_mask, first_cut_col, o, Rcap, Ccap):
    """The round on a Handle, in place.  Returns (src_rows, purged_cols, alphas[K, old Cm]): the K cuts over the columns in front of
    the round (purged ones included, where they are zero)."""
    Cm = h.T.shape[1] - 1
    T2, b2, ub2, lo2, flip2, src, pcol = round_bounded(h.T, h.basis, h.ub, h.lo, h.flip, is_int, n_mask, first_cut_col, o, Rcap, Ccap)
    K, P = len(src), len(pcol)
    al = np.zeros((K, Cm))
    if K:
        keep = [j for j in range(Cm) if j not in set(pcol)]
        R2 = T2.shape[0]
        al[:, keep] = -T2[R2 - 1 - K:R2 - 1, :Cm - P]
    h.T, h.basis, h.ub, h.lo, h.flip = np.ascontiguousarray(T2), b2, ub2, lo2, flip2
    return src, pcol, al


def cut_loop(h, is_int, n_mask, first_cut_col, nint, node_is_int, o, flags, Rcap, Ccap, max_iter=10000, exprs=None):
    """lpx_bounded_cut_loop on a Handle, in place.  Returns the record as a dict (stop: a name of STOPS).  exprs: the affine
    expression (a, c) of every column in the unflipped, shifted structural variables y (column value = a.y + c) when the columns
    are unflipped; given, the dict also carries cuts: a list of (a, c) with a.y + c >= 1 for every cut ever added."""
    rec = {"rounds": 0, "added": 0, "purged": 0, "events": 0, "stop": "rounds", "status": L.OPTIMAL, "z_before": [], "z_after": [],
           "src_rows": [], "purged_cols": [], "traces": [], "cuts": []}
    pick = N.pick(h.T, h.basis, h.flip, h.ub, h.lo, nint, node_is_int, o.int_tol)

    def note(pcol, al):
        if exprs is None:
            return
        cur = []
        for j, (a, c) in enumerate(exprs):                  # the value of internal column j as it stands: flipped columns are ub - value
            cur.append((-a, h_ub[j] - c) if h_flip[j] else (a, c))
        new = [(sum((al[k, j] * cur[j][0] for j in range(len(cur))), np.zeros_like(exprs[0][0])),
                sum(al[k, j] * cur[j][1] for j in range(len(cur)) if al[k, j] != 0.0)) for k in range(len(al))]
        for p in sorted(pcol, reverse=True):
            del exprs[p]
        for a, c in new:
            rec["cuts"].append((a, c))
            exprs.append((a, c - 1.0))                      # the slack of the cut: a.y + c - 1

    while True:
        if pick["var"] < 0:
            rec["stop"] = "integral"
            break
        if rec["rounds"] >= o.max_rounds:
            rec["stop"] = "rounds"
            break
        h_ub, h_flip = h.ub.copy(), h.flip.copy()
        src, pcol, al = handle_round(h, is_int, n_mask, first_cut_col, o, Rcap, Ccap)
        note(pcol, al)
        rec["purged"] += len(pcol)
        rec["src_rows"].append(src); rec["purged_cols"].append(pcol)
        if not src:
            rec["stop"] = "stalled"
            break
        rec["added"] += len(src)
        z0 = pick["z"]
        nr = h.node2(np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0), nint, node_is_int, o.int_tol, flags | L.SKIP_FIXED, -INF,
                     max_iter=max_iter)
        assert nr["status"] is not None, "unrepairable column"
        rec["z_before"].append(z0); rec["z_after"].append(nr["z"])
        rec["rounds"] += 1; rec["events"] += nr["events"]; rec["status"] = nr["status"]
        rec["traces"].append(h.trace.copy())
        pick = {k: nr[k] for k in ("var", "candidates", "x_var", "z")}
        if nr["status"] == L.INFEASIBLE:
            rec["stop"] = "infeasible"
            break
        if nr["status"] == L.ITER_LIMIT:
            rec["stop"] = "iter_limit"
            break
        if nr["status"] != L.OPTIMAL:
            rec["stop"] = "status"
            break
    if o.purge and rec["stop"] in ("integral", "stalled", "rounds"):
        po = G.CutOpts(**vars(o)); po.cuts_per_round = 0
        h_ub, h_flip = h.ub.copy(), h.flip.copy()
        src, pcol, al = handle_round(h, is_int, n_mask, first_cut_col, po, Rcap, Ccap)
        note(pcol, al)
        rec["purged"] += len(pcol)
        rec["final_purge"] = pcol
    rec.update(pick)
    rec["R"], rec["C"] = h.T.shape
    return rec


def slack_mask(T0, n, is_int):
    """The round's flags [n + m] of a prepared model (T0 of _bnb_bounded_ref.prepare): the structural flags as given, and the slack
    of row i integer iff its coefficients and its shifted RHS are integral and every variable with a non-zero coefficient is integer."""
    m = T0.shape[0] - 1
    sint = np.ones(n, dtype=np.uint8) if is_int is None else (np.asarray(is_int) != 0).astype(np.uint8)
    out = np.zeros(n + m, dtype=np.uint8)
    out[:n] = sint
    for i in range(m):
        row, rhs = T0[i, :n], T0[i, -1]
        out[n + i] = 1 if (np.all(row == np.floor(row)) and rhs == np.floor(rhs) and np.all(sint[row != 0.0] != 0)) else 0
    return out


def spare(R, C, max_active):
    """The largest a <= max_active for which (R + a, C + a) fits the on-chip node."""
    a = max_active
    while a > 0 and not node_fits(R + a, C + a):
        a -= 1
    return a


def divers_from(hs, n, root_lo, root_ub, mask, W, max_nodes, max_iter, search_flags, out):
    """The diver loop of _bnb_divers_ref.solve_divers from the W handles hs (its own copy: that one starts from the model).
    Fills out and returns (best, best_x)."""
    cur = [(root_lo.copy(), root_ub.copy()) for _ in range(W)]
    stacks = [[] for _ in range(W)]
    stacks[0].append((0, []))
    best, best_x = -INF, None
    log, rounds, divers = [], [], []
    stop = False
    while not stop and any(stacks):
        if max_nodes > 0 and out["nodes"] >= max_nodes:
            out["rc"] = L.ITER_LIMIT
            break
        for d in range(W):
            if stacks[d]:
                continue
            v = max(range(W), key=lambda i: (len(stacks[i]), -i))
            if len(stacks[v]) >= 2:
                stacks[d].append(stacks[v].pop(0))
                out["steals"] += 1
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
            cols = np.flatnonzero((nb_lo != cur[d][0]) | (nb_ub != cur[d][1])).astype(np.int32)
            rec = hs[d].node2(cols, nb_lo[cols], nb_ub[cols], n, mask, EPS, L.SKIP_FIXED | search_flags, cutoff, max_iter=max_iter)
            assert rec["status"] is not None, "unrepairable column"
            recs.append((d, depth, path, nb_lo, nb_ub, len(cols), rec))
        rnd = out["rounds"]
        out["rounds"] += 1
        out["largest_batch"] = max(out["largest_batch"], len(recs))
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
            stacks[d].append((depth + 1, path + [(v, np.ceil(xv), nb_ub[v])]))
    out["log"] = np.array(log, dtype=N.LOG_DTYPE)
    out["round"] = np.array(rounds, dtype=np.int32)
    out["diver"] = np.array(divers, dtype=np.int32)
    return best, best_x


def clone(h):
    return L.Handle(h.T, h.basis, h.ub, h.flip, h.lo)


def solve_cuts(c, A, b, upper, W, root_cuts=None, lower=None, is_int=None, sense=0, max_nodes=0, max_iter=10000, rel=None,
               search_flags=0, want_cuts=False):
    """lpx_solve_bnb_bounded9.  root_cuts: a _gmi_ref.CutOpts or None (the search of _bnb_divers_ref.solve_divers).  Returns that
    search's dict (without critical_events) plus cut: the loop's record with spare and ran (None without root_cuts)."""
    assert W >= 1 and not search_flags & ~(L.LONG_STEP | L.CUTOFF_FLAG)
    T0, basis0, ub0, lower, is_min, shifted, constant = N.prepare(c, A, b, lower, upper, sense, rel)
    n = len(c)
    mask = None if is_int is None else np.asarray(is_int, dtype=np.uint8)
    st, Ts, bs, flip, _, _ = B.run(T0, basis0, ub0, max_iter=max_iter)
    out = {"rc": 0, "status": st, "x": None, "value": 0.0, "nodes": 0, "events": 0, "flips": 0, "incumbents": 0,
           "pruned_bound": 0, "pruned_infeasible": 0, "max_K": 0, "constant": constant, "rounds": 0, "steals": 0,
           "largest_batch": 0, "log": np.zeros(0, dtype=N.LOG_DTYPE), "round": np.zeros(0, dtype=np.int32),
           "diver": np.zeros(0, dtype=np.int32), "cut": None}
    if st != L.OPTIMAL:
        return out
    h = L.Handle(Ts, bs, ub0, flip)
    if root_cuts is not None:
        R, C = Ts.shape
        a = spare(R, C, root_cuts.max_active)
        cut = {"spare": a, "ran": 0}
        if a > 0:
            flags = slack_mask(T0, n, is_int)
            exprs = None
            if want_cuts:
                m = R - 1
                exprs = [(np.eye(n)[j], 0.0) for j in range(n)] + [(-T0[i, :n].copy(), float(T0[i, -1])) for i in range(m)]
            cut.update(cut_loop(h, flags, C - 1, C - 1, n, mask, root_cuts, search_flags, R + a, C + a, max_iter, exprs))
            cut["ran"] = 1
        out["cut"] = cut
        if cut["ran"] and cut["stop"] == "infeasible":
            out["status"] = L.INFEASIBLE
            return out
        if cut["ran"] and cut["stop"] == "iter_limit":
            out["rc"] = L.ITER_LIMIT
            out["status"] = L.INFEASIBLE
            return out
    hs = [h] + [clone(h) for _ in range(W - 1)]
    best, best_x = divers_from(hs, n, np.zeros(n), ub0[:n].copy(), mask, W, max_nodes, max_iter, search_flags, out)
    if best_x is None:
        out["status"] = L.INFEASIBLE
        return out
    x = best_x + lower if np.any(lower != 0.0) else best_x
    value = -best if is_min else best
    if shifted:
        value = value + constant
    out.update(status=L.OPTIMAL, x=x, value=float(value))
    return out
