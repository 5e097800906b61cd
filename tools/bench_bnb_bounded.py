"""Branch and bound to optimality, two ways on the device, on random 0/1 programs.

For each model -- synth.binary_ip(60, 12) and synth.binary_ip(128, 64) --
  (a) rows:    the bounds as explicit rows; the warm engine search BranchAndBound(bnb_mode=1, bnb_search=2, bnb_dive=1,
               concurrent_nodes=128): a new row and slack column per node, children assembled from parked parent tableaux
  (b) bounded: the bounds beside the tableau; LPSolver().SolveBnbBounded: one handle whose shape never changes, a node is a
               list of (column, lower, upper) triples (lpx_bounded_node)
Profiler off, both sides warm (two untimed solves each), the sides alternating, REPS timed solves.  A timed solve is the whole
call, model preparation and root solve included.  Prints one JSON line: per side the median / min / max milliseconds to
optimality and nodes/s, node counts and optima (the two searches must reach the same optimum; they follow different paths
through alternative optima, so the node counts may differ); for (b) the mean events per node, the wall microseconds per node,
and the wall microseconds of a K = 0 node call on the solved root -- the fixed cost of a node outside its events: five small
launches, one batch of the loop and three waits (host time outside the kernels proper needs a kernel trace and is not
collected here); and the device memory each side added (hipMemGetInfo through torch, read before the first solve and after
each side's first solve; handle caches keep what they allocated, so the reading after a solve is that side's peak).

`--model NAME` keeps one of the two models (bip_60x12, bip_128x64); `--max-nodes N` bounds both searches (then neither
reaches optimality and the optima are incumbents so far).  `--node-form launches|onchip|auto` is the node form of side (b)
and of its K = 0 node call (lpx_bounded_node3 / lpx_solve_bnb_bounded3; default launches).

`--compare-forms` measures the two node forms against each other instead: per model the wall of a K = 0
node call on the solved root and of the root's first child (200 calls a sample, REPS samples, the forms alternating), the
child's events, and the driver to optimality under `--flag-sets` (comma-separated out of plain,long_step,cutoff,both; default
all four) in both forms, alternating, REPS timed solves after one untimed solve of 2000 nodes each (`--flag-sets none`: no driver runs); counts must
be equal across forms.
`--compare-divers LIST` measures the search by W divers (lpx_solve_bnb_bounded4) against the single-diver
on-chip driver: per model and flag set (`--flag-sets`, default here plain,both) the on-chip driver and each W of the
comma-separated LIST alternate in one process, REPS timed solves each after one untimed solve; nodes, events, rounds, nodes/s
and wall per form, and `wins`: a W wins iff its median lies below the single-diver form's minimum.
`--divers W` makes side (b), and `--trace-only`, the search by W divers.
`--plunge D` makes them the plunge (lpx_solve_bnb_bounded5): up to D nodes per diver and launch; without
`--divers` it means one diver.
`--compare-plunge LIST` measures the plunge at the W of `--divers` (default 1) against the same search without it -- divers=W,
for W = 1 the sequential on-chip driver: per model and flag set the baseline and each D of the comma-separated LIST alternate
in one process, REPS timed solves each after one untimed solve; nodes, events, rounds, launched, dropped and wall per form, and
`wins`: a D wins iff its median lies below the baseline's minimum.  A search that ends at a node's event limit is reported
(`limit`) and not timed against.
`--compare-branching LIST` measures strong branching by probes (lpx_solve_bnb_bounded6) at the W of
`--divers` (default 1) against the most-fractional rule at the same W and flags: LIST is comma-separated settings C or C:L --
C candidates, probes of at most L events (no L: the node's limit); per model and flag set the baseline and each setting
alternate in one process, REPS timed solves each after one untimed solve; nodes, events, rounds, probes, probe events, children
pruned by a probe, changed picks and wall per side, and `wins`: a setting wins iff its median lies below the baseline's minimum.
`--branching R [--candidates C] [--probe-iter L]` makes side (b), and `--trace-only`, the search with that rule.
`--compare-guard LIST` measures the stall guard (lpx_solve_bnb_bounded7) at the W of `--divers` (default 1)
against the same search without it: LIST is comma-separated values of stall_events; per model and flag set the baseline
(divers=W, the kernels without the guard) and each S alternate in one process, REPS timed solves each after one untimed solve;
nodes, events, rounds, guarded nodes, Bland pivots, the most events of one node and wall per side, `ratio` (median over the
baseline's median) and `limit` where a search ends at a node's event limit (reported, not timed against).  Beside the two
binary_ip models it knows bip_40x16_s6, synth.binary_ip(40, 16, seed=6), whose plain search by one diver meets a cycling node.
`--stall-events S` makes side (b), and `--trace-only`, the search with the guard.
`--trace-only` runs one solve of side (b) and nothing else (for a kernel trace of the node form given).

usage: bench_bnb_bounded.py [--model NAME] [--max-nodes N] [--node-form F] [--divers W] [--plunge D]
                            [--compare-forms [--flag-sets LIST]] [--compare-divers LIST [--flag-sets LIST]]
                            [--compare-plunge LIST [--flag-sets LIST]] [--compare-branching LIST [--flag-sets LIST]]
                            [--branching R [--candidates C] [--probe-iter L]] [--compare-guard LIST [--flag-sets LIST]]
                            [--stall-events S] [--long-step] [--cutoff] [--trace-only] [--compare-root LIST]
                            [--compare-cuts [LIST] [--rounds LIST] [--cuts-per-round K]]
                            [--compare-tighten [LIST] [--flag-sets LIST]] [REPS]

`--compare-root LIST` measures the form of the root solve (lpx_solve_bnb_bounded8) at every W of LIST, with the
long step and the cutoff: root_form "launches" against "onchip", the sides alternating, one untimed solve each first.  Beside the
search it times the root solve alone in either form (lpx_solve_bounded / lpx_solve_bounded2) and reports its share of the search's
wall on both sides.  A side wins iff its median lies below the other's minimum.

`--compare-cuts [LIST]` measures cut-and-branch at the root (lpx_solve_bnb_bounded9) at every W of LIST (default
1,16,256), with the long step and the cutoff: the search with N rounds of K GMI cuts at the root, N over `--rounds` (default 2,4,8) and
K = `--cuts-per-round` (default 8), against the same search without cuts (lpx_solve_bnb_bounded8, root_form "launches") in the same
process, the settings alternating, one untimed solve each first.  Per setting: nodes, wall to optimality, the cut counts and the shape
the search runs on.  A setting wins iff its median lies below the baseline's minimum, and loses iff the baseline's median lies below
its minimum.  Beside the searches it times lpx_bounded_cut_loop alone on the solved root in both node forms (the handle is put back
from a snapshot between the runs) and checks that the two forms leave the same record.  No ratio is expected in advance: whether the
tree shrinks depends on the model.

`--compare-tighten [LIST]` measures reduced-cost bound tightening (lpx_solve_bnb_bounded10) at every W of LIST
(default 1,16,256) and every flag set of `--flag-sets` (default plain,both): the search with tighten=True against the same binary
with tighten = 0 (root_form "launches", by contract lpx_solve_bnb_bounded9 without cuts), the sides alternating in one process, one
untimed solve each first, REPS (default 7) timed solves each.  Per side: nodes, events, rounds, the three counters and wall as
median (min-max); the tightening wins iff its median lies below the baseline's minimum and loses iff the baseline's median lies
below its minimum.  A side that ends at a node's event limit is reported (`limit`) and not timed against.  Beside the searches it times one node call with K = 0 on the solved root in three kernels -- lpx_bounded_node4
with stall_events = 0 (the node kernel, its record a kernel argument), with a stall_events it never reaches (the guarded kernel,
its record read from pinned memory) and lpx_bounded_node5 with a fix_bound so far below z that the step runs and tightens nothing
(the guarded kernel's shape plus the step).  No
speed-up is expected in advance: at large W the tighter bounds arrive a round late.

`--compare-packed [--flag-sets NAME] [REPS]` measures the packed branch and bound (lpx_solve_packed_bnb): 256
and 4096 right-hand sides of one 9 x 29 binary model as ONE SolvePackedBnb call against the same models as single
SolveBnbBounded(node_form="onchip") calls, host wall of whole calls, the sides alternating in one process, one untimed round first,
REPS (default 7; 2 at 4096) timed rounds, the results asserted equal; then one model alone against the sequential driver and
divers=4,16,64; then binary_ip(60, 12) alone against the sequential on-chip driver, as time per node.  A side wins iff its median lies
below the other's minimum.  `--packed-trace` makes four packed calls and the binary_ip(60, 12) call for a kernel trace.

`--compare-packed-dual [--flag-sets NAME] [REPS]` measures the packed branch and bound from a dual start
(lpx_solve_packed_bnb_dual) the same way: 256 and 4096 right-hand sides of one 8 x 16 covering model (Min c.x,
A x >= b over binaries) as ONE SolvePackedBnbDual call against the same models as single SolveBnbBoundedDual(node_form="onchip")
calls, the results asserted equal; then, on the <= family of --compare-packed, which both packed calls accept, SolvePackedBnbDual
against SolvePackedBnb: what the dual root costs or saves where the primal one would do.  No time or ratio is promised."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import linear_programming_solver_lpr381_amd as L
from linear_programming_solver_lpr381_amd import synth


def models():
    yield "bip_60x12", 60, 12
    yield "bip_128x64", 128, 64


def stats(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "samples": len(ts)} if ts else None


def device_used_mb():
    try:
        import torch
        free, total = torch.cuda.mem_get_info()
        return (total - free) / 2 ** 20
    except Exception:
        return None


FORMS = ("launches", "onchip")
FLAG_SETS = {"plain": {}, "long_step": {"long_step": True}, "cutoff": {"cutoff": True}, "both": {"long_step": True, "cutoff": True}}


def compare_forms(n, m, reps, max_nodes, flag_sets):
    """The two node forms against each other on binary_ip(n, m): node call wall and the driver (see the module docstring)."""
    c, A, rel, b = synth.binary_ip(n, m)
    bnd_p = L.LPProblem.from_arrays(0, c, A[:m], rel[:m], b[:m])
    rec = {"n": n, "m": m, "bounded_shape": [m + 1, n + m + 1], "node_call_us": {}, "driver": {}}
    T, basis = synth.primal_tableau_from(c, A[:m], b[:m])
    ub = np.full(T.shape[1] - 1, np.inf); ub[:n] = 1.0
    calls = 200
    with L.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        dt.bounded_run()
        dt.snapshot()
        rec["fits"] = dt.bounded_node_fits()
        root = dt.bounded_node([], [], [], n, batch=16)
        j = root["var"]
        child = None
        for what, edit in (("empty", ([], [], [])), ("child", ([j], [1.0], [1.0]))):
            ts = {f: [] for f in FORMS}
            for i in range(reps + 1):
                for f in FORMS:
                    total = 0.0
                    for _ in range(calls):
                        if what == "child":
                            dt.restore()
                        t0 = time.perf_counter()
                        got = dt.bounded_node(*edit, n, batch=16, form=f)
                        total += time.perf_counter() - t0
                    if what == "child":
                        assert child is None or child == got, "the forms disagree on the child"
                        child = got
                    if i >= 1:
                        ts[f].append(1e6 * total / calls)
            rec["node_call_us"][what] = {f: stats(ts[f]) for f in FORMS}
        rec["child"] = {"var": j, "events": child["events"], "status": child["status"]}
        ev = max(1, child["events"])
        rec["us_per_event"] = {f: (rec["node_call_us"]["child"][f]["median"] - rec["node_call_us"]["empty"][f]["median"]) / ev for f in FORMS}

    def solve(f, kw, limit=None):
        limit = max_nodes if limit is None else limit
        t0 = time.perf_counter()
        try:
            r = L.LPSolver().SolveBnbBounded(bnd_p, 1.0, max_nodes=limit, node_form=f, **kw)
        except L.SolverException as e:
            if e.code != L._lib.ITER_LIMIT or not limit:
                raise
            r = e.result
        return 1e3 * (time.perf_counter() - t0), r

    for fs in flag_sets:
        kw = FLAG_SETS[fs]
        ts = {f: [] for f in FORMS}
        last = {}
        for i in range(reps + 1):
            for f in FORMS:
                if i == 0:          # the untimed solve: what a first solve pays once is paid within its first nodes
                    solve(f, kw, max_nodes if max_nodes else 2000)
                    continue
                ms, r = solve(f, kw)
                last[f] = r
                ts[f].append(ms)
        a, o = last["launches"], last["onchip"]
        d = {f: {"ms": stats(ts[f]), "nodes_per_s": a.Nodes / (statistics.median(ts[f]) / 1e3)} for f in FORMS}
        d.update(nodes=int(a.Nodes), events=a.BnbInfo["events"], pruned_bound=a.BnbInfo["pruned_bound"],
                 counts_equal=bool(a.BnbLog.tobytes() == o.BnbLog.tobytes() and a.BnbInfo == o.BnbInfo),
                 onchip_wins=bool(d["onchip"]["ms"]["median"] < d["launches"]["ms"]["min"]),
                 launches_wins=bool(d["launches"]["ms"]["median"] < d["onchip"]["ms"]["min"]))
        rec["driver"][fs] = d
    return rec


def compare_divers(n, m, reps, max_nodes, flag_sets, widths):
    """The search by W divers against the single-diver on-chip driver on binary_ip(n, m) (see the module docstring)."""
    c, A, rel, b = synth.binary_ip(n, m)
    bnd_p = L.LPProblem.from_arrays(0, c, A[:m], rel[:m], b[:m])
    rec = {"n": n, "m": m, "bounded_shape": [m + 1, n + m + 1]}
    sides = ["onchip"] + [f"W{w}" for w in widths]

    def solve(side, kw, limit=None):
        limit = max_nodes if limit is None else limit
        how = {"node_form": "onchip"} if side == "onchip" else {"divers": int(side[1:])}
        t0 = time.perf_counter()
        try:
            r = L.LPSolver().SolveBnbBounded(bnd_p, 1.0, max_nodes=limit, **how, **kw)
            r.Limit = None
        except L.SolverException as e:
            if e.code != L._lib.ITER_LIMIT:
                raise
            r = e.result
            r.Limit = None if limit and r.Nodes >= limit else str(e)      # a node at its event limit ends the solve: reported, not timed against
        return 1e3 * (time.perf_counter() - t0), r

    for fs in flag_sets:
        kw = FLAG_SETS[fs]
        ts = {s: [] for s in sides}
        last = {}
        for i in range(reps + 1):
            for s in sides:
                if i == 0:          # the untimed solve: clones, the batch's slab and the first launch are paid here
                    solve(s, kw, max_nodes if max_nodes else 2000)
                    continue
                ms, r = solve(s, kw)
                last[s] = r
                ts[s].append(ms)
        base = stats(ts["onchip"])
        d = {}
        for s in sides:
            r = last[s]
            st = stats(ts[s])
            d[s] = {"ms": st, "nodes": int(r.Nodes), "events": r.BnbInfo["events"], "rounds": r.BnbInfo.get("rounds", int(r.Nodes)),
                    "steals": r.BnbInfo.get("steals", 0), "largest_batch": r.BnbInfo.get("largest_batch", 1),
                    "nodes_per_s": r.Nodes / (st["median"] / 1e3), "optimum": r.OptimalValue, "limit": r.Limit,
                    "wins": bool(s != "onchip" and r.Limit is None and st["median"] < base["min"])}
        rec[fs] = d
    return rec


def compare_plunge(n, m, reps, max_nodes, flag_sets, W, depths):
    """The plunge (lpx_solve_bnb_bounded5) at W divers against the same search without it on binary_ip(n, m): the baseline is
    divers=W, for W = 1 the sequential on-chip driver (see the module docstring)."""
    c, A, rel, b = synth.binary_ip(n, m)
    bnd_p = L.LPProblem.from_arrays(0, c, A[:m], rel[:m], b[:m])
    rec = {"n": n, "m": m, "bounded_shape": [m + 1, n + m + 1], "divers": W}
    sides = ["base"] + [f"D{d}" for d in depths]

    def solve(side, kw, limit=None):
        limit = max_nodes if limit is None else limit
        if side != "base":
            how = {"divers": W, "plunge": int(side[1:])}
        else:
            how = {"node_form": "onchip"} if W == 1 else {"divers": W}
        t0 = time.perf_counter()
        try:
            r = L.LPSolver().SolveBnbBounded(bnd_p, 1.0, max_nodes=limit, **how, **kw)
            r.Limit = None
        except L.SolverException as e:
            if e.code != L._lib.ITER_LIMIT:
                raise
            r = e.result
            r.Limit = None if limit and r.Nodes >= limit else str(e)      # a node at its event limit ends the solve: reported, not timed against
        return 1e3 * (time.perf_counter() - t0), r

    for fs in flag_sets:
        kw = FLAG_SETS[fs]
        ts = {s: [] for s in sides}
        last = {}
        for i in range(reps + 1):
            for s in sides:
                if i == 0:          # the untimed solve: clones, the batch's slab and the first launch are paid here
                    solve(s, kw, max_nodes if max_nodes else 2000)
                    continue
                ms, r = solve(s, kw)
                last[s] = r
                ts[s].append(ms)
        base = stats(ts["base"])
        d = {}
        for s in sides:
            r = last[s]
            st = stats(ts[s])
            d[s] = {"ms": st, "nodes": int(r.Nodes), "events": r.BnbInfo["events"], "rounds": r.BnbInfo.get("rounds", int(r.Nodes)),
                    "launched": r.BnbInfo.get("launched", int(r.Nodes)), "dropped": r.BnbInfo.get("dropped", 0),
                    "longest_chain": r.BnbInfo.get("longest_chain", 1), "nodes_per_s": r.Nodes / (st["median"] / 1e3),
                    "optimum": r.OptimalValue, "limit": r.Limit,
                    "wins": bool(s != "base" and r.Limit is None and last["base"].Limit is None and st["median"] < base["min"])}
        rec[fs] = d
    return rec


def compare_branching(n, m, reps, max_nodes, flag_sets, W, settings):
    """Strong branching (lpx_solve_bnb_bounded6) at W divers against the most-fractional rule at the same W on binary_ip(n, m)
    (see the module docstring).  settings: (candidates, probe_iter or None)."""
    c, A, rel, b = synth.binary_ip(n, m)
    bnd_p = L.LPProblem.from_arrays(0, c, A[:m], rel[:m], b[:m])
    rec = {"n": n, "m": m, "bounded_shape": [m + 1, n + m + 1], "divers": W}
    sides = {"base": None}
    for cand, limit in settings:
        sides[f"C{cand}" + ("" if limit is None else f"L{limit}")] = (cand, limit)

    def solve(side, kw, limit=None):
        limit = max_nodes if limit is None else limit
        how = {"divers": W, "branching": "most_fractional"}
        if sides[side] is not None:
            how = {"divers": W, "branching": "strong", "candidates": sides[side][0], "probe_iter": sides[side][1]}
        t0 = time.perf_counter()
        try:
            r = L.LPSolver().SolveBnbBounded(bnd_p, 1.0, max_nodes=limit, **how, **kw)
            r.Limit = None
        except L.SolverException as e:
            if e.code != L._lib.ITER_LIMIT:
                raise
            r = e.result
            r.Limit = None if limit and r.Nodes >= limit else str(e)      # a node at its event limit ends the solve: reported, not timed against
        return 1e3 * (time.perf_counter() - t0), r

    for fs in flag_sets:
        kw = FLAG_SETS[fs]
        ts = {s: [] for s in sides}
        last = {}
        for i in range(reps + 1):
            for s in sides:
                if i == 0:          # the untimed solve: clones, the batch's slab and workspace and the first launches are paid here
                    solve(s, kw, max_nodes if max_nodes else 2000)
                    continue
                ms, r = solve(s, kw)
                last[s] = r
                ts[s].append(ms)
        base = stats(ts["base"])
        d = {}
        for s in sides:
            r = last[s]
            st = stats(ts[s])
            d[s] = {"ms": st, "nodes": int(r.Nodes), "events": r.BnbInfo["events"], "rounds": r.BnbInfo["rounds"],
                    "probes": r.BnbInfo["probes"], "probe_events": r.BnbInfo["probe_events"], "probe_limit": r.BnbInfo["probe_limit"],
                    "pruned_by_probe": r.BnbInfo["pruned_by_probe"], "changed_picks": r.BnbInfo["changed_picks"],
                    "nodes_per_s": r.Nodes / (st["median"] / 1e3), "optimum": r.OptimalValue, "limit": r.Limit,
                    "wins": bool(s != "base" and r.Limit is None and last["base"].Limit is None and st["median"] < base["min"])}
        rec[fs] = d
    return rec


def compare_guard(n, m, reps, max_nodes, flag_sets, W, stalls, seed=None):
    """The stall guard (lpx_solve_bnb_bounded7) at W divers against the same search without it (lpx_solve_bnb_bounded4) on
    binary_ip(n, m) (see the module docstring)."""
    c, A, rel, b = synth.binary_ip(n, m) if seed is None else synth.binary_ip(n, m, seed)
    bnd_p = L.LPProblem.from_arrays(0, c, A[:m], rel[:m], b[:m])
    rec = {"n": n, "m": m, "bounded_shape": [m + 1, n + m + 1], "divers": W}
    sides = {"base": None}
    for S in stalls:
        sides[f"S{S}"] = S

    def solve(side, kw, limit=None):
        limit = max_nodes if limit is None else limit
        how = {"divers": W} if sides[side] is None else {"divers": W, "stall_events": sides[side]}
        t0 = time.perf_counter()
        try:
            r = L.LPSolver().SolveBnbBounded(bnd_p, 1.0, max_nodes=limit, **how, **kw)
            r.Limit = None
        except L.SolverException as e:
            if e.code != L._lib.ITER_LIMIT:
                raise
            r = e.result
            r.Limit = None if limit and r.Nodes >= limit else str(e)      # a node at its event limit ends the solve: reported, not timed against
        return 1e3 * (time.perf_counter() - t0), r

    for fs in flag_sets:
        kw = FLAG_SETS[fs]
        ts = {s: [] for s in sides}
        last = {}
        for i in range(reps + 1):
            for s in sides:
                if i == 0:          # the untimed solve: clones, the batch's slab and the first launch of either kernel are paid here
                    solve(s, kw, max_nodes if max_nodes else 2000)
                    continue
                ms, r = solve(s, kw)
                last[s] = r
                ts[s].append(ms)
        base = stats(ts["base"])
        d = {}
        for s in sides:
            r = last[s]
            st = stats(ts[s])
            d[s] = {"ms": st, "nodes": int(r.Nodes), "events": r.BnbInfo["events"], "rounds": r.BnbInfo["rounds"],
                    "guarded_nodes": r.BnbInfo.get("guarded_nodes", 0), "bland_events": r.BnbInfo.get("bland_events", 0),
                    "max_events": r.BnbInfo.get("max_events", int(r.BnbLog["events"].max()) if len(r.BnbLog) else 0),
                    "nodes_per_s": r.Nodes / (st["median"] / 1e3), "optimum": r.OptimalValue, "limit": r.Limit,
                    "ratio": None if last["base"].Limit is not None or r.Limit is not None else st["median"] / base["median"]}
        rec[fs] = d
    return rec


def compare_root(n, m, reps, max_nodes, widths):
    """The root solve's form (lpx_solve_bnb_bounded8) at W divers on binary_ip(n, m), long step and cutoff (see the module docstring)."""
    c, A, rel, b = synth.binary_ip(n, m)
    p = L.LPProblem.from_arrays(0, c, A[:m], rel[:m], b[:m])
    rec = {"n": n, "m": m, "bounded_shape": [m + 1, n + m + 1]}
    root = {f: [] for f in FORMS}
    for i in range(reps + 2):
        for f in FORMS:
            t0 = time.perf_counter()
            r = L.LPSolver().SolveBounded(p, 1.0, form=f)
            if i >= 2:
                root[f].append(1e3 * (time.perf_counter() - t0))
    rec["root_alone_ms"] = {f: stats(root[f]) for f in FORMS}
    rec["root_events"] = int(sum(r.BoundCounts))

    def solve(W, f):
        t0 = time.perf_counter()
        try:
            r = L.LPSolver().SolveBnbBounded(p, 1.0, max_nodes=max_nodes, divers=W, root_form=f, long_step=True, cutoff=True)
            r.Limit = None
        except L.SolverException as e:
            if e.code != L._lib.ITER_LIMIT:
                raise
            r = e.result
            r.Limit = str(e)
        return 1e3 * (time.perf_counter() - t0), r

    for W in widths:
        ts = {f: [] for f in FORMS}
        last = {}
        for i in range(reps + 1):
            for f in FORMS:
                ms, r = solve(W, f)
                if i >= 1:
                    ts[f].append(ms)
                last[f] = r
        assert last["launches"].BnbLog.tobytes() == last["onchip"].BnbLog.tobytes(), "the node logs differ"
        d = {}
        for f in FORMS:
            st = stats(ts[f])
            d[f] = {"ms": st, "nodes": int(last[f].Nodes), "limit": last[f].Limit,
                    "root_share": rec["root_alone_ms"][f]["median"] / st["median"]}
        a, o = d["launches"]["ms"], d["onchip"]["ms"]
        d["winner"] = "onchip" if o["median"] < a["min"] else "launches" if a["median"] < o["min"] else "tie"
        rec[f"W{W}"] = d
    return rec


def compare_cuts(n, m, reps, max_nodes, widths, rounds, K, max_active=64):
    """Cut-and-branch at the root (lpx_solve_bnb_bounded9) against the search without cuts on binary_ip(n, m) (see the module docstring)."""
    c, A, rel, b = synth.binary_ip(n, m)
    p = L.LPProblem.from_arrays(0, c, A[:m], rel[:m], b[:m])
    rec = {"n": n, "m": m, "bounded_shape": [m + 1, n + m + 1], "cuts_per_round": K, "max_active": max_active}

    # the loop alone, on the solved root, in both node forms
    T, basis = synth.primal_tableau_from(c, A[:m], b[:m])
    R, C_ = T.shape
    ub = np.full(C_ - 1, np.inf); ub[:n] = 1.0
    spare = max_active
    while spare > 0 and not L._lib.lib().lpx_bounded_node_fits(R + spare, C_ + spare):
        spare -= 1
    rec["spare"] = spare
    flags = np.zeros(C_ - 1, dtype=np.uint8); flags[:n] = 1
    for i in range(m):
        flags[n + i] = 1 if (np.all(T[i, :n] == np.floor(T[i, :n])) and T[i, -1] == np.floor(T[i, -1])) else 0
    loop = {}
    if spare > 0:
        with L.DeviceTableau.with_capacity(T, basis, R + spare, C_ + spare) as dt:
            dt.set_bounds(ub)
            dt.bounded_run()
            dt.snapshot()
            for N in rounds:
                ts, last = {f: [] for f in FORMS}, {}
                for i in range(reps + 1):
                    for f in FORMS:
                        dt.set_shape(R, C_)
                        dt.restore()
                        t0 = time.perf_counter()
                        r = dt.cut_loop(flags, C_ - 1, n, cuts_per_round=K, max_rounds=N, max_active=max_active, long_step=True,
                                        cutoff=True, form=f)
                        if i >= 1:
                            ts[f].append(1e3 * (time.perf_counter() - t0))
                        last[f] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in r.items()}
                assert last["launches"] == last["onchip"], "the two forms of the loop leave different records"
                loop[f"rounds{N}"] = {"ms": {f: stats(ts[f]) for f in FORMS}, "record": {k: last["onchip"][k] for k in
                                      ("rounds", "added", "purged", "events", "stop", "R", "C")}, "z": [last["onchip"]["z_before"][:1],
                                      last["onchip"]["z_after"]]}
    rec["loop_alone"] = loop

    def solve(W, N):
        kw = dict(root_cuts=N, cuts_per_round=K, max_active=max_active) if N else dict(root_form="launches")
        t0 = time.perf_counter()
        try:
            r = L.LPSolver().SolveBnbBounded(p, 1.0, max_nodes=max_nodes, divers=W, long_step=True, cutoff=True, **kw)
            r.Limit = None
        except L.SolverException as e:
            if e.code != L._lib.ITER_LIMIT:
                raise
            r = e.result
            r.Limit = str(e)
        return 1e3 * (time.perf_counter() - t0), r

    settings = [0] + [N for N in rounds if N]
    for W in widths:
        ts, last = {N: [] for N in settings}, {}
        for i in range(reps + 1):
            for N in settings:
                ms, r = solve(W, N)
                if i >= 1:
                    ts[N].append(ms)
                last[N] = r
        d = {}
        base = stats(ts[0])
        for N in settings:
            st, r = stats(ts[N]), last[N]
            e = {"ms": st, "nodes": int(r.Nodes), "value": float(r.OptimalValue), "limit": r.Limit}
            if N:
                bi = r.BnbInfo
                e.update(cut_rounds=bi["cut_rounds"], cuts_added=bi["cuts_added"], cuts_purged=bi["cuts_purged"], cut_stop=bi["cut_stop"],
                         shape=[bi["cut_R"], bi["cut_C"]], nodes_vs_baseline=r.Nodes / max(last[0].Nodes, 1),
                         wall_vs_baseline=st["median"] / base["median"],
                         verdict="win" if st["median"] < base["min"] else "loss" if base["median"] < st["min"] else "tie")
                assert r.Limit or last[0].Limit or abs(r.OptimalValue - last[0].OptimalValue) <= 1e-9 * abs(last[0].OptimalValue), "optimum differs"
            d["baseline" if not N else f"rounds{N}"] = e
        rec[f"W{W}"] = d
    return rec


def compare_tighten(n, m, reps, max_nodes, flag_sets, widths):
    """Reduced-cost tightening (lpx_solve_bnb_bounded10) against the same search without it on binary_ip(n, m) (see the module docstring)."""
    c, A, rel, b = synth.binary_ip(n, m)
    p = L.LPProblem.from_arrays(0, c, A[:m], rel[:m], b[:m])
    rec = {"n": n, "m": m, "bounded_shape": [m + 1, n + m + 1]}

    # one node call with K = 0 on the solved root: the node kernel against the kernel with the step, which tightens nothing
    T, basis = synth.primal_tableau_from(c, A[:m], b[:m])
    ub = np.full(T.shape[1] - 1, np.inf); ub[:n] = 1.0
    none = (np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0))
    with L.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        dt.bounded_run()
        z = dt.bounded_node(*none, n, form="onchip")["z"]
        # node4_guard: the guarded kernel with a threshold it never reaches -- batch-shaped like the kernel with the step, its
        # parameter record read from pinned host memory, so node5 against it is the step alone
        calls = {"node4": dict(stall_events=0), "node4_guard": dict(stall_events=1000000), "node5": dict(fix_bound=z - 1e9)}
        ts = {k: [] for k in calls}
        fixed = 0
        for i in range(40 * (reps + 1)):
            for k, kw in calls.items():
                t0 = time.perf_counter()
                r = dt.bounded_node(*none, n, form="onchip", **kw)
                if i >= 40:
                    ts[k].append(1e6 * (time.perf_counter() - t0))
                if k == "node5":
                    fixed += len(r["fixed"][0])
        assert fixed == 0, "the timed node call tightened a column"
        rec["node_call_us"] = {k: stats(ts[k]) for k in calls}

    def solve(W, side, kw):
        how = dict(tighten=True) if side == "tighten" else dict(root_form="launches")
        t0 = time.perf_counter()
        try:
            r = L.LPSolver().SolveBnbBounded(p, 1.0, max_nodes=max_nodes, divers=W, **how, **kw)
            r.Limit = None
        except L.SolverException as e:
            if e.code != L._lib.ITER_LIMIT:
                raise
            r = e.result
            r.Limit = None if max_nodes and r.Nodes >= max_nodes else str(e)
        return 1e3 * (time.perf_counter() - t0), r

    sides = ("base", "tighten")
    for fs in flag_sets:
        kw = FLAG_SETS[fs]
        for W in widths:
            ts, last = {s: [] for s in sides}, {}
            for i in range(reps + 1):
                for s in sides:
                    ms, r = solve(W, s, kw)
                    if i >= 1:
                        ts[s].append(ms)
                    last[s] = r
            d = {}
            for s in sides:
                st, r = stats(ts[s]), last[s]
                d[s] = {"ms": st, "nodes": int(r.Nodes), "events": r.BnbInfo["events"], "rounds": r.BnbInfo["rounds"],
                        "max_K": r.BnbInfo["max_K"], "tightened_nodes": r.BnbInfo.get("tightened_nodes", 0),
                        "tightened_cols": r.BnbInfo.get("tightened_cols", 0), "max_per_node": r.BnbInfo.get("max_per_node", 0),
                        "optimum": float(r.OptimalValue), "limit": r.Limit}
            a, t = d["base"]["ms"], d["tighten"]["ms"]
            limited = last["base"].Limit is not None or last["tighten"].Limit is not None     # a side that ended at a node's event limit: reported, not timed against
            d["ratio"] = None if limited else t["median"] / a["median"]
            d["verdict"] = "limit" if limited else "win" if t["median"] < a["min"] else "loss" if a["median"] < t["min"] else "tie"
            if not (last["base"].Limit or last["tighten"].Limit or max_nodes):
                assert abs(d["base"]["optimum"] - d["tighten"]["optimum"]) <= 1e-9 * abs(d["base"]["optimum"]), "optimum differs"
            rec[f"{fs}_W{W}"] = d
    return rec


def rhs_family(n, m, count, seed=5):
    """count right-hand sides of ONE binary model of n variables and m rows (synth.binary_ip's rows): b_i scaled by U(0.8, 1.2),
    floored, plus 0.5 -- (c, A [m, n], bs [count, m])."""
    c, A, _, b = synth.binary_ip(n, m, seed)
    g = np.random.default_rng(seed)
    bs = np.floor(b[:m] * g.uniform(0.8, 1.2, size=(count, m))) + 0.5
    return c, np.ascontiguousarray(A[:m]), bs


def compare_packed(reps, counts, big_reps, widths, kw_name="plain"):
    """The packed branch and bound (lpx_solve_packed_bnb) against the same models as single
    SolveBnbBounded(node_form="onchip") calls: host wall of whole calls, the sides alternating in one process, one untimed round
    first.  Then, on one model, the best of divers=W; then binary_ip(60, 12) alone against the sequential on-chip driver."""
    S = L.LPSolver()
    kw = FLAG_SETS[kw_name]
    out = {"flags": kw_name, "families": {}}
    n, m = 20, 8
    for count in counts:
        c, A, bs = rhs_family(n, m, count)
        probs = [L.LPProblem.from_arrays(0, c, A, [0] * m, bs[i]) for i in range(count)]
        r = big_reps if count > 1024 else reps
        ts = {"packed": [], "single": []}
        for i in range(r + 1):
            t0 = time.perf_counter()
            pk = S.SolvePackedBnb(c, A, bs, 1.0, **kw)
            t1 = time.perf_counter()
            ones = [S.SolveBnbBounded(p, 1.0, node_form="onchip", **kw) for p in probs]
            t2 = time.perf_counter()
            if i >= 1:
                ts["packed"].append(1e3 * (t1 - t0)); ts["single"].append(1e3 * (t2 - t1))
        assert pk.Status.tolist() == [o.Status for o in ones] and (pk.Stop == 0).all()
        assert pk.Nodes.tolist() == [o.Nodes for o in ones]
        assert all(np.array_equal(pk.Solution[i], o.Solution) and pk.OptimalValue[i] == o.OptimalValue for i, o in enumerate(ones))
        d = {k: stats(v) for k, v in ts.items()}
        d.update(count=count, shape=[m + 1, n + m + 1], nodes=int(pk.Nodes.sum()), events=int(pk.Info["events"].sum()),
                 max_nodes_of_a_model=int(pk.Nodes.max()), deepest=int(pk.Info["deepest"].max()),
                 kernel_ms=pk.Stats["loop_ms"], us_per_node_packed=1e3 * statistics.median(ts["packed"]) / int(pk.Nodes.sum()),
                 us_per_node_single=1e3 * statistics.median(ts["single"]) / int(pk.Nodes.sum()),
                 packed_wins=bool(d["packed"]["median"] < d["single"]["min"]), single_wins=bool(d["single"]["median"] < d["packed"]["min"]))
        out["families"][str(count)] = d
    # one model: the packed call (count = 1) against the sequential driver and the divers
    c, A, bs = rhs_family(n, m, 1)
    p = L.LPProblem.from_arrays(0, c, A, [0] * m, bs[0])
    sides = {"packed": lambda: S.SolvePackedBnb(c, A, bs, 1.0, **kw), "onchip": lambda: S.SolveBnbBounded(p, 1.0, node_form="onchip", **kw)}
    for W in widths:
        sides["divers=%d" % W] = (lambda W=W: S.SolveBnbBounded(p, 1.0, divers=W, **kw))
    out["one_model"] = alternate(sides, reps)
    # binary_ip(60, 12) alone: ONE workgroup, every node in the one launch
    c, A, rel, b = synth.binary_ip(60, 12)
    A12, b12 = np.ascontiguousarray(A[:12]), b[:12]
    p = L.LPProblem.from_arrays(0, c, A12, [0] * 12, b12)
    sides = {"packed": lambda: S.SolvePackedBnb(c, A12, b12, 1.0, max_nodes=1000000, max_events=100000000, **kw),
             "onchip": lambda: S.SolveBnbBounded(p, 1.0, node_form="onchip", **kw)}
    d = alternate(sides, reps)
    pk, one = sides["packed"](), sides["onchip"]()
    assert pk.Status[0] == one.Status and pk.Nodes[0] == one.Nodes and pk.OptimalValue[0] == one.OptimalValue
    d.update(nodes=int(pk.Nodes[0]), events=int(pk.Info["events"][0]), deepest=int(pk.Info["deepest"][0]),
             us_per_node_packed=1e3 * d["packed"]["median"] / int(pk.Nodes[0]), us_per_node_onchip=1e3 * d["onchip"]["median"] / int(pk.Nodes[0]))
    out["bip_60x12"] = d
    return out


def cover_family(m, n, count, seed=3):
    """count right-hand sides of ONE covering model (Min c.x, A x >= b, binaries): A = integers(1, 9), c = integers(1, 12),
    b_i = floor(U(0.3, 0.5) rowsum) -- (c, A [m, n], bs [count, m])."""
    g = np.random.default_rng(seed)
    A = g.integers(1, 9, (m, n)).astype(np.float64)
    c = g.integers(1, 12, n).astype(np.float64)
    bs = np.floor(A.sum(axis=1) * g.uniform(0.3, 0.5, size=(count, m)))
    return c, A, bs


def compare_packed_dual(reps, counts, big_reps, kw_name="plain"):
    """The packed branch and bound from a dual start (lpx_solve_packed_bnb_dual) against the same covering
    models as single SolveBnbBoundedDual(node_form="onchip") calls, as compare_packed measures; then against SolvePackedBnb on a
    family of <= models that both accept."""
    S = L.LPSolver()
    kw = FLAG_SETS[kw_name]
    out = {"flags": kw_name, "families": {}}
    m, n = 8, 16
    rel = np.ones(m, dtype=np.int32)
    for count in counts:
        c, A, bs = cover_family(m, n, count)
        probs = [L.LPProblem.from_arrays(1, c, A, [1] * m, bs[i]) for i in range(count)]
        r = big_reps if count > 1024 else reps
        ts = {"packed": [], "single": []}
        for i in range(r + 1):
            t0 = time.perf_counter()
            pk = S.SolvePackedBnbDual(c, A, bs, rel, 1.0, sense="min", **kw)
            t1 = time.perf_counter()
            ones = [S.SolveBnbBoundedDual(p, 1.0, node_form="onchip", **kw) for p in probs]
            t2 = time.perf_counter()
            if i >= 1:
                ts["packed"].append(1e3 * (t1 - t0)); ts["single"].append(1e3 * (t2 - t1))
        assert pk.Status.tolist() == [o.Status for o in ones] and (pk.Stop <= 1).all()
        assert pk.Nodes.tolist() == [o.Nodes for o in ones]
        assert all(pk.OptimalValue[i] == o.OptimalValue and (o.Status != 0 or np.array_equal(pk.Solution[i], o.Solution))
                   for i, o in enumerate(ones))
        nodes = max(1, int(pk.Nodes.sum()))
        d = {k: stats(v) for k, v in ts.items()}
        d.update(count=count, shape=[m + 1, n + m + 1], nodes=int(pk.Nodes.sum()), events=int(pk.Info["events"].sum()),
                 root_events=int(pk.Info["root_events"].sum()), infeasible=int((pk.Status == 2).sum()),
                 max_nodes_of_a_model=int(pk.Nodes.max()), deepest=int(pk.Info["deepest"].max()), kernel_ms=pk.Stats["loop_ms"],
                 us_per_node_packed=1e3 * statistics.median(ts["packed"]) / nodes, us_per_node_single=1e3 * statistics.median(ts["single"]) / nodes,
                 packed_wins=bool(d["packed"]["median"] < d["single"]["min"]), single_wins=bool(d["single"]["median"] < d["packed"]["min"]))
        out["families"][str(count)] = d
    # a family both packed calls accept (every row <=, b >= 0): the dual root against the primal root, the searches behind them
    c, A, bs = rhs_family(20, 8, 256)
    sides = {"dual_root": lambda: S.SolvePackedBnbDual(c, A, bs, None, 1.0, **kw), "primal_root": lambda: S.SolvePackedBnb(c, A, bs, 1.0, **kw)}
    d = alternate(sides, reps)
    a, b = sides["dual_root"](), sides["primal_root"]()
    assert a.Status.tolist() == b.Status.tolist() and np.array_equal(a.OptimalValue, b.OptimalValue)
    d.update(count=256, nodes_dual_root=int(a.Nodes.sum()), nodes_primal_root=int(b.Nodes.sum()),
             root_events_dual=int(a.Info["root_events"].sum()), root_events_primal=int(b.Info["root_events"].sum()))
    out["le_family"] = d
    return out


def alternate(sides, reps):
    """Host wall in ms of every side, the sides alternating in one process, one untimed round first; a side wins against another iff
    its median lies below the other's minimum."""
    ts = {k: [] for k in sides}
    for i in range(reps + 1):
        for k, f in sides.items():
            t0 = time.perf_counter()
            f()
            if i >= 1:
                ts[k].append(1e3 * (time.perf_counter() - t0))
    d = {k: stats(v) for k, v in ts.items()}
    d["wins"] = {a: [b for b in sides if b != a and d[a]["median"] < d[b]["min"]] for a in sides}
    return d


def main():
    args = sys.argv[1:]
    if "--packed-trace" in args:        # four packed calls of 256 right-hand sides and one of binary_ip(60, 12), for a kernel trace
        L._lib.check(L._lib.lib().lpx_init(0))
        c, A, bs = rhs_family(20, 8, 256)
        for _ in range(4):
            L.LPSolver().SolvePackedBnb(c, A, bs, 1.0)
        c, A, rel, b = synth.binary_ip(60, 12)
        r = L.LPSolver().SolvePackedBnb(c, np.ascontiguousarray(A[:12]), b[:12], 1.0, max_nodes=1000000, max_events=100000000)
        print(json.dumps({"bip_60x12_nodes": int(r.Nodes[0]), "status": int(r.Status[0]), "loop_ms": r.Stats["loop_ms"]}))
        return
    if "--compare-packed-dual" in args:
        args.remove("--compare-packed-dual")
        flag_set = "plain"
        if "--flag-sets" in args:
            j = args.index("--flag-sets")
            flag_set = args[j + 1]
            del args[j:j + 2]
        reps = int(args[0]) if args else 7
        L._lib.check(L._lib.lib().lpx_init(0))
        print(json.dumps(compare_packed_dual(reps, [256, 4096], 2, flag_set)))
        return
    if "--compare-packed" in args:
        args.remove("--compare-packed")
        flag_set = "plain"
        if "--flag-sets" in args:
            j = args.index("--flag-sets")
            flag_set = args[j + 1]
            del args[j:j + 2]
        reps = int(args[0]) if args else 7
        L._lib.check(L._lib.lib().lpx_init(0))
        print(json.dumps(compare_packed(reps, [256, 4096], 2, [4, 16, 64], flag_set)))
        return
    if "--compare-tighten" in args:
        k = args.index("--compare-tighten")
        widths = [1, 16, 256]
        if k + 1 < len(args) and args[k + 1][:1].isdigit() and ("," in args[k + 1] or k + 2 < len(args) and args[k + 2][:1].isdigit()):
            widths = [int(w) for w in args[k + 1].split(",") if w]
            del args[k + 1]
        del args[k]
        only, max_nodes, flag_sets = None, 0, "plain,both"
        for flag in ("--model", "--max-nodes", "--flag-sets"):
            if flag in args:
                j = args.index(flag)
                if flag == "--model":
                    only = args[j + 1]
                elif flag == "--max-nodes":
                    max_nodes = int(args[j + 1])
                else:
                    flag_sets = args[j + 1]
                del args[j:j + 2]
        reps = int(args[0]) if args else 7
        L._lib.check(L._lib.lib().lpx_init(0))
        out = {name: compare_tighten(n, m, reps, max_nodes, [f for f in flag_sets.split(",") if f and f != "none"], widths)
               for name, n, m in models() if only is None or name == only}
        print(json.dumps(out))
        return
    if "--compare-cuts" in args:
        k = args.index("--compare-cuts")
        widths = [1, 16, 256]
        if k + 1 < len(args) and args[k + 1][:1].isdigit() and "," in args[k + 1]:
            widths = [int(w) for w in args[k + 1].split(",") if w]
            del args[k + 1]
        del args[k]
        only, max_nodes, rounds, K = None, 0, [2, 4, 8], 8
        for flag in ("--model", "--max-nodes", "--rounds", "--cuts-per-round"):
            if flag in args:
                j = args.index(flag)
                if flag == "--model":
                    only = args[j + 1]
                elif flag == "--max-nodes":
                    max_nodes = int(args[j + 1])
                elif flag == "--rounds":
                    rounds = [int(w) for w in args[j + 1].split(",") if w]
                else:
                    K = int(args[j + 1])
                del args[j:j + 2]
        reps = int(args[0]) if args else None
        L._lib.check(L._lib.lib().lpx_init(0))
        out = {name: compare_cuts(n, m, reps if reps is not None else (3 if n >= 128 else 7), max_nodes, widths, rounds, K)
               for name, n, m in models() if only is None or name == only}
        print(json.dumps(out))
        return
    if "--compare-root" in args:
        k = args.index("--compare-root")
        widths = [int(w) for w in args[k + 1].split(",") if w]
        del args[k:k + 2]
        only, max_nodes = None, 0
        for flag in ("--model", "--max-nodes"):
            if flag in args:
                j = args.index(flag)
                if flag == "--model":
                    only = args[j + 1]
                else:
                    max_nodes = int(args[j + 1])
                del args[j:j + 2]
        reps = int(args[0]) if args else 7
        L._lib.check(L._lib.lib().lpx_init(0))
        out = {name: compare_root(n, m, reps, max_nodes, widths) for name, n, m in models() if only is None or name == only}
        print(json.dumps(out))
        return
    stall_events, stalls = None, None
    for flag in ("--stall-events", "--compare-guard"):
        if flag in args:
            k = args.index(flag)
            if flag == "--stall-events":
                stall_events = int(args[k + 1])
            else:
                stalls = [int(x) for x in args[k + 1].split(",") if x]
            del args[k:k + 2]
    branching, candidates, probe_iter, settings = None, 4, None, None
    for flag in ("--branching", "--candidates", "--probe-iter", "--compare-branching"):
        if flag in args:
            k = args.index(flag)
            if flag == "--branching":
                branching = args[k + 1]
            elif flag == "--candidates":
                candidates = int(args[k + 1])
            elif flag == "--probe-iter":
                probe_iter = int(args[k + 1])
            else:
                settings = [(int(x.split(":")[0]), int(x.split(":")[1]) if ":" in x else None) for x in args[k + 1].split(",") if x]
            del args[k:k + 2]
    side_flags = {"long_step": "--long-step" in args, "cutoff": "--cutoff" in args}
    args = [a for a in args if a not in ("--long-step", "--cutoff")]
    only, max_nodes, node_form, flag_sets, divers, widths, plunge, depths = None, 0, None, None, None, None, None, None
    for flag in ("--model", "--max-nodes", "--node-form", "--flag-sets", "--divers", "--compare-divers", "--plunge", "--compare-plunge"):
        if flag in args:
            k = args.index(flag)
            if flag == "--model":
                only = args[k + 1]
            elif flag == "--node-form":
                node_form = args[k + 1]
            elif flag == "--flag-sets":
                flag_sets = args[k + 1]
            elif flag == "--divers":
                divers = int(args[k + 1])
            elif flag == "--compare-divers":
                widths = [int(w) for w in args[k + 1].split(",") if w]
            elif flag == "--plunge":
                plunge = int(args[k + 1])
            elif flag == "--compare-plunge":
                depths = [int(w) for w in args[k + 1].split(",") if w]
            else:
                max_nodes = int(args[k + 1])
            del args[k:k + 2]
    compare = "--compare-forms" in args
    trace_only = "--trace-only" in args
    args = [a for a in args if a not in ("--compare-forms", "--trace-only")]
    reps = int(args[0]) if args else 7
    lib = L._lib.lib()
    L._lib.check(lib.lpx_init(0))
    out = {}
    if flag_sets is None:
        flag_sets = "plain,both" if widths or depths or settings or stalls else "plain,long_step,cutoff,both"
    if stalls:
        for name, n, m, seed in list((nm, n, m, None) for nm, n, m in models()) + [("bip_40x16_s6", 40, 16, 6)]:
            if name == only or (only is None and seed is None):
                out[name] = compare_guard(n, m, reps, max_nodes, [f for f in flag_sets.split(",") if f and f != "none"],
                                          divers if divers else 1, stalls, seed)
        print(json.dumps(out))
        return
    if stall_events is not None and divers is None:
        divers = 1
    if settings:
        for name, n, m in models():
            if only is None or name == only:
                out[name] = compare_branching(n, m, reps, max_nodes, [f for f in flag_sets.split(",") if f and f != "none"],
                                              divers if divers else 1, settings)
        print(json.dumps(out))
        return
    if branching is not None and divers is None:
        divers = 1
    if depths:
        for name, n, m in models():
            if only is None or name == only:
                out[name] = compare_plunge(n, m, reps, max_nodes, [f for f in flag_sets.split(",") if f and f != "none"],
                                           divers if divers else 1, depths)
        print(json.dumps(out))
        return
    if plunge is not None and divers is None:
        divers = 1
    if widths:
        for name, n, m in models():
            if only is None or name == only:
                out[name] = compare_divers(n, m, reps, max_nodes, [f for f in flag_sets.split(",") if f and f != "none"], widths)
        print(json.dumps(out))
        return
    if node_form is None:
        node_form = "launches" if divers is None else "onchip"
    if compare:
        for name, n, m in models():
            if only is None or name == only:
                out[name] = compare_forms(n, m, reps, max_nodes, [f for f in flag_sets.split(",") if f and f != "none"])
        print(json.dumps(out))
        return
    for name, n, m in models():
        if only is not None and name != only:
            continue
        c, A, rel, b = synth.binary_ip(n, m)
        rows_p = L.LPProblem.from_arrays(0, c, A, rel, b)
        bnd_p = L.LPProblem.from_arrays(0, c, A[:m], rel[:m], b[:m])
        rec = {"n": n, "m": m, "rows_shape": [m + n + 1, 2 * n + m + 1], "bounded_shape": [m + 1, n + m + 1]}

        def run_rows():
            t0 = time.perf_counter()
            r = L.BranchAndBound(bnb_mode=1, bnb_search=2, bnb_dive=1, concurrent_nodes=128, max_nodes=max_nodes).Solve(rows_p)
            return 1e3 * (time.perf_counter() - t0), r

        def run_bounded():
            t0 = time.perf_counter()
            try:
                how = {} if branching is None else {"branching": branching, "candidates": candidates, "probe_iter": probe_iter}
                if stall_events is not None:
                    how["stall_events"] = stall_events
                r = L.LPSolver().SolveBnbBounded(bnd_p, 1.0, max_nodes=max_nodes, node_form=node_form, divers=divers, plunge=plunge,
                                                 **side_flags, **how)
            except L.SolverException as e:
                if e.code != L._lib.ITER_LIMIT or not max_nodes:
                    raise
                r = e.result
            return 1e3 * (time.perf_counter() - t0), r

        if trace_only:
            ms, rb = run_bounded()
            out[name] = {"node_form": node_form, "divers": divers, "plunge": plunge, "ms": ms, "nodes": int(rb.Nodes),
                         "events": rb.BnbInfo["events"], "rounds": rb.BnbInfo.get("rounds"), "launched": rb.BnbInfo.get("launched"),
                         "dropped": rb.BnbInfo.get("dropped"), "branching": branching, "probes": rb.BnbInfo.get("probes"),
                         "probe_events": rb.BnbInfo.get("probe_events"), "pruned_by_probe": rb.BnbInfo.get("pruned_by_probe"),
                         "stall_events": stall_events, "guarded_nodes": rb.BnbInfo.get("guarded_nodes"),
                         "bland_events": rb.BnbInfo.get("bland_events")}
            continue
        base = device_used_mb()
        ta, tb, na, nb = [], [], [], []
        peak_a = peak_b = None
        for i in range(reps + 2):
            ms, ra = run_rows()
            if i == 0:
                peak_a = device_used_mb()
            if i >= 2:
                ta.append(ms); na.append(ra.LpSolves / (ms / 1e3))
            ms, rb = run_bounded()
            if i == 0:
                peak_b = device_used_mb()
            if i >= 2:
                tb.append(ms); nb.append(rb.Nodes / (ms / 1e3))
        rec["rows"] = {"ms": stats(ta), "nodes_per_s": stats(na), "lp_solves": int(ra.LpSolves), "nodes": int(ra.Nodes),
                       "optimum": ra.OptimalValue}
        info = rb.BnbInfo
        rec["bounded"] = {"ms": stats(tb), "nodes_per_s": stats(nb), "nodes": int(rb.Nodes), "optimum": rb.OptimalValue,
                          "events": info["events"], "flips": info["flips"], "max_K": info["max_K"],
                          "events_per_node": info["events"] / max(1, rb.Nodes),
                          "wall_us_per_node": 1e3 * statistics.median(tb) / max(1, rb.Nodes)}
        rec["same_optimum"] = bool(abs(ra.OptimalValue - rb.OptimalValue) <= 1e-9 * max(1.0, abs(ra.OptimalValue)))
        if base is not None:
            # (a) ran first: its reading is its own footprint; (b)'s is what it added on top (caches of (a) stay allocated)
            rec["device_mb"] = {"before": base, "after_rows_first_solve": peak_a, "after_bounded_first_solve": peak_b,
                                "rows_added": peak_a - base, "bounded_added": peak_b - peak_a}
        # the fixed cost of a node: a K = 0 node call on a solved root (no event, no flip)
        T, basis = synth.primal_tableau_from(c, A[:m], b[:m])
        ub = np.full(T.shape[1] - 1, np.inf); ub[:n] = 1.0
        with L.DeviceTableau.from_host(T, basis) as dt:
            dt.set_bounds(ub)
            dt.bounded_run()
            for _ in range(20):
                dt.bounded_node([], [], [], n, batch=16, form=node_form)
            t0 = time.perf_counter()
            for _ in range(200):
                dt.bounded_node([], [], [], n, batch=16, form=node_form)
            rec["bounded"]["empty_node_us"] = 1e6 * (time.perf_counter() - t0) / 200
        rec["bounded"]["node_form"] = node_form
        out[name] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
