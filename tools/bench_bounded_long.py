"""Host wall of the bounded dual loop with and without the long-step ratio test and the objective cutoff, on the device.

Legs (the method of tools/bench_bounded_dual.py: profiler off, handles warm, sides alternating, REPS timed runs, host wall; a timed
run starts from a restored snapshot, the restore is not timed, and ends when the call returns, which is after the device has
finished):
  (a) dual start: covering(256, 768, 1) and covering(1024, 2048, 1) with u = 1 -- Min c.x, A x >= b, 0 <= x <= 1 -- from the
      slack basis by lpx_bounded_dual_run3, plain (flags 0) against LPX_BDUAL_LONG_STEP: pivots, passes, ms.
  (b) search: synth.binary_ip(60, 12) and synth.binary_ip(128, 64) without their bound rows, to optimality by
      LPSolver().SolveBnbBounded with the four flag sets {-, long_step, cutoff, both}: nodes, pivots, passes, ms, nodes/s.
      The larger model is timed BIG_REPS times (default 2) without an untimed run of its own: a solve takes tens of seconds, and
      what a first run pays once (handle, graph capture) is milliseconds.
  (c) unchanged: the SKIP_FIXED-only driver (SolveBnbBounded without flags) on binary_ip(60, 12), REPS timed solves; run it once
      per checkout with `--root DIR` (the tree whose package is imported; default: this one) to compare two commits on one box.
Prints one JSON line.

`--compare-packed` measures the packed call by a dual start (lpx_solve_packed_dual) instead of the legs: host
wall of whole calls, REPS (default 15) timed rounds behind one warm-up round, the sides alternating in one process; a side wins iff
its median lies below the other's minimum.  256 covering models covering(12, 60, seed) as Min c.x, A x >= b:
SolvePackedDual with and without the long step against 256 SolveBoundedDual calls (statuses, optima and counts asserted equal);
then 4096 right-hand sides of ONE shared model (stride 0 for c, A and rel), long step on against off.  With `--parent-lib
PATH/liblpx.so` (the library of the parent commit) the existing packed primal call, lpx_solve_packed, is measured on both libraries
in the same process, alternating, with the bits of their outputs asserted equal.  `--packed-trace` makes four packed dual calls
and nothing else, for a run of its own under `rocprofv3 --kernel-trace --stats`.

`--compare-warm` measures the packed calls from a solved base (lpx_packed_base_open / _solve) against the
cold packed call of the same scenarios, SolvePackedDual with c, A and rel at stride 0, in the same library and process: +-20 %
right-hand sides of covering(12, 60, 1) (13 x 73) and of covering(110, 50, 1) (111 x 161, near the fit limit), count 256, 4096 and
65536 (the last with BIG_REPS timed rounds), with and without the long step.  Three sides alternate in every round: cold; warm with
the base kept open (PackedBase.solve alone is timed); warm with the open and the close inside the timed region.  Host wall of whole
calls, the rule of section 4.17 per pair; statuses asserted equal and optima within 1e-9 relative; events per scenario of both
sides.  `--warm-trace` makes three calls of each side at count 4096 on the 13 x 73 model with the long step and nothing else, for a
run of its own under
`rocprofv3 --kernel-trace --stats`.

`--compare-costs` measures the packed cost scenarios from a solved base (lpx_packed_base_solve_costs) against
the cold packed call of the same scenarios, SolvePackedDual with c at stride n and everything else at stride 0, in the same library
and process: +-20 % costs of covering(12, 60, 1) and covering(110, 50, 1), count 256, 4096 and 65536 (the last with BIG_REPS timed
rounds), without b and with +-20 % right-hand sides, the long step on.  Two sides alternate in every round: cold; kept =
PackedBase.solve_costs with the base opened outside the timed region.  Host wall of whole calls, the rule of section 4.17; every
scenario asserted OPTIMAL on both sides and optima within 1e-9 relative; events per scenario of both sides.  With `--parent-lib
PATH/liblpx.so` the existing PackedBase.solve call (lpx_packed_base_open / _solve) is measured on both libraries in the same
process, alternating, with the bits of their outputs asserted equal.

`--trace-only` runs leg (a) on the smaller model once per side (no untimed run in front), for a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_bounded_long.py --trace-only`, whose kernel table gives the mean launch
time of lpx_bounded_long_select, lpx_bounded_dual_select and the lpx_update launches they feed.

usage: bench_bounded_long.py [--leg a|b|c]... [--root DIR] [--big-reps N] [--skip-big] [--trace-only]
                             [--compare-packed [--parent-lib PATH] | --packed-trace | --compare-warm | --warm-trace |
                              --compare-costs [--parent-lib PATH]] [REPS]"""
import json
import os
import statistics
import sys
import time


def _args():
    a = sys.argv[1:]
    opt = {"legs": [], "root": None, "big_reps": 2, "skip_big": False, "trace_only": False, "reps": None, "compare_packed": False,
           "packed_trace": False, "parent_lib": None, "compare_warm": False, "warm_trace": False, "compare_costs": False}
    i = 0
    while i < len(a):
        if a[i] == "--leg":
            opt["legs"].append(a[i + 1]); i += 2
        elif a[i] == "--root":
            opt["root"] = a[i + 1]; i += 2
        elif a[i] == "--big-reps":
            opt["big_reps"] = int(a[i + 1]); i += 2
        elif a[i] == "--skip-big":
            opt["skip_big"] = True; i += 1
        elif a[i] == "--trace-only":
            opt["trace_only"] = True; i += 1
        elif a[i] == "--compare-packed":
            opt["compare_packed"] = True; i += 1
        elif a[i] == "--packed-trace":
            opt["packed_trace"] = True; i += 1
        elif a[i] == "--compare-warm":
            opt["compare_warm"] = True; i += 1
        elif a[i] == "--compare-costs":
            opt["compare_costs"] = True; i += 1
        elif a[i] == "--warm-trace":
            opt["warm_trace"] = True; i += 1
        elif a[i] == "--parent-lib":
            opt["parent_lib"] = a[i + 1]; i += 2
        else:
            opt["reps"] = int(a[i]); i += 1
    if not opt["legs"]:
        opt["legs"] = ["a", "b", "c"]
    if opt["reps"] is None:
        opt["reps"] = 15 if opt["compare_packed"] else 7           # --compare-warm, --compare-costs: 7
    return opt


OPT = _args()
ROOT = os.path.abspath(OPT["root"]) if OPT["root"] else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import linear_programming_solver_lpr381_amd as L
from linear_programming_solver_lpr381_amd import synth

LONG, CUT = 2, 4


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "samples": len(ts)} if ts else None


def covering(m, n, seed):
    """Min c.x, A x >= b, 0 <= x <= 1 with A, c > 0 as an internal tableau: dual feasible, every RHS negative."""
    c, A, _ = synth.dense_lp(m, n, seed)
    A = np.abs(A)
    c = np.abs(c) + 1.0
    b = A.sum(axis=1) * np.random.default_rng(seed).uniform(0.2, 0.5, size=m)
    T, basis = synth.primal_tableau_from(-c, -A, -b)
    ub = np.full(T.shape[1] - 1, np.inf)
    ub[:n] = 1.0
    return T, basis, ub


def leg_a(reps, shapes, warm=2):
    out = {}
    for m, n in shapes:
        T, basis, ub = covering(m, n, 1)
        sides = {}
        for name in ("plain", "long_step"):
            dt = L.DeviceTableau.from_host(T, basis)
            dt.set_bounds(ub)
            dt.snapshot()
            sides[name] = dt
        t = {k: [] for k in sides}
        rec = {"shape": list(T.shape)}
        for i in range(reps + warm):
            for name, dt in sides.items():
                dt.restore()
                t0 = time.perf_counter()
                status, st = dt.bounded_dual_run(long_step=(name == "long_step"), max_iter=1000000)
                if i >= warm:
                    t[name].append(1e3 * (time.perf_counter() - t0))
                k0, k1, passes = dt.bounded_counts()
                rec[name] = dict(status=status, pivots=k0 + k1, passes=passes, launches=st["launches"], z=dt.bounded_solution(n)[1])
        for name, dt in sides.items():
            rec[name]["ms"] = stats(t[name])
            dt.close()
        rec["rel_diff_z"] = abs(rec["plain"]["z"] - rec["long_step"]["z"]) / max(1.0, abs(rec["plain"]["z"]))
        out["covering_%dx%d" % (m, n)] = rec
    return out


def _bnb(problem, flags):
    kw = {}
    if flags & LONG:
        kw["long_step"] = True
    if flags & CUT:
        kw["cutoff"] = True
    t0 = time.perf_counter()
    res = L.LPSolver().SolveBnbBounded(problem, 1.0, **kw)
    ms = 1e3 * (time.perf_counter() - t0)
    log = res.BnbLog
    return ms, dict(status=res.Status, value=res.OptimalValue, nodes=int(res.Nodes), events=int(res.BnbInfo["events"]),
                    flips=int(res.BnbInfo["flips"]), pruned_bound=int(res.BnbInfo["pruned_bound"]),
                    cutoff_nodes=int((log["status"] == 5).sum()), longest_node=int(log["events"].max()))


def _binary(n, m):
    c, A, rel, b = synth.binary_ip(n, m)
    return L.LPProblem.from_arrays(0, c, A[:m], rel[:m], b[:m])


def leg_b(reps, big_reps, skip_big):
    out = {}
    for (n, m), r in (((60, 12), reps), ((128, 64), 0 if skip_big else big_reps)):
        if r <= 0:
            continue
        p = _binary(n, m)
        t = {f: [] for f in (0, LONG, CUT, LONG | CUT)}
        rec = {}
        warm = 2 if (n, m) == (60, 12) else 0
        for i in range(r + warm):
            for f in t:
                ms, info = _bnb(p, f)
                if i >= warm:
                    t[f].append(ms)
                rec[f] = info
        for f in t:
            rec[f]["ms"] = stats(t[f])
            rec[f]["nodes_per_s"] = 1e3 * rec[f]["nodes"] / rec[f]["ms"]["median_ms"]
        out["binary_ip_%dx%d" % (n, m)] = {{0: "plain", LONG: "long_step", CUT: "cutoff", LONG | CUT: "both"}[f]: v for f, v in rec.items()}
    return out


def leg_c(reps):
    p = _binary(60, 12)
    ts, info = [], None
    for i in range(reps + 2):
        t0 = time.perf_counter()
        res = L.LPSolver().SolveBnbBounded(p, 1.0)
        if i >= 2:
            ts.append(1e3 * (time.perf_counter() - t0))
        info = dict(status=res.Status, value=res.OptimalValue, nodes=int(res.Nodes), events=int(res.BnbInfo["events"]))
    info["ms"] = stats(ts)
    info["spread"] = (max(ts) - min(ts)) / statistics.median(ts)
    return {"root": ROOT, "binary_ip_60x12_skip_fixed_only": info}


def verdict(a, b, na, nb):
    """The rule of DESIGN section 4.17: a side wins iff its median lies below the other's minimum."""
    if a["median_ms"] < b["min_ms"]:
        return na
    if b["median_ms"] < a["min_ms"]:
        return nb
    return "tie"


def covering_models(count, m=12, n=60):
    """covering(m, n, seed) for seeds 1..count as user models: stacked (c, A, b) of Min c.x, A x >= b, 0 <= x <= 1."""
    cs, As, bs = [], [], []
    for s in range(1, count + 1):
        c, A, _ = synth.dense_lp(m, n, s)
        A = np.abs(A)
        cs.append(np.abs(c) + 1.0); As.append(A)
        bs.append(A.sum(axis=1) * np.random.default_rng(s).uniform(0.2, 0.5, size=m))
    return np.stack(cs), np.stack(As), np.stack(bs)


def _timed(f):
    t0 = time.perf_counter()
    r = f()
    return 1e3 * (time.perf_counter() - t0), r


def packed_primal_parent(reps, parent_lib):
    """lpx_solve_packed of this tree's library against the parent commit's, loaded beside it: the same arrays, alternating."""
    import ctypes as C
    Lb = L._lib
    libs = {"tree": Lb.lib(), "parent": C.CDLL(os.path.abspath(parent_lib))}
    libs["parent"].lpx_solve_packed.argtypes = libs["tree"].lpx_solve_packed.argtypes
    count, m, n = 256, 12, 60
    cs, As, bs = [], [], []
    for s in range(1, count + 1):
        c, A, rel, b = synth.binary_ip(n, m, s)
        cs.append(c); As.append(A[:m]); bs.append(b[:m])
    c, A, b = (np.ascontiguousarray(np.stack(v)) for v in (cs, As, bs))
    up = np.ones(n)
    pm = Lb.PackedModels(count, m, n, 0, c.ctypes.data_as(Lb.dp), A.ctypes.data_as(Lb.dp), b.ctypes.data_as(Lb.dp), None,
                         up.ctypes.data_as(Lb.dp), n, m * n, m, 0, 0)
    outs, t = {}, {k: [] for k in libs}
    for k in libs:
        status = np.zeros(count, dtype=np.int32); x = np.zeros((count, n)); value = np.zeros(count)
        recs = (Lb.PrimalRecord * count)(); basis = np.zeros((count, m), dtype=np.int32); at = np.zeros((count, n), dtype=np.uint8)
        pr = Lb.PackedResults(status.ctypes.data_as(Lb.ip), x.ctypes.data_as(Lb.dp), value.ctypes.data_as(Lb.dp), recs,
                              basis.ctypes.data_as(Lb.ip), at.ctypes.data_as(C.POINTER(C.c_uint8)))
        outs[k] = (pr, status, x, value, recs, basis, at)
    for i in range(reps + 1):
        for k, lib in libs.items():
            ms, rc = _timed(lambda: lib.lpx_solve_packed(C.byref(pm), None, C.byref(outs[k][0]), None))
            assert rc == 0, k
            t[k].append(ms)
    a, p = outs["tree"], outs["parent"]
    assert all(a[j].tobytes() == p[j].tobytes() for j in (1, 2, 3, 5, 6)) and bytes(a[4]) == bytes(p[4]), "tree and parent differ"
    rec = {k: stats(v[1:]) for k, v in t.items()}
    rec["winner"] = verdict(rec["tree"], rec["parent"], "tree", "parent")
    rec["equal_bits"] = True
    return rec


def compare_packed(reps, trace, parent_lib):
    S = L.LPSolver()
    count = 256
    c, A, b = covering_models(count)
    rel = np.ones(12, dtype=np.int32)
    if trace:                                           # one warm-up call and three calls: one kernel each in the trace
        for i in range(4):
            r = S.SolvePackedDual(c, A, b, rel, 1.0, sense="min")
        return {"packed_trace": {"count": count, "calls": 4, "events": int(r.Events.sum()), "launches_per_call": r.Stats["launches"]}}
    out = {}
    ps = [L.LPProblem.from_arrays(1, c[k], A[k], [1] * 12, b[k]) for k in range(count)]
    sides = {"packed_long": [], "packed_plain": [], "single_long": [], "single_plain": []}
    for i in range(reps + 1):
        ms, rp = _timed(lambda: S.SolvePackedDual(c, A, b, rel, 1.0, sense="min"))
        sides["packed_long"].append(ms)
        ms, rq = _timed(lambda: S.SolvePackedDual(c, A, b, rel, 1.0, sense="min", long_step=False))
        sides["packed_plain"].append(ms)
        ms, rs = _timed(lambda: [S.SolveBoundedDual(p, 1.0) for p in ps])
        sides["single_long"].append(ms)
        ms, rt = _timed(lambda: [S.SolveBoundedDual(p, 1.0, long_step=False) for p in ps])
        sides["single_plain"].append(ms)
        for packed, singles in ((rp, rs), (rq, rt)):
            assert all(packed.Status[k] == x.Status and packed.OptimalValue[k] == x.OptimalValue and
                       tuple(packed.BoundCounts[k].tolist()) == x.BoundCounts for k, x in enumerate(singles)), "packed and single differ"
    rec = {"count": count, "shape": [13, 73], "events_long": int(rp.Events.sum()), "passes_long": int(rp.Passes.sum()),
           "events_plain": int(rq.Events.sum()), "loop_ms_last": rp.Stats["loop_ms"],
           "bytes_in": int(c.nbytes + A.nbytes + b.nbytes + rel.nbytes + 8 * 60)}
    rec.update({k: stats(v[1:]) for k, v in sides.items()})                     # the first round is the warm-up
    rec["winner_packed_vs_single_long"] = verdict(rec["packed_long"], rec["single_long"], "packed", "single")
    rec["winner_packed_vs_single_plain"] = verdict(rec["packed_plain"], rec["single_plain"], "packed", "single")
    rec["winner_long_vs_plain_packed"] = verdict(rec["packed_long"], rec["packed_plain"], "long_step", "plain")
    rec["single_over_packed_long"] = rec["single_long"]["median_ms"] / rec["packed_long"]["median_ms"]
    rec["single_over_packed_plain"] = rec["single_plain"]["median_ms"] / rec["packed_plain"]["median_ms"]
    out["covering_256_of_13x73"] = rec
    # one shared model, 4096 right-hand sides: stride 0 for c, A and rel
    count = 4096
    bs = b[0] * np.random.default_rng(5).uniform(0.8, 1.2, size=(count, 12))
    sides = {"long_step": [], "plain": []}
    for i in range(reps + 1):
        ms, rl = _timed(lambda: S.SolvePackedDual(c[0], A[0], bs, rel, 1.0, sense="min"))
        sides["long_step"].append(ms)
        ms, rn = _timed(lambda: S.SolvePackedDual(c[0], A[0], bs, rel, 1.0, sense="min", long_step=False))
        sides["plain"].append(ms)
        assert np.array_equal(rl.Status, rn.Status) and (rl.Status == 0).all()
        assert np.abs(rl.OptimalValue - rn.OptimalValue).max() <= 1e-9 * np.abs(rn.OptimalValue).max()
    rec = {"count": count, "shape": [13, 73], "events_long": int(rl.Events.sum()), "passes_long": int(rl.Passes.sum()),
           "events_plain": int(rn.Events.sum()), "bytes_in": int(c[0].nbytes + A[0].nbytes + bs.nbytes + rel.nbytes + 8 * 60)}
    rec.update({k: stats(v[1:]) for k, v in sides.items()})
    rec["winner"] = verdict(rec["long_step"], rec["plain"], "long_step", "plain")
    rec["us_per_model_long"] = 1e3 * rec["long_step"]["median_ms"] / count
    out["rhs_4096_shared"] = rec
    if parent_lib:
        out["packed_primal_tree_vs_parent"] = packed_primal_parent(reps, parent_lib)
    return out


def compare_warm(reps, big_reps, trace):
    S = L.LPSolver()
    out = {}
    for m, n in (((12, 60),) if trace else ((12, 60), (110, 50))):
        assert L._lib.lib().lpx_packed_fits(m, n) == 1
        cs, As, b0s = covering_models(1, m, n)
        c, A, b0 = cs[0], As[0], b0s[0]
        rel = np.ones(m, dtype=np.int32)
        for count in ((4096,) if trace else (256, 4096, 65536)):
            bs = b0 * np.random.default_rng(5).uniform(0.8, 1.2, size=(count, m))
            for long_step in ((True,) if trace else (True, False)):
                rounds = 2 if trace else (big_reps if count == 65536 else reps)
                sides = {"cold": [], "warm_kept": [], "warm_with_open": []}
                with S.OpenPackedBase(c, A, b0, rel, 1.0, sense="min", long_step=long_step) as kept:
                    for i in range(rounds + 1):
                        ms, rc = _timed(lambda: S.SolvePackedDual(c, A, bs, rel, 1.0, sense="min", long_step=long_step))
                        sides["cold"].append(ms)
                        ms, rw = _timed(lambda: kept.solve(bs, long_step=long_step))
                        sides["warm_kept"].append(ms)

                        def opened():
                            with S.OpenPackedBase(c, A, b0, rel, 1.0, sense="min", long_step=long_step) as base:
                                return base.solve(bs, long_step=long_step)
                        ms, ro = _timed(opened)
                        sides["warm_with_open"].append(ms)
                        assert np.array_equal(rc.Status, rw.Status) and np.array_equal(rw.Status, ro.Status), "statuses differ"
                        ok = rc.Status == 0
                        assert (np.abs(rw.OptimalValue - rc.OptimalValue)[ok] <= 1e-9 * np.maximum(1.0, np.abs(rc.OptimalValue[ok]))).all()
                        assert rw.OptimalValue.tobytes() == ro.OptimalValue.tobytes()
                rec = {"shape": [m + 1, n + m + 1], "count": count, "long_step": long_step, "optimal": int(ok.sum()),
                       "events_per_scenario_cold": float(rc.Events.mean()), "events_per_scenario_warm": float(rw.Events.mean()),
                       "base_events": int(kept.Base.Events[0])}
                if not trace:
                    rec.update({k: stats(v[1:]) for k, v in sides.items()})     # the first round is the warm-up
                    rec["winner_kept"] = verdict(rec["warm_kept"], rec["cold"], "warm", "cold")
                    rec["winner_with_open"] = verdict(rec["warm_with_open"], rec["cold"], "warm", "cold")
                    rec["cold_over_warm_kept"] = rec["cold"]["median_ms"] / rec["warm_kept"]["median_ms"]
                out["%dx%d count %d %s" % (m + 1, n + m + 1, count, "long" if long_step else "plain")] = rec
    return out


def packed_warm_parent(reps, parent_lib):
    """lpx_packed_base_open / _solve of this tree's library against the parent commit's, loaded beside it: the same arrays,
    alternating; 4096 right-hand sides of covering(12, 60, 1)."""
    import ctypes as C
    Lb = L._lib
    libs = {"tree": Lb.lib(), "parent": C.CDLL(os.path.abspath(parent_lib))}
    for f in ("lpx_packed_base_open", "lpx_packed_base_solve", "lpx_packed_base_close"):
        getattr(libs["parent"], f).argtypes = getattr(libs["tree"], f).argtypes
    count, m, n = 4096, 12, 60
    cs, As, b0s = covering_models(1, m, n)
    c, A, b0 = (np.ascontiguousarray(v[0]) for v in (cs, As, b0s))
    rel = np.ones(m, dtype=np.int32); up = np.ones(n)
    bs = np.ascontiguousarray(b0 * np.random.default_rng(5).uniform(0.8, 1.2, size=(count, m)))
    pm = Lb.PackedBaseModel(m, n, 1, c.ctypes.data_as(Lb.dp), A.ctypes.data_as(Lb.dp), b0.ctypes.data_as(Lb.dp), None,
                            up.ctypes.data_as(Lb.dp), rel.ctypes.data_as(Lb.ip))
    outs, t, hs = {}, {k: [] for k in libs}, {}
    for k, lib in libs.items():
        status = np.zeros(count, dtype=np.int32); x = np.zeros((count, n)); value = np.zeros(count)
        recs = (Lb.PackedDualRecord * count)(); basis = np.zeros((count, m), dtype=np.int32); at = np.zeros((count, n), dtype=np.uint8)
        y = np.zeros((count, m)); d = np.zeros((count, n))
        pr = Lb.PackedDualResults(status.ctypes.data_as(Lb.ip), x.ctypes.data_as(Lb.dp), value.ctypes.data_as(Lb.dp), recs,
                                  basis.ctypes.data_as(Lb.ip), at.ctypes.data_as(C.POINTER(C.c_uint8)), y.ctypes.data_as(Lb.dp),
                                  d.ctypes.data_as(Lb.dp))
        outs[k] = (pr, status, x, value, recs, basis, at, y, d)
        hs[k] = C.c_void_p()
        assert lib.lpx_packed_base_open(C.byref(pm), Lb.BDUAL_LONG_STEP, None, None, C.byref(hs[k])) == 0, k
    for i in range(reps + 1):
        for k, lib in libs.items():
            ms, rc = _timed(lambda: lib.lpx_packed_base_solve(hs[k], count, bs.ctypes.data_as(Lb.dp), Lb.BDUAL_LONG_STEP, None,
                                                              C.byref(outs[k][0]), None))
            assert rc == 0, k
            t[k].append(ms)
    for k, lib in libs.items():
        lib.lpx_packed_base_close(hs[k])
    a, p = outs["tree"], outs["parent"]
    assert all(a[j].tobytes() == p[j].tobytes() for j in (1, 2, 3, 5, 6, 7, 8)) and bytes(a[4]) == bytes(p[4]), "tree and parent differ"
    rec = {k: stats(v[1:]) for k, v in t.items()}
    rec["winner"] = verdict(rec["tree"], rec["parent"], "tree", "parent")
    rec["equal_bits"] = True
    return rec


def compare_costs(reps, big_reps, parent_lib):
    S = L.LPSolver()
    out = {}
    for m, n in ((12, 60), (110, 50)):
        assert L._lib.lib().lpx_packed_fits(m, n) == 1
        cs, As, b0s = covering_models(1, m, n)
        c0, A, b0 = cs[0], As[0], b0s[0]
        rel = np.ones(m, dtype=np.int32)
        for count in (256, 4096, 65536):
            g = np.random.default_rng(7)
            costs = c0 * g.uniform(0.8, 1.2, size=(count, n))
            rhs = b0 * g.uniform(0.8, 1.2, size=(count, m))
            for with_b in (False, True):
                bs = rhs if with_b else None
                rounds = big_reps if count == 65536 else reps
                sides = {"cold": [], "kept": []}
                with S.OpenPackedBase(c0, A, b0, rel, 1.0, sense="min") as kept:
                    for i in range(rounds + 1):
                        ms, rc = _timed(lambda: S.SolvePackedDual(costs, A, rhs if with_b else b0, rel, 1.0, sense="min"))
                        sides["cold"].append(ms)
                        ms, rw = _timed(lambda: kept.solve_costs(costs, bs))
                        sides["kept"].append(ms)
                        assert (rc.Status == 0).all() and (rw.Status == 0).all(), "a scenario is not OPTIMAL"
                        assert (np.abs(rw.OptimalValue - rc.OptimalValue) <= 1e-9 * np.maximum(1.0, np.abs(rc.OptimalValue))).all()
                rec = {"shape": [m + 1, n + m + 1], "count": count, "with_b": with_b,
                       "events_per_scenario_cold": float(rc.Events.mean()), "events_per_scenario_kept": float(rw.Events.mean()),
                       "primal_events_per_scenario": float(rw.PrimalEvents.mean()), "dual_events_per_scenario": float(rw.DualEvents.mean())}
                rec.update({k: stats(v[1:]) for k, v in sides.items()})         # the first round is the warm-up
                rec["winner"] = verdict(rec["kept"], rec["cold"], "kept", "cold")
                rec["cold_over_kept"] = rec["cold"]["median_ms"] / rec["kept"]["median_ms"]
                out["%dx%d count %d %s" % (m + 1, n + m + 1, count, "c and b" if with_b else "c")] = rec
                print(json.dumps({"row": list(out)[-1], **rec}), file=sys.stderr, flush=True)
    if parent_lib:
        out["packed_base_solve_tree_vs_parent"] = packed_warm_parent(reps, parent_lib)
    return out


def main():
    L._lib.check(L._lib.lib().lpx_init(0))
    out = {}
    if OPT["compare_costs"]:
        print(json.dumps(compare_costs(OPT["reps"], OPT["big_reps"], OPT["parent_lib"])))
        return
    if OPT["compare_warm"] or OPT["warm_trace"]:
        print(json.dumps(compare_warm(OPT["reps"], OPT["big_reps"], OPT["warm_trace"])))
        return
    if OPT["compare_packed"] or OPT["packed_trace"]:
        print(json.dumps(compare_packed(OPT["reps"], OPT["packed_trace"], OPT["parent_lib"])))
        return
    if OPT["trace_only"]:
        out["a"] = leg_a(1, [(256, 768)], warm=0)
    else:
        if "a" in OPT["legs"]:
            out["a"] = leg_a(OPT["reps"], [(256, 768), (1024, 2048)])
        if "b" in OPT["legs"]:
            out["b"] = leg_b(OPT["reps"], OPT["big_reps"], OPT["skip_big"])
        if "c" in OPT["legs"]:
            out["c"] = leg_c(OPT["reps"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
