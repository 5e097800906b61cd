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

`--trace-only` runs leg (a) on the smaller model once per side (no untimed run in front), for a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_bounded_long.py --trace-only`, whose kernel table gives the mean launch
time of lpx_bounded_long_select, lpx_bounded_dual_select and the lpx_update launches they feed.

usage: bench_bounded_long.py [--leg a|b|c]... [--root DIR] [--big-reps N] [--skip-big] [--trace-only] [REPS]"""
import json
import os
import statistics
import sys
import time


def _args():
    a = sys.argv[1:]
    opt = {"legs": [], "root": None, "big_reps": 2, "skip_big": False, "trace_only": False, "reps": 7}
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
        else:
            opt["reps"] = int(a[i]); i += 1
    if not opt["legs"]:
        opt["legs"] = ["a", "b", "c"]
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


def main():
    L._lib.check(L._lib.lib().lpx_init(0))
    out = {}
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
