#!/usr/bin/env python3
"""Differential of the B&B host code (csrc/host/bnb.cpp, bnb_nodes.cpp, knapsack.cpp, sharded.h) between two builds of liblpx.so.

    python tools/diff_bnb_host.py OLD/liblpx.so NEW/liblpx.so            # through the test seams: no GPU needed
    python tools/diff_bnb_host.py OLD/liblpx.so NEW/liblpx.so --device   # on the GPU, the rolling batches in every form

The suite pins optima, counts and the agreement between ranks; it does not pin the whole node log of the level searches.  This
tool does, against another build: for each library a FRESH child process (LPX_LIB_PATH) runs a fixed list of seeded instances and
the parent compares, bit for bit, NodeLog, NodeZ, Nodes, LpSolves, Stats["pivots"], OptimalValue, Solution, Aux (knapsack: its
counters in NodeZ and x in Extra), the number of calls of the all-reduce callback and the length of every vector it was handed.
Every environment form is a process of its own (the LPX_ROLL_* switches are read once per process), each under a time limit.
Exit status 0: every comparison equal.

The sharded code path of a single process: lpx_solve sets `shard_one` only for the library's own communicator (LPX_COMM_SHARD_ONE,
which needs RCCL), never beside a callback.  What a callback reaches alone is one rank of a world of two whose peer never
answers: the callback is the identity, so that rank sees its own vectors come back.  The replicated warm-up, the fingerprint, the
hand-out, the exchange vector with its pool sizes and the publication of x all run; both ranks are driven that way.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEVICE_ENVS = (("default", {}),
               ("rolling sets", {"LPX_WARM_RESIDENT": "0", "LPX_ROLL_BATCH": "4"}),
               ("synchronous rolling", {"LPX_WARM_RESIDENT": "0", "LPX_ROLL_BATCH": "4", "LPX_ROLL_PIPELINE": "0"}),
               ("three rolling sets", {"LPX_WARM_RESIDENT": "0", "LPX_ROLL_BATCH": "4", "LPX_ROLL_SETS": "3"}))


def bits(a):
    import numpy as np
    return np.asarray([] if a is None else a, np.float64).reshape(-1).view(np.uint64).tolist()


def record(r, calls):
    import numpy as np
    log = np.asarray(r.NodeLog).reshape(-1, 3)
    return {"NodeLog": log.tolist(), "NodeZ": bits(r.NodeZ), "Nodes": int(r.Nodes), "LpSolves": int(r.LpSolves),
            "pivots": int(r.Stats["pivots"]), "OptimalValue": bits([r.OptimalValue]), "Solution": bits(r.Solution),
            "Extra": bits(r.Extra), "Aux": bits(r.Aux), "allreduce_calls": len(calls), "allreduce_lengths": list(calls),
            "max_depth": int(log[:, 0].max()) if len(log) else -1}


def run_case(out, name, solve):
    """solve(callback) -> result; the callback is the identity and records the length of every vector"""
    import linear_programming_solver_lpr381_amd as L
    calls = []

    def identity(vals):
        calls.append(len(vals))
        return vals
    try:
        out[name] = record(solve(identity), calls)
    except (L.SolverException, L.LpxError) as e:
        out[name] = {"error": str(e), "allreduce_calls": len(calls), "allreduce_lengths": list(calls)}


def seam_cases(out):
    import numpy as np
    import linear_programming_solver_lpr381_amd as L
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _dist_worker import make_knap_relax, node_lp
    for seed in (5, 6, 7):                 # the 9-variable, 4-row 0/1 program of tests/test_distributed_cpu.py (its seed: 5)
        g = np.random.default_rng(seed)
        n, m = 9, 4
        A = g.integers(0, 10, size=(m, n)).astype(float)
        b = np.floor(0.5 * A.sum(axis=1))
        c = g.integers(1, 21, size=n).astype(float)
        Af = np.vstack([A, np.eye(n)]); bf = np.concatenate([b, np.ones(n)])
        p = L.LPProblem.from_arrays(0, c, Af, np.zeros(m + n, int), bf)
        for mode in (0, 1):
            forms = [("dfs", dict(bnb_search=0)), ("level w1", dict(bnb_search=1, concurrent_nodes=1)),
                     ("level w3", dict(bnb_search=1, concurrent_nodes=3)), ("dive w2", dict(bnb_search=1, bnb_dive=1, concurrent_nodes=2))]
            forms += [(f"level budget {k}", dict(bnb_search=1, concurrent_nodes=2, max_nodes=k)) for k in range(1, 13)]
            for name, kw in forms:
                run_case(out, f"seam seed {seed} mode {mode} {name}",
                         lambda cb, kw=kw: L.BranchAndBound(bnb_mode=mode, test_node_lp=node_lp, **kw).Solve(p))
            for rank in (0, 1):
                for name, kw in (("level", dict(concurrent_nodes=2)), ("dive", dict(bnb_dive=1, concurrent_nodes=1)),
                                 ("budget 5", dict(concurrent_nodes=2, max_nodes=5))):
                    run_case(out, f"seam seed {seed} mode {mode} lone rank {rank} of 2 {name}",
                             lambda cb, kw=kw: L.BranchAndBound(bnb_mode=mode, bnb_search=1, rank=rank, world=2, allreduce_max=cb,
                                                                test_node_lp=node_lp, **kw).Solve(p))
    g = np.random.default_rng(31)          # the knapsack of tests/_dist_worker.py, drawn after its B&B instance
    g.integers(0, 10, size=(6, 14)); g.integers(1, 21, size=14)
    kn = 60
    w = g.integers(1, 60, size=kn).astype(float)
    pr = w + g.integers(0, 12, size=kn)
    cap = float(np.floor(0.5 * w.sum()))
    kp = L.LPProblem(L.Sense.Max, pr.tolist(), [L.Constraint(w.tolist(), L.Rel.LE, cap)])
    relax = make_knap_relax(pr, w, cap)
    run_case(out, "seam knapsack plain", lambda cb: L.BranchAndBoundKnapsack(test_knap_relax=relax).Solve(kp))
    run_case(out, "seam knapsack budget 40", lambda cb: L.BranchAndBoundKnapsack(test_knap_relax=relax, max_nodes=40).Solve(kp))
    for rank in (0, 1):
        run_case(out, f"seam knapsack lone rank {rank} of 2",
                 lambda cb: L.BranchAndBoundKnapsack(rank=rank, world=2, allreduce_max=cb, test_knap_relax=relax).Solve(kp))


def device_cases(out):
    import linear_programming_solver_lpr381_amd as L
    from linear_programming_solver_lpr381_amd import synth
    L._lib.check(L._lib.lib().lpx_init(0))
    # small; a dive past depth 32 (a second capacity class of handles); node tableaux of 1.2 MB, which the streaming kernels roll
    for name, (n, m, seed), kw in (("binary_ip(32, 16)", (32, 16, 1), dict()),
                                   ("deep binary_ip(96, 3)", (96, 3, 2), dict(bnb_dive=1, max_nodes=2000)),
                                   ("rolling binary_ip(200, 100)", (200, 100, 5), dict(max_nodes=300))):
        c, A, rel, b = synth.binary_ip(n, m, seed)
        p = L.LPProblem.from_arrays(0, c, A, rel, b)
        for search in (1, 2):
            if search == 1 and n == 200:
                continue                   # cold nodes of that size take seconds each and never roll
            run_case(out, f"device {name} search {search}",
                     lambda cb: L.BranchAndBound(bnb_mode=1, bnb_search=search, concurrent_nodes=4, **kw).Solve(p))


def child(kind, path):
    out = {}
    (seam_cases if kind == "seam" else device_cases)(out)
    with open(path, "w") as f:
        json.dump(out, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old"); ap.add_argument("new")
    ap.add_argument("--device", action="store_true", help="run the device instances (needs a GPU) instead of the seam instances")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.old)
    import tempfile
    kind = "device" if a.device else "seam"
    different = 0
    for env_name, env in (DEVICE_ENVS if a.device else (("seam", {}),)):
        res = []
        for lib in (a.old, a.new):
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "out.json")
                e = dict(os.environ, LPX_LIB_PATH=os.path.abspath(lib), PYTHONPATH=ROOT, **env)
                subprocess.run([sys.executable, os.path.abspath(__file__), path, "-", "--child", kind], env=e, check=True, timeout=a.timeout)
                res.append(json.load(open(path)))
        old, new = res
        assert old.keys() == new.keys() and old
        for case in old:
            bad = [k for k in old[case] if old[case][k] != new[case].get(k)]
            different += bool(bad)
            o = old[case]
            what = (f"error {o['error']!r}" if "error" in o else
                    f"{len(o['NodeLog'])} log rows, depth {o['max_depth']}, {o['LpSolves']} LPs, {o['pivots']} pivots")
            print(f"[{env_name}] {case}: {'DIFFERENT in ' + ', '.join(bad) if bad else 'equal'} ({what}, "
                  f"{o['allreduce_calls']} all-reduces)", flush=True)
    print(f"{kind}: {'every comparison equal' if not different else str(different) + ' cases DIFFER'}")
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
