"""Probe: warm post-optimal edits on the device (lpx_postopt.hip, lpx_session_*).

Part 1 -- the two combinations at their widest on the headline tableau (4097 x 12289, synth.dense_lp(4096, 8192) after 200
primal pivots): the objective update with all m rows as terms (K = m, the whole 403 MB tableau read once) and the RHS update
with all m slack columns as terms (K = m, the 134 MB slack block).  Host wall per call (each call waits for its result); kernel
times come from running this probe under `rocprofv3 --kernel-trace --stats` (po_row_pass / po_row_combine, po_col_pass /
po_col_combine).

Part 2 -- the session (LPSolver.Open) at config-2 size (dense_lp(1024, 2048)) and at one larger shape: per kind of edit
(one right-hand side, one cost, a new variable, a new constraint cutting the current optimum), the host wall of the first
edit and the median of the following ones, against a cold lpx_solve ("Primal Simplex": every model stays all-<= with b >= 0)
of the model as edited.  Prints one JSON line.

usage: probe_postopt.py [REPS] [EDITS] [BIG_M BIG_N]"""
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


def ms(t0):
    return 1e3 * (time.perf_counter() - t0)


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": len(ts)}


def part1(reps):
    c, A, b = synth.dense_lp(4096, 8192)
    T0, basis0 = synth.primal_tableau_from(c, A, b)
    del A
    R, C = T0.shape
    m, n = R - 1, C - R
    g = np.random.default_rng(1)
    out = {"shape": [R, C]}
    with L.DeviceTableau.from_host(T0, basis0) as dt:
        del T0
        dt.primal_run(max_iter=200)
        dt.snapshot()
        rows, w = np.arange(m, dtype=np.int32), 1e-3 * g.standard_normal(m)
        cols, v = np.arange(n, n + m, dtype=np.int32), 1e-3 * g.standard_normal(m)
        for name, fn, nbytes in (("objective_update_K_m", lambda: dt.objective_update(rows, w), 8 * m * C),
                                 ("rhs_update_K_m", lambda: dt.rhs_update(cols, v), 8 * R * m)):
            ts = []
            for i in range(reps + 2):
                dt.restore()
                t0 = time.perf_counter()
                fn()
                if i >= 2:
                    ts.append(ms(t0))
            out[name] = dict(stats(ts), bytes_read=nbytes)
        ts = []
        Th = np.empty((R, C))
        for i in range(3):
            t0 = time.perf_counter()
            Th, bh = dt.download()
            t1 = time.perf_counter()
            dt.upload(Th, bh)
            ts.append((1e3 * (t1 - t0), ms(t1)))
        out["host_route_transfers_ms"] = {"download": min(t[0] for t in ts), "upload": min(t[1] for t in ts)}
    return out


def edit(ses, kind, rng):
    p = ses.Problem
    if kind == "rhs":
        i = int(rng.integers(0, len(p.Constraints)))
        return ses.ChangeRHS(i, p.Constraints[i].B * float(rng.uniform(0.95, 1.05)))
    if kind == "cost":
        j = int(rng.integers(0, p.NumVars))
        return ses.ChangeCost(j, p.C[j] * float(rng.uniform(0.9, 1.1)))
    if kind == "add_variable":
        return ses.AddActivity(float(rng.uniform(1.0, 1.5)), rng.random(len(p.Constraints)))
    a = rng.random(p.NumVars)
    return ses.AddConstraint(a, 0, float(a @ ses.Result.Solution) * 0.999)


def part2(m, n, edits):
    c, A, b = synth.dense_lp(m, n)
    prob = L.LPProblem.from_arrays(0, c, A, [0] * m, b)
    out = {"shape": [m, n]}
    t0 = time.perf_counter()
    cold0 = L.LPSolver().Solve(prob, "Primal Simplex")
    out["cold_solve_ms"] = ms(t0)
    out["cold_pivots"] = len(cold0.Trace)
    for kind in ("rhs", "cost", "add_variable", "add_constraint"):
        rng = np.random.default_rng(7)
        t0 = time.perf_counter()
        with L.LPSolver().Open(prob, extra_rows=edits + 4, extra_cols=edits + 4) as ses:
            open_ms = ms(t0)
            warmup_ms = ses.Result.Aux[1]
            ts, piv, warm = [], [], []
            for e in range(edits):
                t0 = time.perf_counter()
                r = edit(ses, kind, rng)
                ts.append(ms(t0))
                piv.append(len(r.Trace))
                warm.append(r.Aux[0])
            t0 = time.perf_counter()
            cold = L.LPSolver().Solve(ses.Problem, "Primal Simplex")
            cold_ms = ms(t0)
            assert cold.Status == r.Status == 0
            rel = abs(cold.OptimalValue - r.OptimalValue) / max(1.0, abs(cold.OptimalValue))
        out[kind] = {"open_ms": open_ms, "open_dual_setup_ms": warmup_ms, "first_ms": ts[0],
                     "steady": stats(ts[1:]), "pivots": piv, "all_warm": all(w == 1.0 for w in warm),
                     "cold_of_edited_ms": cold_ms, "cold_of_edited_pivots": len(cold.Trace), "z_rel_diff": rel}
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    edits = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    big = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (1536, 3072)
    L._lib.check(L._lib.lib().lpx_init(0))
    out = {"tableau_ops": part1(reps), "config2": part2(1024, 2048, edits)}
    try:
        out["larger"] = part2(big[0], big[1], edits)
    except L.SolverException as e:
        out["larger"] = {"shape": list(big), "error": str(e)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
