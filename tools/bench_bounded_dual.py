"""Host wall per child re-solve after a bound change on a solved LP, three ways on the device.

For each model -- the config-4 root LP (synth.binary_ip(512, 256), 0/1 bounds) and synth.dense_lp(1024, 2048) with every
u_j = 1 -- the root is solved once per side, then the children x_j = 0 ("down") and x_j = 1 ("up") of its first three
fractional variables are re-solved:
  (a) rows:  the bounds as explicit rows; lpx_tableau_build_child (one more row on the parent's final tableau) + lpx_dual_run
  (b) cold:  bounds beside the tableau; lpx_tableau_set_bounds with the child's bound + lpx_bounded_run from the slack basis
             (down children only: set_bounds cannot express a lower bound)
  (c) warm:  bounds beside the tableau; lpx_tableau_change_bounds + lpx_bounded_dual_run from the root's final tableau
Profiler off, every handle warm (two untimed rounds over the children), the sides alternating, REPS timed rounds; a timed
re-solve starts from a restored snapshot where its side needs one (the restore is not timed) and ends when the run call returns,
which is after the device has finished.  Prints one JSON line: per side and direction the median / min / max milliseconds over
children and rounds, the event counts per child, launches, and the children's optima (the three sides must agree).

`--trace-only` runs side (c) alone, for a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_bounded_dual.py --trace-only`, whose kernel table gives the mean launch
time of lpx_bounded_dual_select, of the lpx_update launches it feeds and of the two lpx_bounds_* kernels.

`--model NAME` keeps one of the two models (config4_root, dense_1024x2048_u1).

usage: bench_bounded_dual.py [--trace-only] [--model NAME] [REPS]"""
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
    c, A, rel, b = synth.binary_ip(512, 256)
    yield "config4_root", c, A[:256], b[:256]
    c, A, b = synth.dense_lp(1024, 2048)
    yield "dense_1024x2048_u1", c, A, b


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "samples": len(ts)} if ts else None


def main():
    args = [a for a in sys.argv[1:] if a != "--trace-only"]
    trace_only = "--trace-only" in sys.argv[1:]
    only = None
    if "--model" in args:
        k = args.index("--model")
        only = args[k + 1]
        del args[k:k + 2]
    reps = int(args[0]) if args else 7
    lib = L._lib.lib()
    L._lib.check(lib.lpx_init(0))
    out = {}
    for name, c, A, b in models():
        if only is not None and name != only:
            continue
        m, n = A.shape
        Tb, bb = synth.primal_tableau_from(c, A, b)
        ub = np.full(Tb.shape[1] - 1, np.inf); ub[:n] = 1.0
        rec = {"bounded_shape": list(Tb.shape)}
        warm = L.DeviceTableau.from_host(Tb, bb)        # (c): solved once, its final state snapshotted
        warm.set_bounds(ub)
        st_root, root_stats = warm.bounded_run()
        x, z_root, _ = warm.bounded_solution(n)
        frac = [int(j) for j in np.flatnonzero(np.minimum(x, 1.0 - x) > 1e-6)[:3]]
        rec.update(root_status=st_root, root_events=sum(warm.bounded_counts()), root_z=z_root, branch_vars=frac)
        warm.snapshot()
        kids = [(j, v) for j in frac for v in (0.0, 1.0)]
        cold = rows = child = None
        if not trace_only:
            cold = L.DeviceTableau.from_host(Tb, bb)    # (b): the slack basis snapshotted, solved again for every child
            cold.set_bounds(ub)
            cold.snapshot()
            Tr, br = synth.primal_tableau_from(c, np.vstack([A, np.eye(n)]), np.concatenate([b, np.ones(n)]))
            rec["rows_shape"] = list(Tr.shape)
            rows = L.DeviceTableau.from_host(Tr, br)    # (a): the parent, solved once; every child is built from it
            st_rows, _ = rows.primal_run()
            rbasis = rows.download()[1]
            rec["rows_root_z"] = float(rows.download()[0][-1, -1])
            child = L.DeviceTableau(Tr.shape[0] + 1, Tr.shape[1] + 1)
            del Tr
        t = {"a_down": [], "a_up": [], "b_down": [], "c_down": [], "c_up": []}
        info = {}
        for i in range(reps + 2):
            for j, v in kids:
                d = "down" if v == 0.0 else "up"
                if rows is not None:
                    row = int(np.flatnonzero(rbasis == j)[0])
                    t0 = time.perf_counter()
                    L._lib.check(lib.lpx_tableau_build_child(child._h, rows._h, j, row, 0 if v == 0.0 else 1, v))
                    child.R, child.C = rows.R + 1, rows.C + 1
                    sa, sta = child.dual_run(fdf_guard=0)
                    if i >= 2:
                        t["a_" + d].append(1e3 * (time.perf_counter() - t0))
                    za = float(child.download()[0][-1, -1])
                    info.setdefault("a", {})[f"{j}_{d}"] = dict(status=sa, pivots=sta["pivots"], launches=sta["launches"], z=za)
                if cold is not None and v == 0.0:
                    cold.restore()
                    ubc = ub.copy(); ubc[j] = 0.0
                    t0 = time.perf_counter()
                    cold.set_bounds(ubc)
                    sb, stb = cold.bounded_run()
                    if i >= 2:
                        t["b_down"].append(1e3 * (time.perf_counter() - t0))
                    info.setdefault("b", {})[f"{j}_{d}"] = dict(status=sb, events=sum(cold.bounded_counts()), launches=stb["launches"],
                                                               z=cold.bounded_solution(n)[1])
                warm.restore()
                t0 = time.perf_counter()
                warm.change_bounds([j], v, v)
                sc, stc = warm.bounded_dual_run()
                if i >= 2:
                    t["c_" + d].append(1e3 * (time.perf_counter() - t0))
                k0, k1, _ = warm.bounded_counts()
                info.setdefault("c", {})[f"{j}_{d}"] = dict(status=sc, kind0=k0, kind1=k1, events=k0 + k1, launches=stc["launches"],
                                                           z=warm.bounded_solution(n)[1])
        rec["ms"] = {k: stats(v) for k, v in t.items()}
        rec["children"] = info
        if rows is not None:
            za = [info["a"][k]["z"] for k in sorted(info["c"])]
            zc = [info["c"][k]["z"] for k in sorted(info["c"])]
            rec["max_rel_diff_z_a_c"] = max(abs(p - q) / max(1.0, abs(p)) for p, q in zip(za, zc))
            for dt in (cold, rows, child):
                dt.close()
        warm.close()
        out[name] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
