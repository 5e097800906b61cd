"""Bounds as rows against bounds beside the tableau, host wall per solve on the device.

For each model -- the config-4 root LP (synth.binary_ip(512, 256), 0/1 bounds) and synth.dense_lp(1024, 2048) with every
u_j = 1 -- two sides solve the same LP from the slack basis:
  (a) rows:    the bounds as explicit rows x_j <= 1, lpx_primal_run (the only way before the bounded loop existed)
  (b) bounded: the bounds beside the tableau, lpx_bounded_run
Profiler off, both handles warm (two untimed runs each), the sides alternating, REPS timed runs each; a timed run starts from
a restored snapshot (the restore is not timed) and ends when the run call returns, which is after the device has finished.
Prints one JSON line: median / min / max milliseconds per side, the pivot and event counts, launches.

`--trace-only` runs side (b) alone (two warm-up runs and REPS runs), for a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_bounded.py --trace-only`, whose kernel table gives the mean launch time
of lpx_bounded_select and of the lpx_update launches it feeds.

`--model NAME` keeps one of the two models (config4_root, dense_1024x2048_u1), so that a trace covers one shape.

usage: bench_bounded.py [--trace-only] [--model NAME] [REPS]"""
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
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": len(ts)}


def main():
    args = [a for a in sys.argv[1:] if a != "--trace-only"]
    trace_only = "--trace-only" in sys.argv[1:]
    only = None
    if "--model" in args:
        k = args.index("--model")
        only = args[k + 1]
        del args[k:k + 2]
    reps = int(args[0]) if args else 7
    L._lib.check(L._lib.lib().lpx_init(0))
    out = {}
    for name, c, A, b in models():
        if only is not None and name != only:
            continue
        m, n = A.shape
        Tb, bb = synth.primal_tableau_from(c, A, b)
        ub = np.full(Tb.shape[1] - 1, np.inf); ub[:n] = 1.0
        rec = {"bounded_shape": list(Tb.shape)}
        with L.DeviceTableau.from_host(Tb, bb) as db:
            db.set_bounds(ub)
            db.snapshot()
            dr = None
            if not trace_only:
                Tr, br = synth.primal_tableau_from(c, np.vstack([A, np.eye(n)]), np.concatenate([b, np.ones(n)]))
                rec["rows_shape"] = list(Tr.shape)
                dr = L.DeviceTableau.from_host(Tr, br)
                dr.snapshot()
                del Tr
            ta, tb = [], []
            for i in range(reps + 2):
                if dr is not None:
                    dr.restore()
                    t0 = time.perf_counter()
                    sa, sta = dr.primal_run()
                    if i >= 2:
                        ta.append(1e3 * (time.perf_counter() - t0))
                db.restore()
                t0 = time.perf_counter()
                sb, stb = db.bounded_run()
                if i >= 2:
                    tb.append(1e3 * (time.perf_counter() - t0))
            k0, k1, fl = db.bounded_counts()
            zb = db.bounded_solution(n)[1]
            rec["bounded"] = dict(stats(tb), status=sb, pivots_to_zero=k0, pivots_to_upper=k1, flips=fl, events=k0 + k1 + fl,
                                  launches=stb["launches"], z=zb)
            if dr is not None:
                zr = dr.download()[0][-1, -1]
                rec["rows"] = dict(stats(ta), status=sa, pivots=sta["pivots"], launches=sta["launches"], z=float(zr))
                rec["rel_diff_z"] = abs(zb - zr) / max(1.0, abs(zr))
                rec["rows_over_bounded"] = rec["rows"]["median_ms"] / rec["bounded"]["median_ms"]
                dr.close()
        out[name] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
