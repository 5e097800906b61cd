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

`--compare-forms` measures the on-chip form of the bounded primal loop (lpx_bounded_run2 with LPX_NODE_ONCHIP)
against the launches form (lpx_bounded_run), by the rule of DESIGN section 4.17: host wall, median with min and max, the sides
alternating in one process, and a side wins iff its median lies below the other's minimum.  Root solves: binary_ip(60, 12),
binary_ip(128, 64) without their bound rows and dense_lp(64, 128), every u_j = 1, one handle each, a timed run starting from a
restored snapshot.  The batch, three ways: 256 models of 13 x 73 through lpx_solve_bounded_batch, as 256 single on-chip solves and
as 256 launches-form solves (lpx_solve_bounded), whole calls timed.  `--forms-trace` runs one warm on-chip solve per root model and
one batch, for a run of its own under `rocprofv3 --kernel-trace --stats`: one kernel per solve and one per batch.

`--compare-packed` measures the packed batch call (lpx_solve_packed) by the same rule: the 256 models of the
batch above with u = 1 four ways, alternating in one process, whole calls timed (SolvePacked, SolveBoundedBatch, 256 single on-chip
solves, 256 launches-form solves; equal optima and counts asserted); then SolvePacked alone on 4096 and 65536 models of that shape;
then 4096 right-hand sides of one shared model (stride 0) against the same 4096 fully packed.  `--packed-trace` makes four packed
calls of 256 models, for a run of its own under `rocprofv3 --kernel-trace --stats`: one kernel per call.

usage: bench_bounded.py [--trace-only] [--model NAME] [--compare-forms | --forms-trace | --compare-packed | --packed-trace] [REPS]"""
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


def form_models():
    for n, m in ((60, 12), (128, 64)):
        c, A, rel, b = synth.binary_ip(n, m)
        yield "binary_bounded_%dx%d" % (n, m), c, A[:m], b[:m]
    c, A, b = synth.dense_lp(64, 128)
    yield "dense_unit_64x128", c, A, b


def verdict(a, b, na, nb):
    """The rule of DESIGN section 4.17: a side wins iff its median lies below the other's minimum."""
    if a["median_ms"] < b["min_ms"]:
        return na
    if b["median_ms"] < a["min_ms"]:
        return nb
    return "tie"


def batch_models(count):
    ps = []
    for s in range(1, count + 1):
        c, A, rel, b = synth.binary_ip(60, 12, s)
        ps.append(L.LPProblem.from_arrays(0, c, A[:12], [0] * 12, b[:12]))
    return ps


def compare_forms(reps, trace):
    out = {}
    for name, c, A, b in form_models():
        m, n = A.shape
        T, basis = synth.primal_tableau_from(c, A, b)
        ub = np.full(T.shape[1] - 1, np.inf); ub[:n] = 1.0
        with L.DeviceTableau.from_host(T, basis) as dt:
            dt.set_bounds(ub)
            dt.snapshot()
            tl, tc = [], []
            for i in range(1 + 2 if trace else reps + 2):
                if not trace:
                    dt.restore()
                    t0 = time.perf_counter()
                    sl, stl = dt.bounded_run()
                    if i >= 2:
                        tl.append(1e3 * (time.perf_counter() - t0))
                    kl, zl = dt.bounded_counts(), dt.bounded_solution(n)[1]
                dt.restore()
                t0 = time.perf_counter()
                sc, stc = dt.bounded_run(form="onchip")
                if i >= 2:
                    tc.append(1e3 * (time.perf_counter() - t0))
            kc, zc = dt.bounded_counts(), dt.bounded_solution(n)[1]
            rec = {"shape": list(T.shape), "events": sum(kc), "counts": list(kc), "status": sc, "z": zc,
                   "onchip": dict(stats(tc), launches=stc["launches"])}
            if not trace:
                assert (sl, kl, zl) == (sc, kc, zc), "the forms differ"
                rec["launches"] = dict(stats(tl), launches=stl["launches"])
                rec["launches_over_onchip"] = rec["launches"]["median_ms"] / rec["onchip"]["median_ms"]
                rec["winner"] = verdict(rec["launches"], rec["onchip"], "launches", "onchip")
        out[name] = rec
    count = 256
    ps = batch_models(count)
    S = L.LPSolver()
    tb, ts, tl = [], [], []
    for i in range(1 + 1 if trace else reps + 1):
        t0 = time.perf_counter()
        rb = S.SolveBoundedBatch(ps, [1.0] * count)
        if i >= 1:
            tb.append(1e3 * (time.perf_counter() - t0))
        if trace:
            continue
        t0 = time.perf_counter()
        rs = [S.SolveBounded(p, 1.0, form="onchip") for p in ps]
        if i >= 1:
            ts.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        rl = [S.SolveBounded(p, 1.0) for p in ps]
        if i >= 1:
            tl.append(1e3 * (time.perf_counter() - t0))
        assert all(a.OptimalValue == b.OptimalValue == c.OptimalValue and a.BoundCounts == b.BoundCounts == c.BoundCounts
                   for a, b, c in zip(rb, rs, rl)), "the three ways differ"
    rec = {"count": count, "shape": [13, 73], "events": int(sum(sum(r.BoundCounts) for r in rb)), "batch": stats(tb)}
    if not trace:
        rec["single_onchip"] = stats(ts); rec["single_launches"] = stats(tl)
        rec["winner_batch_vs_single_onchip"] = verdict(rec["batch"], rec["single_onchip"], "batch", "single_onchip")
        rec["winner_batch_vs_single_launches"] = verdict(rec["batch"], rec["single_launches"], "batch", "single_launches")
        rec["winner_single_onchip_vs_single_launches"] = verdict(rec["single_onchip"], rec["single_launches"], "single_onchip", "single_launches")
    out["batch_256_of_13x73"] = rec
    if not trace:
        # the same 256 LPs on handles that exist already (tableau level): the restores are not timed, each side's runs are
        hs = []
        for s in range(1, count + 1):
            c, A, rel, b = synth.binary_ip(60, 12, s)
            T, basis = synth.primal_tableau_from(c, A[:12], b[:12])
            ub = np.full(T.shape[1] - 1, np.inf); ub[:60] = 1.0
            dt = L.DeviceTableau.from_host(T, basis)
            dt.set_bounds(ub); dt.snapshot()
            hs.append(dt)
        sides = {"batch": [], "single_onchip": [], "single_launches": []}
        with L.NodeBatch(hs) as nb:
            slots = list(range(count))
            for i in range(reps + 2):
                for side, ts in sides.items():
                    for dt in hs:
                        dt.restore()
                    for dt in hs[:16]:          # the handles borrow a few pool streams round robin: this waits for every restore
                        dt.bound_flags()
                    t0 = time.perf_counter()
                    if side == "batch":
                        recs = nb.solve(slots)
                    else:
                        for dt in hs:
                            dt.bounded_run(form="onchip" if side == "single_onchip" else "launches")
                    if i >= 2:
                        ts.append(1e3 * (time.perf_counter() - t0))
        for dt in hs:
            dt.close()
        rec = {"count": count, "shape": [13, 73], "events": int(sum(r["events"] for r in recs))}
        rec.update({k: stats(v) for k, v in sides.items()})
        rec["winner_batch_vs_single_onchip"] = verdict(rec["batch"], rec["single_onchip"], "batch", "single_onchip")
        rec["winner_batch_vs_single_launches"] = verdict(rec["batch"], rec["single_launches"], "batch", "single_launches")
        out["handles_256_of_13x73"] = rec
    print(json.dumps(out))


def packed_arrays(count):
    """The models of batch_models(256) as packed arrays, repeated up to count models."""
    cs, As, bs = [], [], []
    for s in range(1, min(count, 256) + 1):
        c, A, rel, b = synth.binary_ip(60, 12, s)
        cs.append(c); As.append(A[:12]); bs.append(b[:12])
    c, A, b = np.stack(cs), np.stack(As), np.stack(bs)
    reps = -(-count // len(cs))
    return tuple(np.ascontiguousarray(np.tile(v, (reps,) + (1,) * (v.ndim - 1))[:count]) for v in (c, A, b))


def compare_packed(reps, trace):
    """The packed call (lpx_solve_packed) against the three ways of --compare-forms on the same 256 models,
    whole calls timed and the four alternating in one process; then the packed call alone on 4096 and 65536 models of that shape;
    then 4096 right-hand sides of ONE shared model (stride 0) against the same 4096 fully packed."""
    S = L.LPSolver()
    count = 256
    c, A, b = packed_arrays(count)
    if trace:                                           # one warm-up call and three calls: one kernel each in the trace
        for i in range(4):
            r = S.SolvePacked(c, A, b, 1.0)
        print(json.dumps({"packed_trace": {"count": count, "calls": 4, "events": int(r.Events.sum()), "launches_per_call": r.Stats["launches"]}}))
        return
    out = {}
    ps = batch_models(count)
    sides = {"packed": [], "batch": [], "single_onchip": [], "single_launches": []}
    for i in range(reps + 1):
        t0 = time.perf_counter()
        rp = S.SolvePacked(c, A, b, 1.0)
        sides["packed"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        rb = S.SolveBoundedBatch(ps, [1.0] * count)
        sides["batch"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        rs = [S.SolveBounded(p, 1.0, form="onchip") for p in ps]
        sides["single_onchip"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        rl = [S.SolveBounded(p, 1.0) for p in ps]
        sides["single_launches"].append(1e3 * (time.perf_counter() - t0))
        assert all(rp.OptimalValue[k] == x.OptimalValue == y.OptimalValue == z.OptimalValue and
                   tuple(rp.BoundCounts[k].tolist()) == x.BoundCounts == y.BoundCounts == z.BoundCounts and rp.Status[k] == x.Status
                   for k, (x, y, z) in enumerate(zip(rb, rs, rl))), "the four ways differ"
    rec = {"count": count, "shape": [13, 73], "events": int(rp.Events.sum()), "loop_ms_last": rp.Stats["loop_ms"],
           "bytes_in": int(c.nbytes + A.nbytes + b.nbytes + 8 * 60), "bytes_out": int(count * (4 + 8 * 60 + 8 + 40 + 4 * 12 + 60))}
    rec.update({k: stats(v[1:]) for k, v in sides.items()})                     # the first round is the warm-up
    for other in ("batch", "single_onchip", "single_launches"):
        rec["winner_packed_vs_" + other] = verdict(rec["packed"], rec[other], "packed", other)
        rec[other + "_over_packed"] = rec[other]["median_ms"] / rec["packed"]["median_ms"]
    out["four_ways_256_of_13x73"] = rec
    for count in (4096, 65536):
        c, A, b = packed_arrays(count)
        ts, loop = [], []
        for i in range(min(reps, 7) + 1):
            t0 = time.perf_counter()
            r = S.SolvePacked(c, A, b, 1.0)
            ts.append(1e3 * (time.perf_counter() - t0)); loop.append(r.Stats["loop_ms"])
        assert (r.Status == 0).all() and np.array_equal(r.OptimalValue[:256], rp.OptimalValue) and np.array_equal(r.OptimalValue[-256:], rp.OptimalValue)
        out["packed_%d_of_13x73" % count] = dict(stats(ts[1:]), count=count, bytes_in=int(c.nbytes + A.nbytes + b.nbytes + 8 * 60),
                                                 loop_ms_median=statistics.median(loop[1:]),
                                                 us_per_model=1e3 * statistics.median(ts[1:]) / count)
    # one shared model, 4096 right-hand sides: stride 0 for c and A against the same data tiled
    count = 4096
    c1, A1, b1 = packed_arrays(1)
    g = np.random.default_rng(5)
    bs = np.floor(b1[0] * g.uniform(0.8, 1.2, size=(count, 12)))
    ct, At = np.ascontiguousarray(np.tile(c1, (count, 1))), np.ascontiguousarray(np.tile(A1, (count, 1, 1)))
    sides = {"shared": [], "tiled": []}
    for i in range(reps + 1):
        t0 = time.perf_counter()
        rsh = S.SolvePacked(c1[0], A1[0], bs, 1.0)
        sides["shared"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        rti = S.SolvePacked(ct, At, bs, 1.0)
        sides["tiled"].append(1e3 * (time.perf_counter() - t0))
        assert rsh.Solution.tobytes() == rti.Solution.tobytes() and rsh.OptimalValue.tobytes() == rti.OptimalValue.tobytes() and \
            np.array_equal(rsh.BoundCounts, rti.BoundCounts) and np.array_equal(rsh.Status, rti.Status), "shared and tiled differ"
    rec = {"count": count, "shape": [13, 73], "events": int(rsh.Events.sum()), "bytes_in_shared": int(c1[0].nbytes + A1[0].nbytes + bs.nbytes + 8 * 60),
           "bytes_in_tiled": int(ct.nbytes + At.nbytes + bs.nbytes + 8 * 60)}
    rec.update({k: stats(v[1:]) for k, v in sides.items()})
    rec["winner"] = verdict(rec["shared"], rec["tiled"], "shared", "tiled")
    out["rhs_4096_shared_vs_tiled"] = rec
    print(json.dumps(out))


def main():
    if "--compare-packed" in sys.argv[1:] or "--packed-trace" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a not in ("--compare-packed", "--packed-trace")]
        L._lib.check(L._lib.lib().lpx_init(0))
        return compare_packed(int(rest[0]) if rest else 15, "--packed-trace" in sys.argv[1:])
    if "--compare-forms" in sys.argv[1:] or "--forms-trace" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a not in ("--compare-forms", "--forms-trace")]
        L._lib.check(L._lib.lib().lpx_init(0))
        return compare_forms(int(rest[0]) if rest else 15, "--forms-trace" in sys.argv[1:])
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
