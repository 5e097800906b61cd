"""Probe: the GMI cut round on the device (lpx_tableau_gmi_round) and the whole loop.

Part 1 -- the round alone on the headline tableau (4097 x 12289, synth.dense_lp(4096, 8192) after 200 primal pivots, every
column marked integer), in a handle with 64 spare rows and columns:
  * in place: restore the snapshot, one round of K cuts (no cut columns yet: no purge);
  * purge form: the first round's result with its K cut slacks basic at b = -1, and purge_tol = -2 so that the next round
    purges all K of them and appends K new cuts (one compacting pass into the second buffer plus the copy back).
Each call waits for its own results, so the figures are host wall time per round; kernel times come from running this probe
under `rocprofv3 --kernel-trace --stats` (gmi_scan, gmi_pick, gmi_apply_inplace, gmi_apply_purge).  The bytes each form
must move are computed from the shapes and the number of candidate rows.  The host route is timed for comparison: its
transfers (lpx_tableau_download into a reused buffer + lpx_tableau_upload), and apart from them the numpy round of
tests/_gmi_ref.py, a bit-exact restatement that is not optimised for speed.

Part 2 -- a full GMI solve of a random integer program at config-2 size (m = 1024, n = 2048, integer data, Max, <=), the
rounds driven from here so that each round's cut round and dual re-optimisation are timed apart (max_rounds rounds).
Prints one JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import linear_programming_solver_lpr381_amd as L
from linear_programming_solver_lpr381_amd import synth
import _gmi_ref as G


def ms(t0):
    return 1e3 * (time.perf_counter() - t0)


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": len(ts)}


def part1(reps, K):
    c, A, b = synth.dense_lp(4096, 8192)
    T0, basis0 = synth.primal_tableau_from(c, A, b)
    del A
    R, C = T0.shape
    first = C - 1
    is_int = np.ones(first, np.uint8)
    out = {"shape": [R, C], "tableau_bytes": 8 * R * C, "K": K}
    with L.DeviceTableau.with_capacity(T0, basis0, R + 64, C + 64) as dt:
        del T0
        dt.primal_run(max_iter=200)
        Th, bh = dt.download()
        f0 = Th[:-1, -1] - np.floor(Th[:-1, -1])
        ncand = int(np.sum((f0 >= 1e-3) & (f0 <= 1 - 1e-3)))
        dt.snapshot()
        o_in = L._lib.cut_opts(cuts_per_round=K)
        ts = []
        for i in range(reps + 3):
            dt.set_shape(R, C)
            dt.restore()
            t0 = time.perf_counter()
            src, pcol = dt.gmi_round(is_int, first, opts=o_in)
            if i >= 3:
                ts.append(ms(t0))
        assert len(src) == K and len(pcol) == 0
        out["inplace"] = stats(ts)
        # host route on the same tableau: download into a reused buffer (the third of three), numpy round, upload
        dt.set_shape(R, C)
        dt.restore()
        Th = np.empty((R, C)); bh = np.empty(R - 1, dtype=np.int32)
        dl = lambda: L._lib.check(L._lib.lib().lpx_tableau_download(dt._h, Th.ctypes.data_as(L._lib.dp), bh.ctypes.data_as(L._lib.ip)))
        dl(); dl()
        t0 = time.perf_counter(); dl(); t_dl = ms(t0)
        t0 = time.perf_counter()
        T2, b2, src2, _ = G.gmi_round(Th, bh, is_int, first, first, G.CutOpts(cuts_per_round=K), R + 64, C + 64)
        t_cpu = ms(t0)
        assert len(src2) == K
        dt.set_shape(*T2.shape)
        t0 = time.perf_counter(); dt.upload(T2, b2); t_ul = ms(t0)
        dt.set_shape(R, C)
        dt.restore()
        dt.gmi_round(is_int, first, opts=o_in)                  # the state the purge form starts from
        # the CPU round is tests/_gmi_ref.py, written for bit-exactness (a Python loop over the candidate rows), not for speed:
        # the transfers are the comparable part of the host route
        out["host_route_ms"] = {"download": t_dl, "upload": t_ul, "transfers": t_dl + t_ul,
                                "numpy_reference_round_unoptimised": t_cpu}
        # purge form: the state after one round, its K cut slacks purged by the next one
        dt.snapshot()
        o_pg = L._lib.cut_opts(cuts_per_round=K, purge_tol=-2.0)
        ts = []
        for i in range(reps + 3):
            dt.set_shape(R + K, C + K)
            dt.restore()
            t0 = time.perf_counter()
            src, pcol = dt.gmi_round(is_int, first, opts=o_pg)
            if i >= 3:
                ts.append(ms(t0))
        assert len(src) == K and len(pcol) == K
        out["purge"] = stats(ts)
    # bytes each form must move
    out["ncand"] = ncand
    out["bytes"] = {"scan": 8 * ncand * C,
                    "inplace_apply": 8 * ((2 * K + 2) * C + (R - 1) * (K + 2)),
                    "purge_apply_and_copy_back": 8 * (3 * (R + K) * (C + K) + K * C)}
    return out


def part2(max_rounds, K):
    rng = np.random.default_rng(2024)
    n, m = 2048, 1024
    c = rng.integers(1, 20, n).astype(float)
    A = rng.integers(0, 10, (m, n)).astype(float)
    b = rng.integers(2000, 6000, m).astype(float)
    T, basis = G.build_tableau(c, A, b)
    R, C = T.shape
    first = C - 1
    is_int = np.ones(first, np.uint8)
    o = L._lib.cut_opts(cuts_per_round=K)
    rounds = []
    with L.DeviceTableau.with_capacity(T, basis, R + 64, C + 64) as dt:
        t0 = time.perf_counter(); st, s = dt.primal_run(); t_root = ms(t0)
        z0 = dt.download()[0][-1, -1]
        for r in range(max_rounds):
            t0 = time.perf_counter(); src, pcol = dt.gmi_round(is_int, first, opts=o); t_cut = ms(t0)
            if len(src) == 0:
                break
            t0 = time.perf_counter(); st, s = dt.dual_run(fdf_guard=0, cleanup=1); t_dual = ms(t0)
            rounds.append({"cut_ms": t_cut, "dual_ms": t_dual, "pivots": s["pivots"], "added": len(src), "purged": len(pcol),
                           "shape": [dt.R, dt.C], "status": st})
            if st != 0:
                break
        z = dt.download()[0][-1, -1]
    return {"shape": [R, C], "root_ms": t_root, "root_z": z0, "final_z": z, "rounds": rounds,
            "cut_ms_median": statistics.median([x["cut_ms"] for x in rounds]) if rounds else None,
            "dual_ms_median": statistics.median([x["dual_ms"] for x in rounds]) if rounds else None}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    max_rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    L._lib.check(L._lib.lib().lpx_init(0))
    out = {"round_headline": part1(reps, 8), "solve_cfg2": part2(max_rounds, 8)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
