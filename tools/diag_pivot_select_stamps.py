"""Diagnostic (not part of the product): where do the two launches of the select-only step of the deferred-pivot primal loop
(lpx_pivot_ratio, the column launch, and lpx_pivot_select, the row launch; run_fused) spend their cycles?  Needs the -DLPX_STAMPS build (make -C linear_programming_solver_lpr381_amd/csrc stamps):

    LPX_LIB_PATH=.../csrc/build/liblpx_stamps.so python tools/diag_pivot_select_stamps.py [m n [pivots [depths]]]

Runs the bench LP (m = 4096, n = 8192: tableau 4097 x 12289) for `pivots` pivots (default 600) after a warm-up run of the same
length, once per depth (default 12 and 2; LPX_PIVOT_DEFER is read once per process, so each depth is a child process), and
prints cycles and microseconds per phase of workgroup 0's first wave, one table per kernel, each with the kernel's own
s_memrealtime span.  The stamps wait for that wave's loads at the end of the
phases that only issue loads, which serialises what the shipped kernel overlaps: the phases add up to more than the unstamped
launch takes (the kernel trace has that figure); they say where the time is, not how long the launch is.

    rocprofv3 --kernel-trace --stats ... -- python tools/diag_pivot_select_stamps.py --run 3000

is that kernel trace's workload: the same LP on whatever library is loaded, a warm-up run and one run of 3000 pivots.
`--run PIVOTS [m n [reps [profile_pivots]]]` with LPX_PIVOT_DEFER set is also a row of the depth table in DESIGN.md 4.1.
"""
import ctypes as C
import os
import subprocess
import sys

# row launch (and, above SELP_LDS_ROWS rows, the one-launch form lpx_pivot_select_ws, whose slots 1 - 3 are the column gather, the
# pending chain and the ratio store): lpx_g_stamps[8 + k]
# (the row launch of the pair: "barrier" is the exact scan behind a tie, ratios into LDS included, and runs only on the steps the
# last line counts; "scan" is the replay of the chain over the column launch's records.  Since r17 the operands that do not need r
# are issued in the first phase, which waits for them in this build: the shipped kernel leaves them in flight over the replay)
NAMES = ["record, shape, scan records (+ early operands)", "issue of the 3 loads behind r", "(one-launch form only)", "barrier / tie fallback", "scan (records or LDS)",
         "piv chain", "row loop", "block and hand-off reduction", "tail stores"]
# column launch: lpx_g_stamps[21 + k]
COL_NAMES = ["record load and leave tests", "round 2 (column, RHS, factors, scalars)", "chain, ratio and stores"]


def child(m, n, pivots):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import linear_programming_solver_lpr381_amd as L
    from linear_programming_solver_lpr381_amd import synth

    lib = L._lib.lib()
    L._lib.check(lib.lpx_init(0))
    c, A, b = synth.dense_lp(m, n, seed=synth.SEED)
    T, basis = synth.primal_tableau_from(c, A, b)
    del A
    dt = L.DeviceTableau.from_host(T, basis)
    dt.snapshot()
    opts = L.default_opts(False, use_graph=1, max_iter=pivots)
    dt.primal_run(opts)                                  # warm-up: clocks, graph capture, buffers
    dt.restore()
    hs = (C.c_ulonglong * 32)()
    lib.lpx_debug_hs(hs, 1)
    status, st = dt.primal_run(opts)
    lib.lpx_debug_hs(hs, 0)
    v = list(hs)[8:]
    calls, rt, npend = v[21], v[20], v[22]
    d = os.environ.get("LPX_PIVOT_DEFER", "default")
    print(f"d = {d}: {T.shape[0]} x {T.shape[1]}, pivots={st['pivots']} launches={st['launches']} row launches stamped={calls} "
          f"(mean pending pivots {npend / max(calls, 1):.2f})  loop {1e3 * st['loop_ms'] / max(st['pivots'], 1):.2f} us/pivot (stamped build)")
    if not calls:
        print("  no stamps: is LPX_LIB_PATH the -DLPX_STAMPS library?")
        return
    w = list(hs)[21:27]                                  # the column launch's stamps (w[4]: its launches; 0 in the one-launch form)
    tot = sum(v[:9])
    clk = tot / (rt / 100e6) / 1e9 if rt else 0.0        # s_memrealtime counts at 100 MHz
    print(f"  in-kernel clock ~{clk:.2f} GHz; stamped {tot / calls:.0f} cycles = {rt / calls / 100:.2f} us per launch, wave 0 of workgroup 0")
    for nm, x in zip(NAMES, v[:9]):
        print(f"  {nm:30s} {x / calls:9.0f} cycles {x / calls / clk / 1e3 if clk else 0:7.2f} us {100 * x / tot:5.1f}%")
    if w[4]:
        print(f"  steps that took the tie fallback (exact scan over the ratios): {v[9]} of {calls}")
    elif v[9]:
        print(f"  gather trips per launch {v[9] / calls:.2f}: first {v[10] / calls:.0f}, second {v[11] / calls:.0f}, later {v[12] / calls:.0f} cycles")
    ccalls, crt, cpend = w[4], w[3], w[5]
    if not ccalls:
        print("  column launch: no stamps (the one-launch form ran)")
        return
    ctot = sum(w[:3])
    cclk = ctot / (crt / 100e6) / 1e9 if crt else 0.0
    print(f"  column launch (lpx_pivot_ratio): stamped launches={ccalls} (mean pending pivots {cpend / ccalls:.2f}); in-kernel clock ~{cclk:.2f} GHz; "
          f"stamped {ctot / ccalls:.0f} cycles = {crt / ccalls / 100:.2f} us per launch, wave 0 of workgroup 0")
    for nm, x in zip(COL_NAMES, w[:3]):
        print(f"  {nm:40s} {x / ccalls:9.0f} cycles {x / ccalls / cclk / 1e3 if cclk else 0:7.2f} us {100 * x / ctot:5.1f}%")


def plain_run(pivots, m=4096, n=8192, reps=1, prof=0):
    """The LP on the streaming loop (resident kernels off): a warm-up run, then the best of `reps` runs of at most `pivots`
    pivots; prof: also a profile=1 run of that many pivots for the sweep's own duration by HIP events."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import linear_programming_solver_lpr381_amd as L
    from linear_programming_solver_lpr381_amd import synth

    T, basis = synth.primal_tableau_from(*synth.dense_lp(m, n, seed=synth.SEED))
    dt = L.DeviceTableau.from_host(T, basis)
    dt.snapshot()
    opts = L.default_opts(False, use_graph=1, max_iter=pivots, resident=-1)
    dt.primal_run(opts)
    best = None
    for _ in range(reps):
        dt.restore()
        status, st = dt.primal_run(opts)
        if best is None or st["loop_ms"] < best["loop_ms"]:
            best = st
    line = (f"d = {os.environ.get('LPX_PIVOT_DEFER', 'default')}: {T.shape[0]} x {T.shape[1]} status={status} pivots={best['pivots']} "
            f"launches={best['launches']} loop {1e3 * best['loop_ms'] / max(best['pivots'], 1):.2f} us/pivot = "
            f"{best['pivots'] / best['loop_ms']:.1f} k pivots/s (best of {reps})")
    if prof:
        dt.restore()
        status, pst = dt.primal_run(L.default_opts(False, profile=1, max_iter=prof, resident=-1))
        if pst["update_launches"]:
            line += f"; sweep {1e3 * pst['update_ms_sum'] / pst['update_launches']:.1f} us over {pst['update_launches']} sweeps (HIP events)"
    print(line)


def main():
    a = sys.argv[1:]
    if a and a[0] == "--run":
        return plain_run(*map(int, a[1:6]))
    if a and a[0] == "--child":
        return child(int(a[1]), int(a[2]), int(a[3]))
    m, n = (int(a[0]), int(a[1])) if len(a) > 1 else (4096, 8192)
    pivots = int(a[2]) if len(a) > 2 else 600
    depths = a[3].split(",") if len(a) > 3 else ["12", "2"]
    for d in depths:
        env = dict(os.environ, LPX_PIVOT_DEFER=d)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(m), str(n), str(pivots)], env=env)
        if r.returncode:
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
