"""Probe: the ranging pass at the headline shape (4097 x 12289, synth.dense_lp(4096, 8192) after 200 primal pivots).

Times, after 10 warm-up calls each, `reps` calls (default 300) of DeviceTableau.ranging() (rg_pass + rg_combine + the D2H
copy of the outputs), of lpx_tableau_download of the same tableau (fewer repeats: 403 MB each) and of ranging_pairs() at
K = 64.  Every call waits for its own results before it returns, so the timed calls are NOT back to back: each figure is
host wall time per call (launch, kernels, copy-out, synchronisation).  The kernels' own durations come from running this
probe under `rocprofv3 --kernel-trace --stats`.  The 403 MB tableau is only partly displaced from the
256 MiB Infinity Cache between calls, so repeated passes may read part of it on die.  Prints one JSON line."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import linear_programming_solver_lpr381_amd as L
from linear_programming_solver_lpr381_amd import synth


def timed(f, warm, reps):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(1e6 * (time.perf_counter() - t0))
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts), "reps": reps}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    L._lib.check(L._lib.lib().lpx_init(0))
    c, A, b = synth.dense_lp(4096, 8192)
    T0, basis0 = synth.primal_tableau_from(c, A, b)
    del A
    with L.DeviceTableau.from_host(T0, basis0) as dt:
        del T0
        dt.primal_run(max_iter=200)
        R, C = dt.R, dt.C
        Th = np.empty((R, C)); bh = np.empty(R - 1, dtype=np.int32)
        dl = lambda: L._lib.check(L._lib.lib().lpx_tableau_download(dt._h, Th.ctypes.data_as(L._lib.dp), bh.ctypes.data_as(L._lib.ip)))
        a = np.arange(8192, 8192 + 64, dtype=np.int32)
        out = {"shape": [R, C], "tableau_bytes": 8 * R * C,
               "ranging": timed(lambda: dt.ranging(), 10, reps),
               "download": timed(dl, 3, max(reps // 15, 5)),
               "pairs_k64": timed(lambda: dt.ranging_pairs(a, a + 1), 10, reps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
