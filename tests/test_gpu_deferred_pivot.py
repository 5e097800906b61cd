"""Deferred pivots on the fused primal loop (LPX_PIVOT_DEFER=d, run_fused in csrc/lpx_tableau.cpp): every d-th launch is a sweep
that applies the d pivots selected before it, the others select only, reading the stored tableau with the pending pivots
applied on the fly.  Each element goes through the same multiplies and subtractions in the same order as with one sweep per
pivot, so the tableau is bit-identical to the oracle's for every d -- including runs that end with fewer than d pivots pending
(the cap not a multiple of d, optimal, unbounded), which the host flushes before anything reads the tableau.

The knob is read once per process, hence one child process per setting.  These are spot checks on the bench LP and on small
LPs; tests/test_gpu_deferred_matrix.py pins every depth 1 .. 16 in both sweep forms, every flush length and ring half, chained
runs without restore(), graph replay against eager launches, handle reuse through set_shape, long degenerate columns and
profile runs to the oracle."""
import hashlib
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from linear_programming_solver_lpr381_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")


def _h(a, dt):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dt).view(np.uint8)).hexdigest()


def _child(code, env, *args, timeout=900):
    e = dict(os.environ, PYTHONPATH=ROOT, **env)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)] + [str(a) for a in args], env=e, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


_HEADLINE = """
    import hashlib, json, sys, numpy as np
    import linear_programming_solver_lpr381_amd as L
    from linear_programming_solver_lpr381_amd import synth
    h = lambda a, dt: hashlib.sha256(np.ascontiguousarray(a, dtype=dt).view(np.uint8)).hexdigest()
    c, A, b = synth.dense_lp(4096, 8192)
    T, basis = synth.primal_tableau_from(c, A, b)
    del A
    out = []
    with L.DeviceTableau.from_host(T, basis) as dt:
        dt.snapshot()
        for cap in json.loads(sys.argv[1]):
            dt.restore()
            status, st = dt.primal_run(max_iter=cap)
            Tg, bg = dt.download()
            out.append([cap, int(status), int(st["pivots"]), int(st["launches"]), h(dt.trace(), np.int32), h(bg, np.int32),
                        h(Tg, np.float64)])
    print(json.dumps(out))
"""

_CAPS = [150, 151, 157]


@pytest.fixture(scope="module")
def headline_ref(oracle):
    c, A, b = synth.dense_lp(4096, 8192)
    T, basis = synth.primal_tableau_from(c, A, b)
    del A
    ref = {}
    for cap in _CAPS:
        Tr, br = T.copy(), basis.copy()
        st, tr = oracle.primal_tableau(Tr, br, max_iter=cap)
        ref[cap] = [int(st), len(tr), _h(tr, np.int32), _h(br, np.int32), _h(Tr, np.float64)]
    return ref


@pytest.mark.parametrize("d", [2, 3, 8, 16])
def test_headline_lp_first_pivots_vs_oracle(headline_ref, d):
    """The bench LP (4097 x 12289, 403 MB) for 150 / 151 / 157 pivots, one handle restored between runs: most caps are not
    multiples of d, so the runs end with partial flushes of several lengths.  Trace, basis and every tableau bit as the oracle's."""
    got = _child(_HEADLINE, {"LPX_PIVOT_DEFER": str(d)}, json.dumps(_CAPS))
    for cap, status, pivots, launches, tr, bs, tb in got:
        assert [status, pivots, tr, bs, tb] == headline_ref[cap], (d, cap)
        assert launches > cap                                          # a launch per pivot (+ the batch ahead)


_SMALL = """
    import hashlib, json, sys, numpy as np
    sys.path.insert(0, %r)
    import linear_programming_solver_lpr381_amd as L
    from test_gpu_configs import _small_lps
    h = lambda a, dt: hashlib.sha256(np.ascontiguousarray(a, dtype=dt).view(np.uint8)).hexdigest()
    out = []
    for name, T, basis in _small_lps():
        caps = json.loads(sys.argv[1])[name]
        with L.DeviceTableau.from_host(T, basis) as dt:
            dt.snapshot()
            for cap in caps:
                dt.restore()
                status, st = dt.primal_run(max_iter=cap, resident=-1)
                assert st["launches"] >= st["pivots"], st
                Tg, bg = dt.download()
                out.append([name, cap, int(status), int(st["pivots"]), h(dt.trace(), np.int32), h(bg, np.int32), h(Tg, np.float64)])
    print(json.dumps(out))
""" % TESTS


@pytest.fixture(scope="module")
def small_ref(oracle):
    sys.path.insert(0, TESTS)
    from test_gpu_configs import _small_lps
    want = []
    for name, T, basis in _small_lps():
        Tr, br = T.copy(), basis.copy()
        _, tr_ref = oracle.primal_tableau(Tr, br, max_iter=10000)
        caps = [10000] + ([len(tr_ref), len(tr_ref) - 1] if len(tr_ref) > 1 else [])
        for cap in caps:
            Tc, bc = T.copy(), basis.copy()
            s_c, t_c = oracle.primal_tableau(Tc, bc, max_iter=cap)
            want.append([name, cap, int(s_c), len(t_c), _h(t_c, np.int32), _h(bc, np.int32), _h(Tc, np.float64)])
    return want


@pytest.mark.parametrize("policy", ["0", "2"], ids=["cached", "streaming-mix"])
@pytest.mark.parametrize("d", [1, 2, 4, 5, 12, 16])
def test_small_lps_to_the_end_vs_oracle(small_ref, d, policy):
    """Small LPs run to their end (optimal, unbounded, the cap at the optimum's pivot count and one before it) on the streaming
    kernels (resident kernels off), both cache-policy forms of the sweep: status, trace, basis and tableau bits as the oracle's."""
    caps = {}
    for w in small_ref:
        caps.setdefault(w[0], []).append(w[1])
    got = _child(_SMALL, {"LPX_RESIDENT": "0", "LPX_UPDATE_POLICY": policy, "LPX_PIVOT_DEFER": str(d)}, json.dumps(caps), timeout=600)
    assert got == small_ref, [(g, w) for g, w in zip(got, small_ref) if g != w]


_BENCH_LENGTH = """
    import hashlib, json, sys, numpy as np
    import linear_programming_solver_lpr381_amd as L
    from linear_programming_solver_lpr381_amd import synth
    h = lambda a, dt: hashlib.sha256(np.ascontiguousarray(a, dtype=dt).view(np.uint8)).hexdigest()
    c, A, b = synth.dense_lp(4096, 8192)
    T, basis = synth.primal_tableau_from(c, A, b)
    del A
    out = []
    with L.DeviceTableau.from_host(T, basis) as dt:
        dt.snapshot()
        for _ in range(2):                       # snapshot -> run -> restore -> run: the same bits twice
            dt.restore()
            status, st = dt.primal_run(max_iter=10000)
            Tg, bg = dt.download()
            out.append([int(status), int(st["pivots"]), int(st["launches"]), h(dt.trace(), np.int32), h(bg, np.int32), h(Tg, np.float64)])
        dt.restore()
        _, sp = dt.primal_run(L.default_opts(False, profile=1, max_iter=400))
        out.append([int(sp["pivots"]), int(sp["launches"]), int(sp["update_launches"])])
    print(json.dumps(out))
"""


def test_bench_length_run_same_bits_as_one_pivot_per_sweep():
    """10 000 pivots of the bench LP at the default depth and at LPX_PIVOT_DEFER=1 (one sweep per pivot): trace, basis and
    tableau SHA-256 identical, twice on one handle.  One launch per pivot, and in a profile run the sweeps -- the launches
    counted as updates -- are about pivots / d of them."""
    runs = {}
    for tag, env in (("default", {}), ("d1", {"LPX_PIVOT_DEFER": "1"}), ("d8", {"LPX_PIVOT_DEFER": "8"})):
        runs[tag] = _child(_BENCH_LENGTH, env)
    for tag, r in runs.items():
        a, b, prof = r
        assert a[0] == 3 and a[1] == 10000, (tag, a)               # the iteration cap
        assert a[1] < a[2] <= 1.1 * a[1] + 4, (tag, a)
        assert a == b, tag
    assert runs["default"][0][3:] == runs["d1"][0][3:] == runs["d8"][0][3:]
    p1, p8 = runs["d1"][2], runs["d8"][2]
    assert p1[0] == p8[0] == 400
    assert p1[2] >= 390                                            # d = 1: every launch a sweep
    assert abs(p8[2] - 400 / 8) <= 3, p8                           # d = 8: one sweep per eight pivots
