"""The revised path (csrc/lpx_revised.hip, DeviceRevised) at every register width, its tail column, the pricing wrap, the
five-launch path, ties and segmented runs, against oracle/revised_ref.py: the basis-only longdouble reference whose
decisions tests/test_revised_ref.py pins to oracle.revised_solve.  oracle.revised_solve re-inverts the basis every
iteration and cannot reach these sizes; the reference can, because after k pivots from the slack basis every solve is a
k x k system.

Bar, everywhere: status, trace, Bidx and Nidx exactly; x_B, z and iteration_view's rc and d within 1e-9 relative to
max(1, |ref|); binv() within 1e-9 * max |B^-1_ref| where it is read.  Random instances first check that every decision the
reference made has a margin above 1e-7 relative (above 1e-10 for the eps thresholds, where an exact 0 sits 1e-9 away), so no
test passes or fails on a coin-flip of rounding; the crafted tie instances are exact by construction instead and assert, from
the reference's records, that the event they were built for still happens.
"""
import hashlib
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _revised_cases as RC                     # noqa: E402
from oracle import revised_ref as R             # noqa: E402

pytestmark = pytest.mark.gpu
REL = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 32

# register width PER = 1, 2, 4, 8 covers m <= 1024, 2048, 4096, 8192 (cover = 8 * PER * 128): every band at cover - 1, cover
# and cover + 1; each band has an odd n, an n < m and an n > 4096.  m = 64 rows: the pricing wrap (n > 2 * RVF_GRID = 4096).
SHAPES = [(1, 7), (2, 5), (129, 4097), (1023, 301), (1024, 2048),
          (1025, 513), (2047, 4099), (2048, 3000),
          (2049, 1001), (4095, 4097), (4096, 6000),
          (4097, 999), (8191, 4097), (8192, 4101),
          (64, 4095), (64, 4096), (64, 4097), (64, 8193)]
UNFUSED = [(8193, 301), (9000, 400), (8193, 4097)]      # m > RVF_MAXLD = 8192: the five-launch path by itself
FORCED_UNFUSED = [(1024, 2048), (4097, 999), (8192, 4101)]


def _self_check(rr, exact_ties=False):
    assert rr.min_margin(skip_exact_ties=exact_ties) > 1e-7, "instance has a near-tie decision: pin another seed"
    if not exact_ties:
        assert rr.min_threshold_margin() > 1e-10, "instance has a value at the eps threshold: pin another seed"


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max(initial=0.0) <= REL, (what, float(err.max()), int(np.argmax(err)))


def _ref_d(rr):
    """d as the kernels leave it: that of the last iteration that computed one (the last pivot, or the unbounded column)."""
    for s in reversed(rr.steps):
        if s.d is not None:
            return s.d
    return None


def _read(rv):
    """result(), lpx_revised_iteration_view (rc[n + m], d[m]) and trace() of a handle."""
    from linear_programming_solver_lpr381_amd._lib import check, dp, lib
    Bidx, Nidx, xB, z = rv.result()
    rc = np.zeros(rv.n + rv.m)
    d = np.zeros(rv.m)
    check(lib().lpx_revised_iteration_view(rv._h, rc.ctypes.data_as(dp), d.ctypes.data_as(dp)))
    return {"Bidx": Bidx, "Nidx": Nidx, "xB": xB, "z": z, "rc": rc, "d": d, "trace": rv.trace()}


def _compare(out, rr, status, tr0=0):
    """`out` (what the handle reports after a run that ended with `status`) against the reference; the trace of that run
    is the reference's trace from pivot tr0 on."""
    assert status == rr.status
    assert out["trace"].tolist() == rr.trace[tr0:]
    assert out["Bidx"].tolist() == rr.Bidx
    assert out["Nidx"].tolist() == rr.Nidx
    _close(out["xB"], rr.xB, "xB")
    _close([out["z"]], [rr.z], "z")
    rc_ref = rr.reduced_costs()
    assert np.array_equal(np.isinf(out["rc"]), np.isinf(rc_ref)), "rc: basic columns"
    fin = np.isfinite(rc_ref)
    _close(out["rc"][fin], rc_ref[fin], "rc")
    d_ref = _ref_d(rr)
    if d_ref is not None:
        _close(out["d"], d_ref, "d")


def _check_binv(Binv, rr, blk=1024):
    scale, err = 0.0, 0.0
    for r0 in range(0, rr.m, blk):
        ref = rr.binv_rows(r0, min(rr.m, r0 + blk))
        scale = max(scale, np.abs(ref).max())
        err = max(err, np.abs(Binv[r0:r0 + blk] - ref).max())
    assert err <= REL * scale, ("binv", err, scale)


def _run_once(gpu, A, c, b, cap, binv=False):
    with gpu.DeviceRevised(A, c, b) as rv:
        status, st = rv.run(max_iter=cap)
        out = _read(rv)
        assert st["pivots"] == len(out["trace"])
        if binv:
            out["binv"] = rv.binv()
    return status, out


# ---- a. shape matrix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", SHAPES, ids=[f"{m}x{n}" for m, n in SHAPES])
def test_shape_matrix(gpu, m, n):
    A, c, b = RC.dense(m, n, 1)
    rr = R.RevisedRef(A, c, b)
    rr.run(CAP)
    _self_check(rr)
    status, out = _run_once(gpu, A, c, b, CAP, binv=m <= 4097)
    _compare(out, rr, status)
    if "binv" in out:
        _check_binv(out["binv"], rr)


# ---- b. five-launch path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", UNFUSED, ids=[f"{m}x{n}" for m, n in UNFUSED])
def test_five_launch_path_above_8192_rows(gpu, m, n):
    A, c, b = RC.dense(m, n, 1)
    rr = R.RevisedRef(A, c, b)
    rr.run(CAP)
    _self_check(rr)
    status, out = _run_once(gpu, A, c, b, CAP)
    _compare(out, rr, status)


def test_five_launch_path_forced_at_fused_sizes(tmp_path):
    """LPX_REVISED_FUSED=0 (read once per process, hence the child): the same bar at sizes the fused iteration also runs."""
    code = textwrap.dedent('''
        import sys, numpy as np
        sys.path.insert(0, sys.argv[2])
        import linear_programming_solver_lpr381_amd as L
        import _revised_cases as RC
        from test_gpu_revised_shapes import FORCED_UNFUSED, CAP, _read
        L._lib.check(L._lib.lib().lpx_init(0))
        res = {}
        for m, n in FORCED_UNFUSED:
            A, c, b = RC.dense(m, n, 1)
            with L.DeviceRevised(A, c, b) as rv:
                status, st = rv.run(max_iter=CAP)
                out = _read(rv)
            for k, v in out.items():
                res[f"{m}x{n}_{k}"] = np.asarray(v)
            res[f"{m}x{n}_status"] = np.asarray(status)
        np.savez(sys.argv[1], **res)
    ''')
    path = str(tmp_path / "unfused.npz")
    env = dict(os.environ, LPX_REVISED_FUSED="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code, path, os.path.dirname(os.path.abspath(__file__))], env=env,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    res = np.load(path)
    for m, n in FORCED_UNFUSED:
        A, c, b = RC.dense(m, n, 1)
        rr = R.RevisedRef(A, c, b)
        rr.run(CAP)
        _self_check(rr)
        out = {k: res[f"{m}x{n}_{k}"] for k in ("Bidx", "Nidx", "xB", "z", "rc", "d", "trace")}
        out["z"] = float(out["z"])
        _compare(out, rr, int(res[f"{m}x{n}_status"]))


# ---- c. ties -------------------------------------------------------------------------------------------------------------
def test_ratio_chains_cover_every_segment_boundary():
    """The chains of CHAINS put near-tied rows on both sides of 1023/1024, 2047/2048 and 4095/4096, and into a last partial
    segment (m = 4500 is 4 full segments and one of 404 rows)."""
    spans = []
    for name in RC.CHAINS:
        rr = R.RevisedRef(*RC.chain(name))
        rr.run(1)
        rows = [rr.trace[0][0]] + rr.steps[0].ratio_band
        if len(rows) > 1:
            spans.append((min(rows), max(rows)))
    for B in RC.BOUNDARIES + (4096 + 1,):
        assert any(lo < B <= hi for lo, hi in spans), B
    assert any(lo >= 4096 for lo, hi in spans)


@pytest.mark.parametrize("name", sorted(RC.CHAINS))
def test_ratio_chain(gpu, name):
    A, c, b = RC.chain(name)
    rr = R.RevisedRef(A, c, b)
    rr.run(1)
    assert rr.steps[0].q == 0
    status, out = _run_once(gpu, A, c, b, 1, binv=True)
    _compare(out, rr, status)
    _check_binv(out["binv"], rr)


TIES = {
    # twins j, j + 30 in different workgroups of rv_price (column j is priced by workgroup j // 2 when n <= 4096)
    "tie_small": RC.tie_core,
    # twins j, j + 4096: the same workgroup, one pass of the pricing wrap apart (n = 8193: 2048 workgroups, odd n)
    "tie_wrap": lambda: RC.embedded(64, 8193, RC.tie_core(), RC.spread(40, 64), list(range(30)) + list(range(4096, 4126))),
    # twins spread over n = 5001 (both passes of the wrap)
    "tie_far": lambda: RC.embedded(300, 5001, RC.tie_core(), RC.spread(40, 300),
                                   list(RC.spread(30, 2400)) + list(RC.spread(30, 5001, lo=2500))),
}


@pytest.mark.parametrize("name", sorted(TIES))
def test_reduced_cost_ties_follow_list_order(gpu, name):
    A, c, b = TIES[name]()
    rr = R.RevisedRef(A, c, b)
    rr.run(10000)
    _self_check(rr, exact_ties=True)
    ev = rr.key_order_ties()
    assert any(t["winner_larger"] for t in ev), "no tie won by the larger column index (smaller key): instance lost its event"
    status, out = _run_once(gpu, A, c, b, 10000)
    _compare(out, rr, status)


def test_slack_reentry_from_a_later_workgroup(gpu):
    """m = 1100: slacks are priced by the first ceil(m / 512) = 3 workgroups of rv_price; slacks >= 512 re-enter."""
    A, c, b = RC.embedded(1100, 200, RC.reentry_core(), RC.spread(10, 1100, lo=505), RC.spread(12, 200))
    rr = R.RevisedRef(A, c, b)
    rr.run(10000)
    _self_check(rr)
    assert rr.status == R.OPTIMAL
    assert any(e["slack"] >= 512 for e in rr.slack_reentries()), rr.slack_reentries()
    status, out = _run_once(gpu, A, c, b, 10000, binv=True)
    _compare(out, rr, status)
    _check_binv(out["binv"], rr)


# ---- d. segments and accessors --------------------------------------------------------------------------------------------
SEGMENTS = {
    # m = 1025 (PER 2), ends optimal; B^-1 read after every segment
    "1025_optimal": (lambda: RC.embedded(1025, 300, RC.optimal_core(), RC.spread(30, 1025), RC.spread(40, 300)), 10000, True),
    # m = 4097 (PER 8, first row past PER 4), ends unbounded on the crafted column after 5 pivots
    "4097_unbounded": (lambda: RC.unbounded_embedded(4097, 500), 10000, True),
    # m = 8192 (PER 8, x_B in the tail columns), ends on the iteration limit; B^-1 read at the end only
    "8192_limit": (lambda: RC.dense(8192, 4101, 1), CAP, False),
}
CUTS = (1, 2, 3, 7, 15)


def _digest(*arrs):
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _read_all(rv, binv_first, with_binv):
    """Every accessor, twice; the two rounds must give the same bits (the pending update is flushed once)."""
    rounds = []
    for rnd in range(2):
        first = binv_first if rnd == 0 else not binv_first
        got = {}
        if with_binv and first:
            got["binv"] = _digest(rv.binv())
        out = _read(rv)
        got["state"] = _digest(out["Bidx"], out["Nidx"], out["xB"], np.float64(out["z"]), out["rc"], out["d"], out["trace"])
        got["residual"] = rv.residual()
        if with_binv and not first:
            got["binv"] = _digest(rv.binv())
        rounds.append(got)
    assert rounds[0] == rounds[1], "a second read changed the state: an update was applied twice"
    return out


@pytest.mark.parametrize("name", sorted(SEGMENTS))
def test_segments_and_accessors(gpu, name):
    make, end_cap, binv_each = SEGMENTS[name]
    A, c, b = make()
    m = len(b)
    rr = R.RevisedRef(A, c, b)
    rr.run(end_cap)
    _self_check(rr)
    final = rr.status
    assert final == {"1025_optimal": R.OPTIMAL, "4097_unbounded": R.UNBOUNDED, "8192_limit": R.ITER_LIMIT}[name]
    rr = R.RevisedRef(A, c, b)
    bnorm = 1.0 + np.abs(b).max()
    joined = []
    with gpu.DeviceRevised(A, c, b) as rv:
        done = 0
        for k, cut in enumerate(CUTS + (end_cap,)):
            status, st = rv.run(max_iter=cut - done)
            rr.run(cut)
            out = _read_all(rv, binv_first=k % 2 == 0, with_binv=binv_each)
            _compare(out, rr, status, tr0=done)
            assert st["pivots"] == len(out["trace"])
            rho, ab = rv.residual()
            full = np.zeros(A.shape[1] + m)
            full[out["Bidx"]] = out["xB"]
            ab_host = np.abs(A @ full[:A.shape[1]] + full[A.shape[1]:] - b).max()
            assert rho <= 1e-10 and abs(ab - ab_host) <= 1e-12 * bnorm, (rho, ab, ab_host)
            if binv_each:
                _check_binv(rv.binv(), rr)
            joined += out["trace"].tolist()
            done = len(rr.trace)
            if status != R.ITER_LIMIT:
                break
        assert status == final and joined == rr.trace
        if not binv_each:
            B1 = rv.binv()
            _check_binv(B1, rr)
            d1 = _digest(B1)
            del B1
            assert _digest(rv.binv()) == d1
            _read_all(rv, binv_first=False, with_binv=False)
    with gpu.DeviceRevised(A, c, b) as rv:           # one uninterrupted run
        status, st = rv.run(max_iter=end_cap)
        assert status == final and rv.trace().tolist() == joined
