"""The deferred-pivot primal loop (run_fused, LPX_PIVOT_DEFER = d) pinned to the CPU oracle at every depth, flush length and run
shape -- the matrix behind tests/test_gpu_deferred_pivot.py's spot checks.

Launch L of a run selects pivot L; when L is a positive multiple of d it is also the sweep that applies the d pivots before it
(lpx_pivot_fused<d> / lpx_pivot_fused_c<d>).  A run with cap K therefore ends with K mod d pivots pending, the oldest in ring slot
(K // d) % 2 * d, and the stored tableau in buffer (K // d) % 2: lpx_pivot_flush applies the pending ones into buffer 0, or the
tableau is copied home from buffer 1 when none are pending.  The caps below reach every (d, npend, slot half) cell for both sweep
forms.  Every run is compared with oracle.primal_tableau on the same input and cap: status, pivot count, trace, basis and the
SHA-256 of the whole float64 tableau.  No tolerances.

LPX_PIVOT_DEFER, LPX_UPDATE_POLICY, LPX_UPDATE_MIXMOD and LPX_GRAPH are read once per process, hence one child process per
setting; the children also run with the resident kernels off, so every LP here takes the streaming loop."""
import functools
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
DMAX = 16                       # FP_DMAX: sweep kernels are built for d = 1 .. 16
FULL = 10000                    # "to the end"


def _h(a, dt):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dt).view(np.uint8)).hexdigest()


@functools.lru_cache(maxsize=None)
def _lp_cached(name):
    if name == "dense":                 # 302 x 589: rows a multiple of neither sweep tile (3, 8), ld padded to 592; 504 pivots
        T, basis = synth.primal_tableau_from(*synth.dense_lp(301, 287, seed=22))
    elif name == "dense2":              # 401 x 701, 652 pivots
        T, basis = synth.primal_tableau_from(*synth.dense_lp(400, 300, seed=5))
    elif name == "late-unbounded":      # "dense" plus a zero column of cost 0.01: it enters, unbounded, after 500 pivots
        c, A, b = synth.dense_lp(301, 287, seed=22)
        T, basis = synth.primal_tableau_from(np.append(c, 0.01), np.hstack([A, np.zeros((301, 1))]), b)
    elif name in ("ties-low", "ties-high"):
        # 0/1-style degeneracy over 1801 rows (two scan segments, 28 MB): every pivot is a zero-ratio pivot with several rows
        # tied (and near-ties inside the 1e-9 band); "ties-low" resolves all its 115 ties in rows < 35, "ties-high" keeps the
        # first 1100 rows out of the ties, so all 57 of its pivot rows lie in the second segment
        m, n = 1800, 120
        g = np.random.default_rng(5 if name == "ties-low" else 6)
        A = g.integers(-1, 3, size=(m, n)).astype(float)
        b = g.integers(0, 3, size=m).astype(float)
        split = 0 if name == "ties-low" else 1100
        b[:split] += 4.0
        b[[7, split + 3, m - 1]] += np.array([3e-10, 6e-10, 9e-10])
        c = g.integers(1, 9, size=n).astype(float)
        T, basis = synth.primal_tableau_from(c, A, b)
    else:
        raise KeyError(name)
    return T, basis


def _lp(name):
    T, basis = _lp_cached(name)
    return T.copy(), basis.copy()


# One child runs a list of steps on one handle and prints one record per "run" step:
#   ["open", lp]                 a handle sized to the LP, its start kept for restore()
#   ["alloc", R, C]              an empty handle of that capacity
#   ["shape", lp]                the LP into the handle through lpx_tableau_set_shape (+ upload, snapshot)
#   ["restore"]                  back to the snapshot
#   ["run", cap, opts, keep]     primal_run(max_iter=cap, resident=-1, **opts); keep: return the trace itself
_CHILD = """
    import hashlib, json, sys, numpy as np
    sys.path.insert(0, %r)
    import linear_programming_solver_lpr381_amd as L
    from test_gpu_deferred_matrix import _lp
    h = lambda a, dt: hashlib.sha256(np.ascontiguousarray(a, dtype=dt).view(np.uint8)).hexdigest()
    out, dt = [], None
    for step in json.loads(sys.argv[1]):
        op = step[0]
        if op == "open":
            if dt is not None: dt.close()
            dt = L.DeviceTableau.from_host(*_lp(step[1]))
            dt.snapshot()
        elif op == "alloc":
            if dt is not None: dt.close()
            dt = L.DeviceTableau(step[1], step[2])
        elif op == "shape":
            T, basis = _lp(step[1])
            L._lib.check(L._lib.lib().lpx_tableau_set_shape(dt._h, T.shape[0], T.shape[1]))
            dt.R, dt.C = T.shape
            dt.upload(T, basis)
            dt.snapshot()
        elif op == "restore":
            dt.restore()
        elif op == "run":
            status, st = dt.primal_run(L.default_opts(False, max_iter=step[1], resident=-1, **step[2]))
            Tg, bg = dt.download()
            tr = dt.trace()
            out.append([int(status), int(st["pivots"]), int(st["launches"]), int(st["update_launches"]),
                        h(tr, np.int32), h(bg, np.int32), h(Tg, np.float64), tr.tolist() if step[3] else None])
    dt.close()
    print(json.dumps(out))
""" % TESTS


def _child(plan, env, timeout):
    e = dict(os.environ, PYTHONPATH=ROOT, LPX_RESIDENT="0", **env)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(_CHILD), json.dumps(plan)], env=e, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def _run(cap, keep=False, **opts):
    return ["run", cap, opts, keep]


@pytest.fixture(scope="module")
def ref(oracle):
    """ref(lp, cap) -> ([status, pivots, trace, basis, tableau] hashes as a child reports them, trace as a list)."""
    @functools.lru_cache(maxsize=None)
    def get(name, cap):
        T, basis = _lp(name)
        st, tr = oracle.primal_tableau(T, basis, max_iter=cap)
        return [int(st), len(tr), _h(tr, np.int32), _h(basis, np.int32), _h(T, np.float64)], tr.tolist()
    return get


def _same(rec, want):
    """A child's record against the oracle's: status, pivots, trace, basis, tableau."""
    return [rec[0], rec[1], rec[4], rec[5], rec[6]] == want


# ---------------------------------------------------------------------------------------------------------------------------
# 1. depth x flush length: caps 1 .. 2d reach npend = cap mod d = 1 .. d-1 with the oldest pending pivot in slot 0 (cap < d) and
# in slot d (d < cap < 2d), the tableau in buffer 1 with nothing pending (cap = d, copied home) and in buffer 0 (cap = 2d); 2d+1
# and 4d+3 come after whole turns of the ring.  Each child also runs "dense" and "late-unbounded" to their end.
# ---------------------------------------------------------------------------------------------------------------------------
def _matrix_caps(d):
    return sorted(set(range(1, 2 * d + 1)) | {max(d - 1, 1), d, d + 1, 2 * d + 1, 4 * d + 3})


def _cells(d, caps):
    """(npend, slot half) of the runs ending on a cap; npend = 0 ends in buffer `half` (1: the copy home)."""
    return {(k % d, (k // d) % 2) for k in caps}


def test_matrix_reaches_every_depth_flush_length_and_slot_half():
    """All 16 depths x 2 sweep forms x every npend in 0 .. d-1, each with the oldest pending pivot in either half of the ring
    (npend = 0: the tableau in either buffer), plus cap 1 and runs shorter than d (no sweep, the flush does everything)."""
    for d in range(1, DMAX + 1):
        caps = _matrix_caps(d)
        assert _cells(d, caps) == {(n, half) for n in range(d) for half in (0, 1)}, d
        assert 1 in caps and d in caps and d + 1 in caps and (d - 1 in caps or d == 1)
        assert max(caps) < 504                                  # every cap stops "dense" before its optimum
    assert len(_MATRIX) == 2 * DMAX


_MATRIX = [(d, pol) for pol in ("0", "2") for d in range(1, DMAX + 1)]


@pytest.mark.parametrize("d,policy", _MATRIX, ids=[f"d{d}-{'cached' if p == '0' else 'streaming-mix'}" for d, p in _MATRIX])
def test_depth_flush_matrix_vs_oracle(ref, d, policy):
    """One handle, restore() between caps: every cap of _matrix_caps(d), then "dense" and "late-unbounded" to their end, in
    the cached sweep form (lpx_pivot_fused_c<d>) or the streaming one (lpx_pivot_fused<d>; LPX_UPDATE_MIXMOD=7 so that both
    store sequences of the mixed form run, and fp_rows' rescale of mixmod: 7 row blocks at d <= 2, 2 at d >= 3)."""
    caps = _matrix_caps(d)
    plan = [["open", "dense"]]
    for cap in caps:
        plan += [["restore"], _run(cap)]
    plan += [["restore"], _run(FULL), ["open", "late-unbounded"], _run(FULL)]
    env = {"LPX_PIVOT_DEFER": str(d), "LPX_UPDATE_POLICY": policy}
    if policy == "2":
        env["LPX_UPDATE_MIXMOD"] = "7"
    got = _child(plan, env, timeout=300)
    want = [ref("dense", cap)[0] for cap in caps] + [ref("dense", FULL)[0], ref("late-unbounded", FULL)[0]]
    assert len(got) == len(want)
    bad = [(cap, g[:2], w[:2]) for cap, g, w in zip(caps + ["dense-end", "unbounded-end"], got, want) if not _same(g, w)]
    assert not bad, (d, policy, bad)
    assert want[-2][0] == 0 and want[-1][0] == 1                # the oracle: optimal, then unbounded after 500 pivots
    for cap, g in zip(caps, got):
        assert g[0] == 3 and g[1] == cap, (d, cap, g[:3])       # the iteration cap, exactly cap pivots
        assert g[2] >= cap                                      # one launch per pivot (+ the batch ahead, the flush)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. chained runs on one handle, no restore(): each run starts from what the last one left -- flushed into buffer 0, or copied
# home from buffer 1
# ---------------------------------------------------------------------------------------------------------------------------
def _slices(d):
    return [1, d - 1, d, 2 * d + 3, 3 * d]


@pytest.mark.parametrize("d", [3, 4, 12])
def test_chained_runs_continue_where_the_last_one_stopped(ref, d):
    """"dense" and "late-unbounded" in slices of 1, d-1, d, 2d+3 and 3d pivots, then to the end, on one handle: the slices end
    with pivots pending (flushed) and with the tableau in buffer 1 (copied home).  After every slice the tableau and basis are
    the oracle's at the cumulative cap with the iteration-cap status; the slices' traces, joined, are the oracle's trace of one
    uninterrupted run and their pivot counts add up to its length; the last slice ends as that run does."""
    sl = _slices(d)
    plan = []
    for lp in ("dense", "late-unbounded"):
        plan += [["open", lp]] + [_run(k, keep=True) for k in sl] + [_run(FULL, keep=True)]
    got = _child(plan, {"LPX_PIVOT_DEFER": str(d)}, timeout=300)
    assert len(got) == 2 * (len(sl) + 1)
    for i, lp in enumerate(("dense", "late-unbounded")):
        runs = got[i * (len(sl) + 1):(i + 1) * (len(sl) + 1)]
        full, full_tr = ref(lp, FULL)
        done, joined = 0, []
        for k, g in zip(sl, runs):
            done += k
            want, _ = ref(lp, done)
            assert g[0] == 3 and g[1] == k, (lp, d, done, g[:2])
            assert [g[5], g[6]] == want[3:], (lp, d, done)            # basis and tableau bits at the cumulative cap
            joined += g[7]
        last = runs[-1]
        joined += last[7]
        assert last[0] == full[0] and done + last[1] == full[1], (lp, d, last[:2], full[:2])
        assert joined == full_tr, (lp, d)
        assert [last[5], last[6]] == full[3:], (lp, d)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. graph replay against eager launches, at batches that need rounding up to a multiple of 2d
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "eager"])
@pytest.mark.parametrize("d", [4, 7, 12])
def test_graph_and_eager_launches_vs_oracle(ref, d, graph):
    """Batches 1, 7, 33 and the default (rounded up to 2d, 2d, a multiple of 2d above 33, and above 64) with the graph
    (default) and eager (LPX_GRAPH=0): caps d+1 (one pivot pending, slot d), 2d (none, buffer 0), 3d+2, and the end.  Then
    caps alternating on one handle -- the graph of a cap is replayed from the handle's slot (same cap twice) or taken back from
    the park (the other cap between) instead of being captured again.  Every run as the oracle's."""
    caps = [d + 1, 2 * d, 3 * d + 2, FULL]
    plan, want = [["open", "dense"]], []
    for batch in (1, 7, 33, 0):
        for cap in caps:
            plan += [["restore"], _run(cap, batch=batch)]
            want.append(ref("dense", cap)[0])
    for cap in (d + 3, d + 3, 2 * d + 5, d + 3, 2 * d + 5, FULL, 2 * d + 5):
        plan += [["restore"], _run(cap)]
        want.append(ref("dense", cap)[0])
    env = {"LPX_PIVOT_DEFER": str(d)}
    if graph == "0":
        env["LPX_GRAPH"] = "0"
    got = _child(plan, env, timeout=300)
    assert len(got) == len(want)
    bad = [(i, g[:2], w[:2]) for i, (g, w) in enumerate(zip(got, want)) if not _same(g, w)]
    assert not bad, (d, graph, bad)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. handle reuse through lpx_tableau_set_shape
# ---------------------------------------------------------------------------------------------------------------------------
def test_set_shape_handle_above_64mb_picks_depth_from_capacity(ref):
    """A 3000 x 3000 handle (72 MB with ld = 3008) takes "dense" (302 x 589), then "dense2" (401 x 701: more live rows than the
    first snapshot was taken with), through lpx_tableau_set_shape, at the default depth.  Both solves are the oracle's, eager
    and in a profile run.

    The depth comes from the handle's capacity, not from the live shape (pivot_defer(ld, Rcap) in run_fused), like the cache
    policy, mixmod and select width of the same loop: every sizing decision of a handle follows its capacity, and the sweep
    streams the live rows at the capacity's ld.  So both LPs run at d = 12, the > 64 MB default, where their own size would
    give d = 4.  DESIGN.md 4.1 measured the depths on full tableaux only (403 MB and 25 MB), nothing on a small live shape
    in a large handle, so this asserts the current choice rather than a measured better one: one sweep per 12 pivots."""
    plan = [["alloc", 3000, 3000]]
    for lp in ("dense", "dense2"):
        plan += [["shape", lp], _run(FULL), ["restore"], _run(FULL, profile=1)]
    got = _child(plan, {}, timeout=300)
    assert len(got) == 4
    for i, lp in enumerate(("dense", "dense2")):
        eager, prof = got[2 * i], got[2 * i + 1]
        want = ref(lp, FULL)[0]
        assert _same(eager, want) and _same(prof, want), (lp, eager[:2], prof[:2], want[:2])
        p = prof[1]
        assert abs(prof[3] - p // 12) <= 1, (lp, p, prof[3])   # d = 12: from the capacity (d = 4 would give ~p / 4)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. degenerate ties over long columns, and the unbounded exit with a full ring behind it
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 4, 12, 16])
def test_ties_over_two_segments_and_late_unbounded(ref, d):
    """Tie-heavy LPs of 1801 rows (the ratio test's ties broken on values rebuilt through the pending pivots, in the first
    and in the second scan segment) to the end and at caps d+1 and 3d+1; "late-unbounded" to its end, which comes after
    500 pivots with 500 mod d pending; every run the oracle's."""
    plan, want = [], []
    for lp in ("ties-low", "ties-high"):
        plan.append(["open", lp])
        for cap in (d + 1, 3 * d + 1, FULL):
            plan += [["restore"], _run(cap)]
            want.append(ref(lp, cap)[0])
    plan += [["open", "late-unbounded"], _run(FULL)]
    want.append(ref("late-unbounded", FULL)[0])
    assert want[2][1] >= 3 * 16 and want[5][1] >= 3 * 16        # both run past three full rings at d = 16
    assert want[-1][0] == 1 and want[-1][1] >= 3 * d
    got = _child(plan, {"LPX_PIVOT_DEFER": str(d)}, timeout=300)
    assert len(got) == len(want)
    bad = [(i, g[:2], w[:2]) for i, (g, w) in enumerate(zip(got, want)) if not _same(g, w)]
    assert not bad, (d, bad)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. profile mode
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 16])
def test_profile_run_same_bits_and_one_sweep_per_d(ref, d):
    """A profile run (event-bracketed eager launches, one batch at a time) of "dense" to the end and to cap 2d+3: the same
    bits as the plain run and the oracle's, and the launches counted as updates are the sweeps, floor(pivots / d) of them."""
    plan, want = [["open", "dense"]], []
    for cap in (FULL, 2 * d + 3):
        plan += [["restore"], _run(cap), ["restore"], _run(cap, profile=1)]
        want += [ref("dense", cap)[0]] * 2
    got = _child(plan, {"LPX_PIVOT_DEFER": str(d)}, timeout=300)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert _same(g, w), (d, g[:2], w[:2])
    for plain, prof in (got[0:2], got[2:4]):
        assert plain[4:7] == prof[4:7]
        assert abs(prof[3] - prof[1] // d) <= 1, (d, prof[1], prof[3])
