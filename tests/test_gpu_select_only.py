"""The select-only launch of the deferred-pivot primal loop (lpx_pivot_select: the column in passes, ratios staged in LDS)
pinned to the CPU oracle at the shapes where that kernel can go wrong.

A run at LPX_PIVOT_DEFER = d makes d - 1 select-only launches per sweep, with n = 1 .. d - 1 pivots pending.  The kernel covers
SELP_PASS_ROWS rows of the entering column per pass, keeps the ratios of up to SELP_LDS_ROWS rows in LDS (longer tableaux take
lpx_pivot_select_ws, the form that stages them in global memory), scans them in segments of 1024, fetches the pending pivots'
factors SELP_SB at a time and hands one partial argmin per workgroup to the last of select_mb_blocks(C) workgroups.  The cases
sit on those edges; the constants are read from the source so that they follow the kernel.  Every run is compared with
oracle.primal_tableau on the same input and cap: status, pivot count, trace, basis and the SHA-256 of the whole float64 tableau.
No tolerances.  tests/test_gpu_deferred_matrix.py remains the matrix over every depth, flush length and run shape.

The host runs this kernel on handles of more than SELP_MIN_MB megabytes and at most SELP_LDS_ROWS rows (smaller handles keep the
form they had, which the matrix test covers).  So an LP that is smaller than that goes into a handle whose capacity is above it,
through lpx_tableau_set_shape: wider (the LP's rows, more columns) or, where the case is about the width, taller.  One and two
select workgroups (C <= 512) cannot reach the kernel: 10 240 rows of 512 columns are 42 MB.

LPX_PIVOT_DEFER and LPX_GRAPH are read once per process, hence one child process per setting, with the resident kernels off.

The "tall" LPs have m = R - 1 constraints and 40 structural columns (C = R + 40): 19 MB at R = SELP_PASS_ROWS (so it goes into
a wider handle), 77 MB at two passes and a row, 840 MB at the LDS cap -- the smallest tableaux with that many rows that are still
LPs with a slack basis."""
import functools
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from linear_programming_solver_lpr381_amd import synth
from test_gpu_deferred_matrix import FULL, _h, _run, _same
from test_gpu_deferred_matrix import _lp as _matrix_lp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
KERNELS_SRC = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "csrc", "lpx_kernels.hip")
BLOCK_HDR = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "csrc", "lpx_block.h")


def _constants():
    """The select-only kernel's launch constants as the source has them."""
    with open(KERNELS_SRC) as f:
        text = f.read()
    with open(BLOCK_HDR) as f:
        text += f.read()
    env = {}
    for name in ("SELP_NT", "SELP_U", "SELP_PASS_ROWS", "SELP_SB", "SELP_LDS_ROWS", "SELP_MIN_MB", "FP_DMAX", "MB_NT", "WH_PER"):
        m = re.search(r"static\s+constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, f"{name} not found as an integer literal"
        env[name] = int(m.group(1))
    assert env["SELP_PASS_ROWS"] == env["SELP_NT"] * env["SELP_U"]
    assert "b > 32" in text and "(C + MB_NT - 1) / MB_NT" in text      # select_mb_blocks: ceil(C / MB_NT), at most 32
    return env


K = _constants()
P, CAP, SB, SEG = K["SELP_PASS_ROWS"], K["SELP_LDS_ROWS"], K["SELP_SB"], 64 * K["WH_PER"]
MAXB_C = 31 * K["MB_NT"] + 1                 # the first C with 32 select workgroups
MIN_BYTES = K["SELP_MIN_MB"] << 20


@functools.lru_cache(maxsize=2)
def _lp_cached(name):
    kind, a, b, seed = name.split(":")
    assert kind == "lp"
    return synth.primal_tableau_from(*synth.dense_lp(int(a), int(b), seed=int(seed)))


def _lp(name):
    """"lp:m:n:seed": synth.dense_lp(m, n, seed) as a primal tableau of (m + 1) x (m + n + 1); else the matrix test's LPs."""
    if not name.startswith("lp:"):
        return _matrix_lp(name)
    T, basis = _lp_cached(name)
    return T.copy(), basis.copy()


def _shape_of(name):
    if name.startswith("lp:"):
        _, m, n, _ = name.split(":")
        return int(m) + 1, int(m) + int(n) + 1
    return _matrix_lp(name)[0].shape


def _open(name, taller=False):
    """Plan steps that put the LP on a handle the select-only kernel serves: its own when that is above SELP_MIN_MB, else one
    with more columns (or, taller: more rows, the width kept) until it is."""
    R, C = _shape_of(name)
    ld = (C + 15) // 16 * 16
    if 8 * R * ld > MIN_BYTES:
        return [["open", name]]
    if taller:
        Rc = MIN_BYTES // (8 * ld) + 2
        assert Rc <= CAP
        return [["alloc", Rc, C], ["shape", name]]
    return [["alloc", R, MIN_BYTES // (8 * R) + 32], ["shape", name]]


def _tall(R, seed=3):
    return f"lp:{R - 1}:40:{seed}"


def _wide(C, m, seed=3):
    return f"lp:{m}:{C - m - 1}:{seed}"


_CHILD = """
    import hashlib, json, sys, numpy as np
    sys.path.insert(0, %r)
    import linear_programming_solver_lpr381_amd as L
    from test_gpu_select_only import _lp
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
                        h(tr, np.int32), h(bg, np.int32), h(Tg, np.float64), None])
    dt.close()
    print(json.dumps(out))
""" % TESTS


def _child(plan, env, timeout=300):
    e = dict(os.environ, PYTHONPATH=ROOT, LPX_RESIDENT="0", **env)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(_CHILD), json.dumps(plan)], env=e, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def ref(oracle):
    """ref(lp, cap) -> [status, pivots, trace, basis, tableau] hashes as a child reports them; computed once per (lp, cap).
    The long tableaux take the oracle's OpenMP loop (the same bits as its scalar one)."""
    @functools.lru_cache(maxsize=None)
    def get(name, cap):
        T, basis = _lp(name)
        st, tr = oracle.primal_tableau(T, basis, max_iter=cap, threads=8 if T.size > (1 << 24) else None)
        return [int(st), len(tr), _h(tr, np.int32), _h(basis, np.int32), _h(T, np.float64)]
    return get


def _check(got, want, what):
    assert len(got) == len(want)
    bad = [(i, g[:2], w[:2]) for i, (g, w) in enumerate(zip(got, want)) if not _same(g, w)]
    assert not bad, (what, bad)


def test_constants_and_cases():
    """The cases below follow the kernel: the cap holds two passes and a row (so that R = 2 P + 1 runs the LDS form, in three
    passes like the headline LP's 4097 rows), d = 12 and d = 16 cross every factor batch, and cap 25 at d = 12 reaches
    n = 1 .. 11 and two sweeps."""
    assert CAP >= 2 * P + 1 and 2 * P < 4097 <= 3 * P
    assert SB < 11 and 2 * SB >= K["FP_DMAX"] - 1               # n = 1 .. 11 crosses SB; two batches hold every n
    assert {L % 12 for L in range(1, 25)} == set(range(12))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. pass edges: the column in one pass less a row, exactly one pass, one pass and a row, two passes and a row (three passes)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [P - 1, P, P + 1, 2 * P + 1], ids=["P-1", "P", "P+1", "2P+1"])
def test_pass_edges_vs_oracle(ref, R):
    """d = 12, 25 pivots: launches 1 .. 11 and 13 .. 23 are select-only with n = 1 .. 11 pending, 12 and 24 sweep."""
    lp = _tall(R)
    want = ref(lp, 25)
    assert want[:2] == [3, 25]                                  # the oracle makes all 25 pivots
    _check(_child(_open(lp) + [_run(25)], {"LPX_PIVOT_DEFER": "12"}), [want], R)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the LDS row cap: the last shape of the LDS form, the first of the workspace form
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [CAP, CAP + 1], ids=["cap", "cap+1"])
def test_lds_cap_edge_vs_oracle(ref, R):
    """d = 2, 6 pivots: every other launch selects only.  R = cap + 1 takes lpx_pivot_select_ws.  The host compares the
    handle's CAPACITY with the cap, and here the capacity is the LP's own R.  Both forms give the same bits, so equal results
    do not say which one ran; what this pair does catch is a comparison that lets R = cap + 1 into the LDS form, whose launch
    then asks for more dynamic LDS than the kernel's attribute allows and fails.  test_capacity_at_and_above_the_lds_cap has
    the same edge with a small LP in a tall handle."""
    lp = _tall(R)
    want = ref(lp, 6)
    assert want[:2] == [3, 6]
    _check(_child([["open", lp], _run(6)], {"LPX_PIVOT_DEFER": "2"}), [want], R)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the scan reading its ratios from LDS: one segment (the wave scan), two segments, ties handed to the exact replay
# ---------------------------------------------------------------------------------------------------------------------------
def test_scan_from_lds_segments_and_ties(ref):
    """m = 1024 (one segment) and m = 1025 (two) at 25 pivots; "ties-low" and "ties-high" (1801 rows: clean segments, the tie
    hand-over to the exact replay, winners in the second segment) to their end.  d = 12."""
    assert SEG == 1024
    plan, want = [], []
    for lp, cap in ((f"lp:{SEG}:40:3", 25), (f"lp:{SEG + 1}:40:3", 25), ("ties-low", FULL), ("ties-high", FULL)):
        plan += _open(lp) + [_run(cap)]
        want.append(ref(lp, cap))
    assert want[0][:2] == [3, 25] and want[1][:2] == [3, 25] and want[2][1] >= 25 and want[3][1] >= 25
    _check(_child(plan, {"LPX_PIVOT_DEFER": "12"}), want, "scan")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. workgroup counts: one workgroup (the hand-off with itself), two, and the first width with all 32
# ---------------------------------------------------------------------------------------------------------------------------
def test_workgroup_count_edges_vs_oracle(ref):
    """C = 7937 (the first C with 32 workgroups: the select-only launch uses select_mb_blocks(C) workgroups like the sweep
    launches, so that count has no other neighbours), 7936 (31) and 3000 (12, the last one short); C = 32 SELP_NT + 100: more
    columns per workgroup than lanes, so the row loop's second trip loads its operands itself.  Handles made taller, the width
    kept.  d = 12, 25 pivots."""
    plan, want = [], []
    for lp in (_wide(3000, 100), _wide(MAXB_C - 1, 60), _wide(MAXB_C, 60), _wide(32 * K["SELP_NT"] + 100, 60)):
        plan += _open(lp, taller=True) + [_run(25)]
        want.append(ref(lp, 25))
        assert want[-1][:2] == [3, 25], lp
    _check(_child(plan, {"LPX_PIVOT_DEFER": "12"}), want, "workgroups")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. chain grouping: pending counts on both sides of every batch of factor loads
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 5, 16])
def test_chain_grouping_depths_vs_oracle(ref, d):
    """"dense" (302 x 589) to its end and to 2d + 3 pivots: n = 1 .. d - 1, at d = 16 through both batches of SELP_SB."""
    plan, want = _open("dense"), []
    for cap in (2 * d + 3, FULL):
        plan += [["restore"], _run(cap)]
        want.append(ref("dense", cap))
    _check(_child(plan, {"LPX_PIVOT_DEFER": str(d)}), want, d)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. a handle larger than its LP: the factor ring's stride is the capacity, the live shape comes from the device record
# ---------------------------------------------------------------------------------------------------------------------------
def test_capacity_above_shape_vs_oracle(ref):
    """A 3000 x 3000 handle (72 MB) takes "dense" (302 x 589) through lpx_tableau_set_shape; d = 12, to the end."""
    want = ref("dense", FULL)
    _check(_child([["alloc", 3000, 3000], ["shape", "dense"], _run(FULL)], {"LPX_PIVOT_DEFER": "12"}), [want], "capacity")


def test_capacity_at_and_above_the_lds_cap(ref):
    """Handles of cap and cap + 1 rows (900 columns, 74 MB) take "dense" (302 x 589) through lpx_tableau_set_shape: the form is
    chosen by the capacity, so the first runs the LDS form with all 8 * cap bytes of dynamic LDS and a factor-ring stride of cap,
    the second the workspace form although the live rows would fit.  d = 12, to the end."""
    want = ref("dense", FULL)
    plan = [["alloc", CAP, 900], ["shape", "dense"], _run(FULL), ["alloc", CAP + 1, 900], ["shape", "dense"], _run(FULL)]
    _check(_child(plan, {"LPX_PIVOT_DEFER": "12"}), [want, want], "capacity at the cap")


# ---------------------------------------------------------------------------------------------------------------------------
# 7. a terminal status found by a select-only launch, with pivots pending
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "eager"])
def test_termination_in_a_select_only_launch(ref, graph):
    """d = 12: "late-unbounded" ends unbounded after 500 pivots (8 pending); the iteration cap at K = 13, 23, 37 and 47
    (K mod 12 = 1 and 11) is met by a select-only launch with 1 and 11 pivots pending."""
    plan, want = _open("late-unbounded") + [_run(FULL)] + _open("dense"), [ref("late-unbounded", FULL)]
    assert want[0][0] == 1 and want[0][1] % 12 not in (0,)
    for cap in (13, 23, 37, 47):
        assert cap % 12 in (1, 11)
        plan += [["restore"], _run(cap)]
        want.append(ref("dense", cap))
    env = {"LPX_PIVOT_DEFER": "12"}
    if graph == "0":
        env["LPX_GRAPH"] = "0"
    _check(_child(plan, env), want, graph)
