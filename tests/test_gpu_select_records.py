"""The select-only pair with the leaving row from scan records and the entering column reduced by its consumer
(lpx_pivot_ratio, lpx_pivot_select in lpx_pivot_fused.hip), pinned to the CPU oracle bit for bit.

Each workgroup of the column launch reduces its SELC_ROWS = 256 rows to one record (least ratio, its first row, or -1 when
that row is not alone in the band of tol above it); the row launch replays the hysteresis chain over ceil(m / 256) records and
takes the exact scan over the ratios only from a segment that it would enter through a tie.  With n = L mod d pivots pending
and 1 <= n <= d - 2 the row launch leaves one partial argmin per workgroup and no hand-off; the next step's column launch
(n >= 2) reduces the partials itself and patches the record.  tests/test_scan_records_ref.py has the arithmetic of the
records in NumPy; here every run is compared with oracle.primal_tableau on the same input and cap: status, pivot count, trace,
basis and the SHA-256 of the whole float64 tableau.  No tolerances.

The pair serves handles above SELP_MIN_MB, so the small LPs go into wider handles (test_gpu_select_only._open).
LPX_PIVOT_DEFER and LPX_GRAPH are read once per process: one child per setting, the resident kernels off."""
import functools
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from linear_programming_solver_lpr381_amd import synth
from test_gpu_deferred_matrix import FULL, _h, _run, _same
from test_gpu_select_only import MIN_BYTES, _check, _tall
from test_gpu_select_only import _lp as _select_lp
from test_gpu_select_only import _shape_of as _select_shape_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
SELC_ROWS = 256
DUP_PAIRS = [(10, 11), (300, 301), (40, 40 + SELC_ROWS), (500, 500 + SELC_ROWS), (1000, 1030), (1023, 1024), (700, 1099)]
ZERO_BLOCK = slice(SELC_ROWS, 2 * SELC_ROWS)


@functools.lru_cache(maxsize=None)
def _own_lp(name):
    if name == "dup":
        # 1100 constraints, 40 columns; seven constraints made tight and written twice: at distance 1 (inside a record, and
        # over the record edge at row 1024), at distance SELC_ROWS (neighbouring records, same lane), and further apart.  A
        # duplicated row has the ratio of its original bit for bit until one of them is the pivot row.
        c, A, b = synth.dense_lp(1100, 40, seed=3)
        for a, d in DUP_PAIRS:
            b[a] *= 0.6
            A[d] = A[a]; b[d] = b[a]
        return synth.primal_tableau_from(c, A, b)
    if name == "zero-block":
        # 600 constraints whose rows 256 .. 511 are zero in every structural column: no pivot changes them, so the second
        # workgroup of the column launch has no eligible row at any pivot and writes a +inf record
        c, A, b = synth.dense_lp(600, 40, seed=3)
        A[ZERO_BLOCK] = 0.0
        return synth.primal_tableau_from(c, A, b)
    raise KeyError(name)


def _lp(name):
    if name in ("dup", "zero-block"):
        T, basis = _own_lp(name)
        return T.copy(), basis.copy()
    return _select_lp(name)


def _open(name):
    """The LP in a handle of its own rows and enough columns to lie above SELP_MIN_MB."""
    R, C = _lp(name)[0].shape if name in ("dup", "zero-block") else _select_shape_of(name)
    assert 8 * R * ((C + 15) // 16 * 16) <= MIN_BYTES
    return [["alloc", R, MIN_BYTES // (8 * R) + 32], ["shape", name]]


_CHILD = """
    import hashlib, json, sys, numpy as np
    sys.path.insert(0, %r)
    import linear_programming_solver_lpr381_amd as L
    from test_gpu_select_records import _lp
    h = lambda a, dt: hashlib.sha256(np.ascontiguousarray(a, dtype=dt).view(np.uint8)).hexdigest()
    out, dt = [], None
    for step in json.loads(sys.argv[1]):
        op = step[0]
        if op == "alloc":
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


def _child(plan, d, graph=True, timeout=300):
    e = dict(os.environ, PYTHONPATH=ROOT, LPX_RESIDENT="0", LPX_PIVOT_DEFER=str(d))
    if not graph:
        e["LPX_GRAPH"] = "0"
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(_CHILD), json.dumps(plan)], env=e, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def ref(oracle):
    """ref(lp, cap) -> ([status, pivots, trace, basis, tableau] as a child reports them, the trace as rows of (r, q));
    computed once per (lp, cap)."""
    @functools.lru_cache(maxsize=None)
    def get(name, cap):
        T, basis = _lp(name)
        st, tr = oracle.primal_tableau(T, basis, max_iter=cap)
        return [int(st), len(tr), _h(tr, np.int32), _h(basis, np.int32), _h(T, np.float64)], np.asarray(tr).reshape(-1, 2)
    return get


# ---------------------------------------------------------------------------------------------------------------------------
# 1. row edges: the last record short by a row, full, one row over, and three records with one row in the last
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 3, 2])
def test_row_edges_vs_oracle(ref, d):
    """m = 255, 256, 257 and 513 constraints, to the end.  d = 16: hand-offs dropped on 14 steps of 16; d = 3: dropped and kept
    in turn; d = 2: always kept."""
    plan, want = [], []
    for m in (SELC_ROWS - 1, SELC_ROWS, SELC_ROWS + 1, 2 * SELC_ROWS + 1):
        lp = _tall(m + 1)
        plan += _open(lp) + [_run(FULL)]
        want.append(ref(lp, FULL)[0])
        assert want[-1][0] == 0 and want[-1][1] > 2 * d, lp
    _check(_child(plan, d), want, d)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. ties: the exact scan taking over at a record that is not a multiple of 1024 rows in
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [12, 16])
def test_ties_vs_oracle(ref, d):
    """"ties-low" and "ties-high" (1801 rows, zero-ratio pivots with several rows tied and near-ties inside the band; the
    second keeps its ties behind row 1100, so the exact scan starts at record 4: row 1024 is not where it begins), then "dup":
    duplicated constraints at distances 1, SELC_ROWS and across row 1024.  To the end."""
    w, tr = ref("dup", FULL)
    firsts = {a for a, _ in DUP_PAIRS}
    assert sum(int(r) in firsts for r in tr[:, 0]) >= 5, tr[:, 0]       # tied winners do occur: a first row of a pair leaves
    assert {10, 40, 1023} <= {int(r) for r in tr[:, 0]}                 # at distance 1, SELC_ROWS and across row 1024
    plan, want = [], []
    for lp in ("ties-low", "ties-high", "dup"):
        plan += _open(lp) + [_run(FULL)]
        want.append(ref(lp, FULL)[0])
    assert want[0][1] >= 25 and want[1][1] >= 25
    _check(_child(plan, d), want, d)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. a record of +inf; UNBOUNDED and OPTIMAL found with pivots pending
# ---------------------------------------------------------------------------------------------------------------------------
def test_ineligible_block_unbounded_and_optimal_by_the_column_launch(ref, oracle):
    """d = 16.  "zero-block": the entering column is zero in all of rows 256 .. 511 at every pivot.  "late-unbounded" ends
    UNBOUNDED (every record +inf) after 500 pivots, 4 pending.  _tall(257) ends OPTIMAL after 75 pivots: 75 mod 16 = 11, so the
    column launch of step 75 reduces the partials of step 74 itself and finds no entering column."""
    w, tr = ref("zero-block", FULL)
    T0, _ = _lp("zero-block")
    assert w[0] == 0 and w[1] >= 20 and not T0[ZERO_BLOCK, :40].any()
    for k in (0, w[1] // 2, w[1] - 1):                  # the block is ineligible in the entering column of pivot k
        T, basis = _lp("zero-block")
        if k:
            oracle.primal_tableau(T, basis, max_iter=k)
        assert np.all(T[ZERO_BLOCK, tr[k, 1]] <= 1e-9) and np.any(T[:SELC_ROWS, tr[k, 1]] > 1e-9)
    u, o = ref("late-unbounded", FULL)[0], ref(_tall(SELC_ROWS + 1), FULL)[0]
    assert u[0] == 1 and 2 <= u[1] % 16 <= 14
    assert o[0] == 0 and 2 <= o[1] % 16 <= 14
    plan = _open("zero-block") + [_run(FULL)] + _open("late-unbounded") + [_run(FULL)] + _open(_tall(SELC_ROWS + 1)) + [_run(FULL)]
    _check(_child(plan, 16), [w, u, o], "ends")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. stale records: a handle whose earlier LP had more rows
# ---------------------------------------------------------------------------------------------------------------------------
def test_stale_records_of_a_taller_lp(ref):
    """d = 16.  One handle takes the 513-constraint LP (three records) and then "dense" (302 rows: two records, the third one
    stale); a handle of 3000 rows (twelve records of capacity) takes "dense"."""
    tall, dense = ref(_tall(2 * SELC_ROWS + 2), FULL)[0], ref("dense", FULL)[0]
    plan = _open(_tall(2 * SELC_ROWS + 2)) + [_run(FULL), ["shape", "dense"], _run(FULL), ["alloc", 3000, 3000], ["shape", "dense"], _run(FULL)]
    _check(_child(plan, 16), [tall, dense, dense], "stale")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the iteration cap at every pending count, and a run continued behind a dropped hand-off
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 16])
def test_caps_at_every_pending_count(ref, d):
    """"dense", caps 1 .. 2d + 1 with restore() between: the cap is met by a launch of every pending count, behind kept and
    dropped hand-offs.  Then cap d // 2 + 1 -- its last pivot comes from a row launch that dropped its hand-off, so the record
    the run ends on never had an entering column -- and, without restore(), on to the end."""
    caps = list(range(1, 2 * d + 2))
    plan, want = _open("dense"), []
    for cap in caps:
        plan += [["restore"], _run(cap)]
        want.append(ref("dense", cap)[0])
    k = d // 2 + 1
    assert 1 <= (k - 1) % d <= d - 2                    # the launch that selects pivot k - 1 drops its hand-off
    plan += [["restore"], _run(k), _run(FULL)]
    got = _child(plan, d)
    _check(got[:len(caps)], want, d)
    for cap, g in zip(caps, got):
        assert g[0] == 3 and g[1] == cap, (d, cap, g[:3])
    full = ref("dense", FULL)[0]
    assert _same(got[-2], ref("dense", k)[0]), (d, k)
    last = got[-1]
    assert [last[0], k + last[1], last[5], last[6]] == [full[0], full[1], full[3], full[4]], (d, last[:2], full[:2])


# ---------------------------------------------------------------------------------------------------------------------------
# 6. graph replay and eager launches
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_graph_and_eager_vs_oracle(ref, graph):
    """d = 16: "dense" to cap 37 and to the end, "dup" to the end, with the captured graph and with LPX_GRAPH=0."""
    plan = _open("dense") + [_run(37), ["restore"], _run(FULL)] + _open("dup") + [_run(FULL)]
    want = [ref("dense", 37)[0], ref("dense", FULL)[0], ref("dup", FULL)[0]]
    _check(_child(plan, 16, graph=graph), want, graph)
