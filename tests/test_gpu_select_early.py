"""The select-only pair with the row launch's operands issued early (lpx_pivot_ratio, lpx_pivot_select in lpx_pivot_fused.hip),
pinned to the CPU oracle bit for bit at the shapes where the new order of loads can go wrong.

The row launch issues, beside its first round of loads, everything whose address follows from the launch arguments alone: the
pending pivot rows of its columns and the pending pivots' rows; behind the record the objective row and the pending pivots'
scalars that need q or the live m; behind r only three loads.  The live shape arrives in that first round, so the early loads
follow the CAPACITY of the handle: a workgroup owns ceil(Ccap / nsel) columns of the capacity (not of the live columns) and guards
what it feeds and stores by the live C.  What a lane past the live columns loads is whatever an earlier LP left in the handle.
The block argmin of the row launch takes one barrier.  (The column launch's counterpart -- its factor columns by the capacity's
rows, its scan record in one exchange: tests/test_select_exchange_ref.py -- was measured and is not in the kernel; the cases on
the rows stay, they cost a second each.)

Hence the cases: capacity != live shape in either direction, with the live edge inside a workgroup's share, on its edge and
workgroups wholly past it; handles that held a larger LP before (one of them UNBOUNDED: every ratio it left is +inf); every pending
count n = 1 .. 15 with runs that end on n = 0, 1, d - 2, d - 1 and resume; duplicated constraints inside a wave, across waves and
across workgroups; the captured graph against eager launches.  Every run is compared with oracle.primal_tableau on the same input
and cap: status, pivot count, trace, basis and the SHA-256 of the whole float64 tableau.  No tolerances.

The pair serves handles above SELP_MIN_MB, so the small LPs go into larger handles through lpx_tableau_set_shape.
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
from test_gpu_select_only import K, MIN_BYTES, _check, _tall
from test_gpu_select_records import _lp as _records_lp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
SELC_ROWS = 256
SELP_NT, MB_NT = K["SELP_NT"], K["MB_NT"]
# (first, copy) rows of "dup-waves": inside one wave; in waves 0 and 1 of the first workgroup of the column launch; in waves 0 and
# 3 of the second; in the same lane of neighbouring workgroups; far apart
DUP_PAIRS = [(50, 51), (20, 100), (SELC_ROWS + 44, SELC_ROWS + 224), (40, 40 + SELC_ROWS), (130, 590)]


@functools.lru_cache(maxsize=None)
def _own_lp(name):
    if name == "dup-waves":
        # 600 constraints, 40 columns; five constraints made tight and written twice.  A duplicated row has the ratio of its
        # original bit for bit until one of them is the pivot row
        c, A, b = synth.dense_lp(600, 40, seed=3)
        for a, d in DUP_PAIRS:
            b[a] *= 0.6
            A[d] = A[a]; b[d] = b[a]
        return synth.primal_tableau_from(c, A, b)
    if name == "big":
        # 901 x 1201: four scan records, more rows and columns than every small LP that follows it in a handle
        return synth.primal_tableau_from(*synth.dense_lp(900, 300, seed=7))
    if name == "big-unbounded":
        # "big" plus a zero column of cost 0.01: it enters last, and the run ends UNBOUNDED with every ratio and every scan record
        # of its 900 rows at +inf and its pending pivots left in the ring
        c, A, b = synth.dense_lp(900, 300, seed=7)
        return synth.primal_tableau_from(np.append(c, 0.01), np.hstack([A, np.zeros((900, 1))]), b)
    raise KeyError(name)


def _lp(name):
    if name in ("dup-waves", "big", "big-unbounded"):
        T, basis = _own_lp(name)
        return T.copy(), basis.copy()
    return _records_lp(name)                            # "dup", and through it the LPs of the tests before


def _alloc(R, C):
    assert 8 * R * ((C + 15) // 16 * 16) > MIN_BYTES, (R, C)
    return ["alloc", R, C]


_CHILD = """
    import hashlib, json, sys, numpy as np
    sys.path.insert(0, %r)
    import linear_programming_solver_lpr381_amd as L
    from test_gpu_select_early import _lp
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
# 1. capacity != live columns
# ---------------------------------------------------------------------------------------------------------------------------
WIDE_C = 32 * SELP_NT + 100                     # 32 workgroups of 516 columns: a lane with a second column pass
EDGE_C = 32 * 589                               # 32 workgroups of exactly "dense"'s 589 columns


@pytest.mark.parametrize("d", [16, 3])
def test_capacity_columns_vs_oracle(ref, d):
    """"dense" (302 x 589) to the end in three handles.  3000 x 3000: 12 workgroups of 250 columns, the live edge inside the
    third, nine wholly past it.  520 x (32 SELP_NT + 100): 32 workgroups of 516, the first with four lanes on a second pass, the
    edge inside the second.  460 x (32 x 589): the live edge exactly on the first workgroup's, which takes a second pass for 77
    columns, and 31 workgroups wholly past it."""
    assert (3000 + MB_NT - 1) // MB_NT == 12 and (WIDE_C + 31) // 32 == SELP_NT + 4 and (EDGE_C + 31) // 32 == 589
    assert _lp("dense")[0].shape == (302, 589)
    want = ref("dense", FULL)[0]
    assert want[0] == 0 and want[1] > 2 * d
    plan = []
    for R, C in ((3000, 3000), (520, WIDE_C), (460, EDGE_C)):
        plan += [_alloc(R, C), ["shape", "dense"], _run(FULL)]
    _check(_child(plan, d), [want] * 3, d)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. capacity != live rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 2])
def test_capacity_rows_vs_oracle(ref, d):
    """m = SELC_ROWS - 1, SELC_ROWS, SELC_ROWS + 1 constraints (the objective row last in the first workgroup of the column
    launch, first in the second, second in the second) in one handle of 1100 rows: five workgroups, at least three of them past
    the live rows, over rows of the handle that the LP before left behind."""
    plan, want = [_alloc(1100, 7700)], []
    for m in (SELC_ROWS + 1, SELC_ROWS, SELC_ROWS - 1):
        lp = _tall(m + 1)
        plan += [["shape", lp], _run(FULL)]
        want.append(ref(lp, FULL)[0])
        assert want[-1][0] == 0 and want[-1][1] > 2 * d, lp
    _check(_child(plan, d), want, d)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. stale data behind the live shape
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["big", "big-unbounded"])
def test_stale_handle_vs_oracle(ref, first):
    """d = 16.  A handle of 1100 x 7700 takes a 901-row LP to its end and then, unchanged, "dense" and the 257-row LP: the ring,
    the ratio buffer, the scan records and the rows and columns past the live shape hold the first LP's values.  "big-unbounded"
    ends UNBOUNDED with pivots pending: all its ratios and records are +inf, and the ring is left as the run stopped."""
    big, dense, tall = ref(first, FULL)[0], ref("dense", FULL)[0], ref(_tall(SELC_ROWS + 1), FULL)[0]
    assert big[0] == (1 if first == "big-unbounded" else 0) and big[1] > 300
    if first == "big-unbounded":
        assert big[1] % 16 != 0                         # pivots pending when it ends
    plan = [_alloc(1100, 7700), ["shape", first], _run(FULL), ["shape", "dense"], _run(FULL), ["shape", _tall(SELC_ROWS + 1)], _run(FULL)]
    _check(_child(plan, 16), [big, dense, tall], first)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. pending counts: runs that end on n = 0, 1, d - 2, d - 1 and resume
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3, 12, 16])
def test_pending_counts_end_and_resume(ref, d):
    """"dense" in the 3000 x 3000 handle.  A run to the end passes n = 1 .. d - 1 on every period (d = 12, 16: both SELP_SB
    groups; the hand-off kept at n = 0 and d - 1, dropped between).  Caps d, d + 1, 2d - 2, 2d - 1 end a run with 0, 1, d - 2 and
    d - 1 pivots pending (the flush applies them); each is followed, without restore(), by a second run to the end."""
    caps = sorted({d, d + 1, 2 * d - 2, 2 * d - 1})
    assert {k % d for k in caps} == {0, 1 % d, (d - 2) % d, d - 1}
    plan = [_alloc(3000, 3000), ["shape", "dense"], _run(FULL)]
    for k in caps:
        plan += [["restore"], _run(k), _run(FULL)]
    got = _child(plan, d)
    full = ref("dense", FULL)[0]
    assert _same(got[0], full), (d, got[0][:2], full[:2])
    for n, k in enumerate(caps):
        part, rest = got[1 + 2 * n], got[2 + 2 * n]
        assert part[0] == 3 and _same(part, ref("dense", k)[0]), (d, k, part[:2])
        assert [rest[0], k + rest[1], rest[5], rest[6]] == [full[0], full[1], full[3], full[4]], (d, k, rest[:2], full[:2])


# ---------------------------------------------------------------------------------------------------------------------------
# 5. ties: duplicated constraints inside a wave, across waves, across workgroups
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 3])
def test_duplicated_rows_vs_oracle(ref, d):
    """"dup-waves" and the "dup" of test_gpu_select_records (pairs at distance 1, SELC_ROWS and across row 1024) to the end: a
    tied minimum makes the record "not alone", whether the copy sits in the same wave or another, and the row launch takes the
    exact scan.  The oracle's trace shows that first rows of pairs do leave."""
    w, tr = ref("dup-waves", FULL)
    left = {int(r) for r in tr[:, 0]}
    assert w[0] == 0 and {50, 20, SELC_ROWS + 44} <= left, sorted(left)      # in-wave, across waves (either workgroup)
    assert 40 in left or 130 in left                                         # across workgroups
    plan = [_alloc(1110, 7700), ["shape", "dup-waves"], _run(FULL), ["shape", "dup"], _run(FULL)]
    _check(_child(plan, d), [w, ref("dup", FULL)[0]], d)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. graph replay against eager launches
# ---------------------------------------------------------------------------------------------------------------------------
def test_graph_and_eager_same_bits(ref):
    """d = 16: "dense" in the 3000 x 3000 handle to cap 37 and to the end, "dup-waves" to the end -- with the captured graph and
    with LPX_GRAPH=0: the same bits, and the oracle's."""
    plan = [_alloc(3000, 3000), ["shape", "dense"], _run(37), ["restore"], _run(FULL), _alloc(1100, 7700), ["shape", "dup-waves"], _run(FULL)]
    want = [ref("dense", 37)[0], ref("dense", FULL)[0], ref("dup-waves", FULL)[0]]
    g, e = _child(plan, 16, graph=True), _child(plan, 16, graph=False)
    assert [x[:2] + x[4:7] for x in g] == [x[:2] + x[4:7] for x in e]
    _check(g, want, "graph")
    _check(e, want, "eager")
