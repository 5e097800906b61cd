"""The select-only step of the deferred-pivot primal loop as two launches -- lpx_pivot_ratio (the column launch: one row per
lane, SELC_ROWS rows per workgroup, the grid sized by the handle's capacity) and lpx_pivot_select (the row launch, which reads
the column launch's ratios from the handle's ratio buffer) -- pinned to the CPU oracle at the shapes where the split can go wrong.

Every run is compared with oracle.primal_tableau on the same input and cap: status, pivot count, trace, basis and the SHA-256 of
the whole float64 tableau.  No tolerances.  The set-up is tests/test_gpu_select_only.py's: one child process per environment,
resident kernels off, the LP placed into a handle just above SELP_MIN_MB through lpx_tableau_set_shape (the host runs the pair on
handles above SELP_MIN_MB with at most SELP_LDS_ROWS rows).

`launches` of lpx_stats counts the steps of the loop (the prologue, every enqueued step, the flush), not kernels: a select-only
step of this form is two kernels and counts once (tests/test_gpu_distributed.py pins the headline run to one count per pivot)."""
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from test_gpu_deferred_matrix import FULL, _h, _run, _same
from test_gpu_select_only import BLOCK_HDR, CAP, ROOT, TESTS, _check, _child, _lp, _open, _tall, ref  # noqa: F401 (ref: fixture)

pytestmark = pytest.mark.gpu


def _selc_rows():
    with open(BLOCK_HDR) as f:
        m = re.search(r"static\s+constexpr\s+int\s+SELC_ROWS\s*=\s*(\d+)\s*;", f.read())
    assert m, "SELC_ROWS not found as an integer literal"
    return int(m.group(1))


S = _selc_rows()
D = 12
ENV = {"LPX_PIVOT_DEFER": str(D)}
# oracle pivot counts of lp:{R-1}:40:3 to the end, by R (checked again below, on the CPU)
PIVOTS = {255: 32, 256: 53, 257: 75, 513: 58, 63: 26, 64: 29, 65: 23, 127: 47, 128: 53, 129: 18}
EDGES = [S - 1, S, S + 1, 2 * S + 1]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. row-split edges: a workgroup one row short, exactly one, one and the objective row alone in the next, two and a row
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", EDGES, ids=["S-1", "S", "S+1", "2S+1"])
def test_row_split_edges_vs_oracle(ref, R):
    """Tall LPs at d = 12, to the end: the oracle ends OPTIMAL after at least 13 pivots, and not on a multiple of 12, so
    optimality is found by the pair with pivots pending.  R = SELC_ROWS + 1 puts the objective row alone into the last
    workgroup: one live lane, which also stores T[m, q]."""
    lp = _tall(R)
    want = ref(lp, FULL)
    assert want[0] == 0 and want[1] >= 13 and want[1] % D != 0, want[:2]
    assert want[1] == PIVOTS[R], (R, want[1])
    _check(_child(_open(lp) + [_run(FULL)], ENV), [want], R)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. capacity above shape: the column grid follows the capacity, workgroups past the live rows leave without a store
# ---------------------------------------------------------------------------------------------------------------------------
def test_capacity_above_shape_vs_oracle(ref):
    """"dense" (302 x 589) in a 3000 x 3000 handle (12 column workgroups, 2 live) and in a SELP_LDS_ROWS x 900 handle (40, and all
    8 * SELP_LDS_ROWS bytes of dynamic LDS in the row launch); d = 12, to the end."""
    want = ref("dense", FULL)
    plan = [["alloc", 3000, 3000], ["shape", "dense"], _run(FULL), ["alloc", CAP, 900], ["shape", "dense"], _run(FULL)]
    _check(_child(plan, ENV), [want, want], "capacity")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. two handles alternating: the ratio buffer belongs to the handle, and a run never sees the ratios of the run before it
# ---------------------------------------------------------------------------------------------------------------------------
_CHILD2 = """
    import hashlib, json, sys, numpy as np
    sys.path.insert(0, %r)
    import linear_programming_solver_lpr381_amd as L
    from test_gpu_select_only import _lp
    h = lambda a, dt: hashlib.sha256(np.ascontiguousarray(a, dtype=dt).view(np.uint8)).hexdigest()
    out, hs = [], {}
    for step in json.loads(sys.argv[1]):
        op, k = step[0], step[1]
        if op == "alloc":
            hs[k] = L.DeviceTableau(step[2], step[3])
        elif op == "shape":
            T, basis = _lp(step[2])
            L._lib.check(L._lib.lib().lpx_tableau_set_shape(hs[k]._h, T.shape[0], T.shape[1]))
            hs[k].R, hs[k].C = T.shape
            hs[k].upload(T, basis)
            hs[k].snapshot()
        elif op == "restore":
            hs[k].restore()
        elif op == "run":
            status, st = hs[k].primal_run(L.default_opts(False, max_iter=step[2], resident=-1))
            Tg, bg = hs[k].download()
            tr = hs[k].trace()
            out.append([int(status), int(st["pivots"]), int(st["launches"]), int(st["update_launches"]),
                        h(tr, np.int32), h(bg, np.int32), h(Tg, np.float64), None])
    for dt in hs.values():
        dt.close()
    print(json.dumps(out))
""" % TESTS


def test_two_handles_alternating_vs_oracle(oracle):
    """"dense" and "dense2" on two 3000 x 3000 handles (72 MB each), interleaved: cap 13 on both, restore, cap 23 on both, then
    to the end on both without a restore (the third run of a handle continues where its second stopped).  The oracle is run the
    same way: 13 from the start, 23 from the start, then on from there."""
    plan, want = [], []
    for k, lp in enumerate(("dense", "dense2")):
        plan += [["alloc", k, 3000, 3000], ["shape", k, lp]]
    state = {}
    for i, cap in enumerate((13, 23, FULL)):
        for k, lp in enumerate(("dense", "dense2")):
            if i == 1:
                plan.append(["restore", k])
            plan.append(["run", k, cap])
            if i < 2:
                state[k] = _lp(lp)
            T, basis = state[k]
            st, tr = oracle.primal_tableau(T, basis, max_iter=cap)
            want.append([int(st), len(tr), _h(tr, np.int32), _h(basis, np.int32), _h(T, np.float64)])
    assert [w[:2] for w in want[:4]] == [[3, 13], [3, 13], [3, 23], [3, 23]] and want[4][0] == 0 and want[5][0] == 0
    assert want[4][1] % D != 0 or want[5][1] % D != 0          # an end found with pivots pending
    e = dict(os.environ, PYTHONPATH=ROOT, LPX_RESIDENT="0", **ENV)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(_CHILD2), json.dumps(plan)], env=e, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    _check(json.loads(r.stdout.strip().splitlines()[-1]), want, "two handles")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. graph and eager at small batches, and what `launches` counts
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["1", "0"], ids=["graph", "eager"])
def test_graph_and_eager_small_batches_vs_oracle(ref, graph):
    """"dense" at d = 12 with batch 1 and 7 (both rounded up to 2d = 24), caps 13, 25 and the end.  launches = 1 (the prologue)
    + the enqueued steps, whole batches of 24 -- at least one step per pivot, at most the poll lag and the batch ahead
    more -- + 1 for the flush when pivots are pending at the end."""
    plan, want = [["alloc", 3000, 3000], ["shape", "dense"]], []
    for batch in (1, 7):
        for cap in (13, 25, FULL):
            plan += [["restore"], _run(cap, batch=batch)]
            want.append(ref("dense", cap))
    env = dict(ENV)
    if graph == "0":
        env["LPX_GRAPH"] = "0"
    got = _child(plan, env)
    _check(got, want, graph)
    for g in got:
        pivots, launches = g[1], g[2]
        steps = launches - 1 - (1 if pivots % D else 0)
        assert steps % (2 * D) == 0 and pivots <= steps <= pivots + 2 + 2 * (2 * D), (graph, pivots, launches)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. profile run: one event pair brackets the two launches of a select-only step
# ---------------------------------------------------------------------------------------------------------------------------
def test_profile_run_same_bits_and_one_sweep_per_12(ref):
    """"dense" in a 3000 x 3000 handle, plain and profile=1, to the end: the same bits, and the launches counted as updates are
    the sweeps."""
    want = ref("dense", FULL)
    plan = [["alloc", 3000, 3000], ["shape", "dense"], _run(FULL), ["restore"], _run(FULL, profile=1)]
    got = _child(plan, ENV)
    _check(got, [want, want], "profile")
    assert got[0][4:7] == got[1][4:7]
    assert abs(got[1][3] - got[1][1] // D) <= 1, got[1][:4]
