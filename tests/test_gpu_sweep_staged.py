"""The deferred sweep at its deepest (lpx_pivot_fused<d>, d up to 16: the default of handles that cannot live in the Infinity
Cache) pinned to the CPU oracle at row, column and pending-row edges, and the default depth of every size tier.

A sweep wave owns fp_rows(d) rows (8 for d >= 3, read from lpx_pivot_fused.hip) of one 128-column window; a wave whose rows hold
a pending pivot's row, or run past R, takes the row-wise path.  B is two such tiles: R = B, B + 1, 2B - 1 and 2B + 1 are two and
four tiles, exact, plus a row and less a row; ld = 256, 272 and 112 end on a full window, on 8 live lanes and inside the first
window; the pending-row case puts pivot rows on the first and last row of a B-row block (a tile's first and last row too) and
into the last, partial one.  Every run is compared with oracle.primal_tableau on the same input and cap: status, pivot count,
trace, basis and the SHA-256 of the whole float64 tableau.  No tolerances.  tests/test_gpu_deferred_matrix.py remains the matrix
over every depth, flush length and run shape.

The environment switches are read once per process, hence one child process per setting, with the resident kernels off; the
children run with LPX_UPDATE_POLICY=2, so that small tableaux take the streaming kernels.

The tall and wide LPs are synth.dense_lp at the seed, of the first hundred or so, whose oracle run is the longest: the small
ones end after a few dozen pivots, and a run of at most d pivots never sweeps.  The tests assert the lengths they rely on."""
import os
import re

import pytest

from test_gpu_deferred_matrix import FULL, _run, _same
from test_gpu_select_only import _check, _child, _lp, _open, _tall, _wide, ref  # noqa: F401  (ref: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "csrc")


def _constants():
    env = {}
    with open(os.path.join(CSRC, "lpx_block.h")) as f:
        text = f.read()
    for name in ("FP_DMAX",):
        m = re.search(r"static\s+constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, f"{name} not found as an integer literal"
        env[name] = int(m.group(1))
    with open(os.path.join(CSRC, "lpx_tile.h")) as f:
        m = re.search(r"UPD_STREAM_BYTES\s*=\s*\(size_t\)\s*(\d+)\s*<<\s*20\s*;", f.read())
    assert m, "UPD_STREAM_BYTES not found as MiB << 20"
    env["UPD_STREAM_BYTES"] = int(m.group(1)) << 20
    with open(os.path.join(CSRC, "lpx_pivot_fused.hip")) as f:
        m = re.search(r"constexpr\s+int\s+fp_rows\(int D\)\s*\{\s*return\s+D\s*<=\s*2\s*\?\s*UPDS_ROWS\s*:\s*(\d+)\s*;", f.read())
    assert m, "fp_rows: rows per sweep wave at d >= 3 not found as an integer literal"
    env["FP_ROWS"] = int(m.group(1))
    return env


K = _constants()
TILE = K["FP_ROWS"]             # rows per sweep wave at d >= 3
B = 2 * TILE
STREAMING = {"LPX_UPDATE_POLICY": "2"}

# R -> seed of the longest oracle run among seeds 1 .. 119 (26, 39, 51 and 41 pivots).  Chosen at B = 16: after a change of the
# tile the row-edge test asks for new seeds (its assertion on the run's length) and the pending-row test for a new LP
_TALL_SEEDS = {16: 100, 17: 39, 31: 8, 33: 64}
# the LP of about 2B + 3 rows whose trace test_pending_rows_inside_a_workgroups_rows checks
_BLOCKS_LP = f"lp:{2 * B + 2}:40:97"


def _sweeps(trace, d):
    """The pending rows of every sweep of a run with this trace: launch L, a positive multiple of d, applies pivots L - d .. L - 1
    if the run is still going, that is if pivot L was selected."""
    rows = [int(r) for r, _ in trace]
    return [rows[L - d:L] for L in range(d, len(rows), d)]


def _trace(oracle, name, cap=FULL):
    T, basis = _lp(name)
    st, tr = oracle.primal_tableau(T, basis, max_iter=cap)
    return int(st), tr.tolist()


def test_constants_and_cases():
    assert K["FP_DMAX"] == 16 and TILE >= 2 and B + 5 < 128     # d = 16 below is the deepest kernel
    assert set(_TALL_SEEDS) == {B, B + 1, 2 * B - 1, 2 * B + 1}  # the seeds were chosen for these R


# ---------------------------------------------------------------------------------------------------------------------------
# 1. row edges: B rows, B and a row, 2B less a row, 2B and a row
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixmod", ["1", "2"])
@pytest.mark.parametrize("d", [3, 16])
@pytest.mark.parametrize("R", [B, B + 1, 2 * B - 1, 2 * B + 1], ids=["B", "B+1", "2B-1", "2B+1"])
def test_row_edges_vs_oracle(ref, oracle, R, d, mixmod):
    """R counts the objective row.  To the end and to caps d + 1, 2d and 3d + 2, with every row block and with every second one
    keeping its last row in the cache."""
    lp = _tall(R, seed=_TALL_SEEDS.get(R, 3))
    assert len(_trace(oracle, lp)[1]) > 16                      # at d = 16 too the run sweeps at least once
    caps = [FULL, d + 1, 2 * d, 3 * d + 2]
    plan, want = [["open", lp]], []
    for cap in caps:
        plan += [["restore"], _run(cap)]
        want.append(ref(lp, cap))
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER=str(d), LPX_UPDATE_MIXMOD=mixmod)), want, (R, d, mixmod))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. column edges: every window full, a last window of 8 live lanes, one partial window
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,ld,seed", [(256, 256, 5), (260, 272, 22), (100, 112, 1)], ids=["ld256", "ld272", "C100"])
def test_column_edges_vs_oracle(ref, oracle, C, ld, seed):
    """m = B + 5 constraints: two full tiles and a partial one.  d = 12, to cap 25 (two sweeps, one pivot pending) and to the end."""
    lp = _wide(C, B + 5, seed=seed)
    assert (C + 15) // 16 * 16 == ld
    assert len(_trace(oracle, lp)[1]) > 36                      # three sweeps
    plan, want = [["open", lp]], []
    for cap in (25, FULL):
        plan += [["restore"], _run(cap)]
        want.append(ref(lp, cap))
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER="12")), want, C)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. pending rows on the edges of B-row blocks
# ---------------------------------------------------------------------------------------------------------------------------
def _blocks_lp_sweeps(oracle):
    R = 2 * B + 3
    st, tr = _trace(oracle, _BLOCKS_LP)
    sweeps = _sweeps(tr, 16)
    assert st == 0 and len(sweeps) >= 2
    two = any(len({r for r in set(p) if r // B == blk}) >= 2 for p in sweeps for blk in range((R + B - 1) // B))
    first = any(r % B == 0 for p in sweeps for r in p)
    last = any(r % B == B - 1 for p in sweeps for r in p)
    partial = any(r // B == (R - 1) // B for p in sweeps for r in p)
    assert (R - 1) // B == 2 and R % B != 0                     # the last block is partial
    return two, first, last, partial


def test_pending_rows_inside_a_workgroups_rows(ref, oracle):
    """An LP of 2B + 3 rows at d = 16 whose sweeps, by the oracle's trace, hold: two pending rows in one B-row block, one at a
    block's first row, one at a block's last row, one in the last, partial block.  On its own handle (the one-launch select-only
    kernel) and on one above 64 MB (the select-only pair, and some 1900 column windows)."""
    assert _blocks_lp_sweeps(oracle) == (True, True, True, True)
    want = ref(_BLOCKS_LP, FULL)
    plan = [["open", _BLOCKS_LP], _run(FULL)] + _open(_BLOCKS_LP) + [_run(FULL)]
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER="16")), [want, want], "blocks")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. live shape below capacity: the factor ring's stride is the capacity, the rows streamed are the live ones
# ---------------------------------------------------------------------------------------------------------------------------
def test_live_shape_below_capacity_vs_oracle(ref, oracle):
    """A handle of (3B + 5) x 900 takes the LP of 2B + 3 rows through lpx_tableau_set_shape; d = 12.  ("dense" of the matrix test
    has 302 rows and does not fit.)"""
    assert _lp("dense")[0].shape[0] > 3 * B + 5
    assert len(_sweeps(_trace(oracle, _BLOCKS_LP)[1], 12)) >= 3
    want = ref(_BLOCKS_LP, FULL)
    plan = [["alloc", 3 * B + 5, 900], ["shape", _BLOCKS_LP], _run(FULL), ["restore"], _run(25)]
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER="12")), [want, ref(_BLOCKS_LP, 25)], "capacity")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. graph against eager
# ---------------------------------------------------------------------------------------------------------------------------
def test_graph_and_eager_same_bits(ref):
    """The LP of case 3 at d = 16 with batch 1 (rounded up to 32), captured and replayed (the default) and eager."""
    want = ref(_BLOCKS_LP, FULL)
    plan = [["open", _BLOCKS_LP], _run(FULL, batch=1)]
    env = dict(STREAMING, LPX_PIVOT_DEFER="16")
    graph = _child(plan, env)
    eager = _child(plan, dict(env, LPX_GRAPH="0"))
    _check(graph, [want], "graph")
    _check(eager, [want], "eager")
    assert graph[0][4:7] == eager[0][4:7]


# ---------------------------------------------------------------------------------------------------------------------------
# 6. depth tiers: 16 above UPD_STREAM_BYTES, 12 below it (down to 64 MB)
# ---------------------------------------------------------------------------------------------------------------------------
def test_default_depth_tiers_vs_oracle(ref):
    """Two handles of 12000 columns, 100 rows above and 100 rows below the boundary, take "dense" through lpx_tableau_set_shape
    with no LPX_PIVOT_DEFER; a profile run counts the sweeps: one per 16 pivots above, one per 12 below."""
    C = 12000
    assert C % 16 == 0
    rows = K["UPD_STREAM_BYTES"] // (8 * C)
    want = ref("dense", FULL)
    plan = [["alloc", rows + 100, C], ["shape", "dense"], _run(FULL, profile=1),
            ["alloc", rows - 100, C], ["shape", "dense"], _run(FULL, profile=1)]
    above, below = _child(plan, dict(STREAMING))
    assert _same(above, want) and _same(below, want), (above[:2], below[:2], want[:2])
    p = want[1]
    assert p // 16 + 1 < p // 12 - 1                            # the two counts cannot be taken for each other
    assert abs(above[3] - p // 16) <= 1, (p, above[3])
    assert abs(below[3] - p // 12) <= 1, (p, below[3])
