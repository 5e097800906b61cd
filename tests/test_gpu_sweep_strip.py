"""The deferred sweep in strips (fused_sweep_strip: the streaming lpx_pivot_fused<d>, 3 <= d <= 16) pinned to the CPU oracle at
the edges of its strips.

A sweep wave owns one 128-column window and S = FP_STRIP_BLOCKS (lpx_block.h) consecutive blocks of fp_rows(d) = 8 rows, a strip
of 8 S rows; it keeps its d pivot-row pairs in registers over the strip.  A block that holds a pending pivot's row takes a
block-uniform branch, the block that runs past R a per-row loop.  Row edges: R = 8S, 8S + 1, 16S - 1 and 16S + 1 are one strip
exact, a strip and a row, and a last strip whose last block is partial.  Pending rows: on a strip's first and last row, on a
block's first and last row inside a strip, two in one block, in the partial tail block, and hit blocks in front of and behind
blocks of the fast path in one strip.  Column edges: ld = 256, 272 and 112 end on a full window, on 8 live lanes and inside the
first window.  Every run is compared with oracle.primal_tableau on the same input and cap: status, pivot count, trace, basis and
the SHA-256 of the whole float64 tableau.  No tolerances.

The environment switches are read once per process, hence one child process per setting, with the resident kernels off; the
children run with LPX_UPDATE_POLICY=2, so that small tableaux take the streaming kernels.

The seeds were chosen on the CPU with the oracle among seeds 1 .. 399 (rows: the longest runs; pending rows: the traces that
hold the placements); the tests assert what they rely on."""
import os
import re

import pytest

from test_gpu_deferred_matrix import FULL, _run
from test_gpu_select_only import _check, _child, _lp, _open, _tall, _wide, ref  # noqa: F401  (ref: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "csrc")


def _constants():
    env = {}
    with open(os.path.join(CSRC, "lpx_block.h")) as f:
        text = f.read()
    for name in ("FP_DMAX", "FP_STRIP_BLOCKS"):
        m = re.search(r"static\s+constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, f"{name} not found as an integer literal"
        env[name] = int(m.group(1))
    with open(os.path.join(CSRC, "lpx_pivot_fused.hip")) as f:
        m = re.search(r"constexpr\s+int\s+fp_rows\(int D\)\s*\{\s*return\s+D\s*<=\s*2\s*\?\s*UPDS_ROWS\s*:\s*(\d+)\s*;", f.read())
    assert m, "fp_rows: rows per block at d >= 3 not found as an integer literal"
    env["FP_ROWS"] = int(m.group(1))
    return env


K = _constants()
S, H = K["FP_STRIP_BLOCKS"], K["FP_ROWS"]
STRIP = S * H                                                   # rows of a strip
STREAMING = {"LPX_UPDATE_POLICY": "2"}

# R -> the LP of the longest oracle run among seeds 1 .. 399 (48, 39, 51 and 46 pivots: two sweeps at d = 16; with 40 columns no
# LP of 16 rows runs longer than 29 pivots, hence its 100), chosen at a strip of 16 rows: after a change of the strip the tests
# ask for new seeds (their assertions on the runs' lengths and on the placements)
_ROW_LPS = {16: "lp:15:100:127", 17: _tall(17, seed=39), 31: _tall(31, seed=8), 33: _tall(33, seed=216)}
# 2 * STRIP + 3 rows: every placement but a fast block in front of a hit block; 6 * STRIP + 3 rows: that one too
_EDGES_LP = f"lp:{2 * STRIP + 2}:40:156"
_STRIPS_LP = f"lp:{6 * STRIP + 2}:40:100"


def _trace(oracle, name, cap=FULL):
    T, basis = _lp(name)
    st, tr = oracle.primal_tableau(T, basis, max_iter=cap)
    return int(st), [int(r) for r, _ in tr.tolist()]


def _sweeps(rows, d):
    """The pending rows of every sweep of a run with these pivot rows: launch L, a positive multiple of d, applies pivots
    L - d .. L - 1 if the run is still going, that is if pivot L was selected."""
    return [rows[L - d:L] for L in range(d, len(rows), d)]


def _placements(R, sweeps):
    """Which placements of pending rows the sweeps of a run hold, by the kernel's own indexing: block = row // H, strip =
    row // STRIP; a block is full when it ends at or before R."""
    nb = (R + H - 1) // H
    got = set()
    for p in sweeps:
        rows = set(p)
        hit = {r // H for r in rows}
        for r in rows:
            if r % STRIP == 0:
                got.add("strip first row")
            if r % STRIP == STRIP - 1:
                got.add("strip last row")
            if r % H == 0 and r % STRIP != 0:
                got.add("block first row inside a strip")
            if r % H == H - 1 and r % STRIP != STRIP - 1:
                got.add("block last row inside a strip")
            if R % H and r // H == (R - 1) // H:
                got.add("partial tail block")
        if any(len({r for r in rows if r // H == b}) >= 2 for b in range(nb)):
            got.add("two in one block")
        for b in range(nb - 1):
            if b % S != S - 1 and (b + 2) * H <= R:              # b and b + 1: full blocks of one strip
                if b in hit and b + 1 not in hit:
                    got.add("fast block behind a hit block")
                if b in hit and b + 1 in hit:
                    got.add("hit block behind a hit block")
                if b not in hit and b + 1 in hit:
                    got.add("hit block behind a fast block")
    return got


def test_constants_and_cases():
    assert K["FP_DMAX"] == 16 and H == 8 and S >= 2 and 6 * STRIP + 3 < 128     # d = 16 below is the deepest kernel
    assert set(_ROW_LPS) == {STRIP, STRIP + 1, 2 * STRIP - 1, 2 * STRIP + 1}      # the LPs were chosen for these R


# ---------------------------------------------------------------------------------------------------------------------------
# 1. row edges: one strip exact, a strip and a row, two strips less a row (a partial last block), two strips and a row
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixmod", ["1", "2"])
@pytest.mark.parametrize("d", [3, 16])
@pytest.mark.parametrize("R", [STRIP, STRIP + 1, 2 * STRIP - 1, 2 * STRIP + 1], ids=["8S", "8S+1", "16S-1", "16S+1"])
def test_row_edges_vs_oracle(ref, oracle, R, d, mixmod):
    """R counts the objective row.  To the end and to caps d + 1, 2d and 3d + 2, with every row block and with every second one
    keeping its last row in the cache."""
    lp = _ROW_LPS[R]
    assert _lp(lp)[0].shape[0] == R
    assert len(_sweeps(_trace(oracle, lp)[1], d)) >= 2          # at least two sweeps, at d = 16 too
    caps = [FULL, d + 1, 2 * d, 3 * d + 2]
    plan, want = [["open", lp]], []
    for cap in caps:
        plan += [["restore"], _run(cap)]
        want.append(ref(lp, cap))
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER=str(d), LPX_UPDATE_MIXMOD=mixmod)), want, (R, d, mixmod))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. pending rows on the edges of strips and blocks
# ---------------------------------------------------------------------------------------------------------------------------
_EDGES = {"strip first row", "strip last row", "block first row inside a strip", "block last row inside a strip",
          "two in one block", "partial tail block", "fast block behind a hit block", "hit block behind a hit block"}


def test_pending_rows_on_strip_and_block_edges(ref, oracle):
    """An LP of 2 * STRIP + 3 rows at d = 16 whose sweeps, by the oracle's trace, hold a pending row on a strip's first and on a
    strip's last row, on a block's first and last row inside a strip, two in one block, one in the partial tail block, and a
    hit block followed in its strip by a block of the fast path and by another hit block.  On its own handle (the one-launch
    select-only kernel) and on one above 64 MB (the select-only pair, and some 1900 column windows)."""
    R = 2 * STRIP + 3
    st, rows = _trace(oracle, _EDGES_LP)
    sweeps = _sweeps(rows, 16)
    assert st == 0 and len(sweeps) >= 2 and R % H != 0
    assert _placements(R, sweeps) >= _EDGES, _EDGES - _placements(R, sweeps)
    want = ref(_EDGES_LP, FULL)
    plan = [["open", _EDGES_LP], _run(FULL)] + _open(_EDGES_LP) + [_run(FULL)]
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER="16")), [want, want], "edges")


def test_pending_rows_over_six_strips(ref, oracle):
    """An LP of 6 * STRIP + 3 rows at d = 16, four sweeps: every placement of the case above and a hit block behind a block of
    the fast path; to the end and to cap 3d + 2 (two pivots pending behind the third sweep)."""
    R = 6 * STRIP + 3
    st, rows = _trace(oracle, _STRIPS_LP)
    sweeps = _sweeps(rows, 16)
    assert st == 0 and len(sweeps) >= 4
    want_p = _EDGES | {"hit block behind a fast block"}
    assert _placements(R, sweeps) >= want_p, want_p - _placements(R, sweeps)
    plan = [["open", _STRIPS_LP], _run(FULL), ["restore"], _run(50)]
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER="16")), [ref(_STRIPS_LP, FULL), ref(_STRIPS_LP, 50)], "strips")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. column edges: every window full, a last window of 8 live lanes, one partial window
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,ld,seed", [(256, 256, 5), (260, 272, 22), (100, 112, 1)], ids=["ld256", "ld272", "C100"])
def test_column_edges_vs_oracle(ref, oracle, C, ld, seed):
    """m = 8S + 5 constraints: a full strip and a partial block.  d = 12, to cap 25 (two sweeps, one pivot pending) and to the end."""
    lp = _wide(C, STRIP + 5, seed=seed)
    assert (C + 15) // 16 * 16 == ld
    assert len(_sweeps(_trace(oracle, lp)[1], 12)) >= 2
    plan, want = [["open", lp]], []
    for cap in (25, FULL):
        plan += [["restore"], _run(cap)]
        want.append(ref(lp, cap))
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER="12")), want, C)
