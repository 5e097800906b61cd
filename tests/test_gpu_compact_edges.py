"""The compact form of the primal loop where tests/test_gpu_compact.py does not reach: the sweep kernels of depths 4
and 8, a result with nothing pending in either buffer of the pair, the store policies and mix periods, the row edges of the _cm
launches, what runs next on a handle a compact run has used, and the default selection with no switch set.

The rules are those of tests/test_gpu_compact.py, whose child and helpers run every case: status, pivot count, trace, basis and the
SHA-256 of the whole float64 tableau against the CPU oracle, no tolerances, the form of every run asked of the handle, one child
process per environment setting with the resident kernels off.  Depths 4 and 8 on the endings, the re-entries and the reversed
ties are further values of that file's own parametrisations.  Every case asserts, on the CPU, that its LP holds the situation it
is there for before it uses the GPU (tests/test_compact_ref.py has the same assertions without one)."""
import os
import re

import numpy as np
import pytest

import test_compact_ref as CR
from test_gpu_compact import STREAMING, _big, _check, _child, _run, ref  # noqa: F401  (ref: the module's fixture)
from test_gpu_deferred_matrix import FULL, _h
from test_gpu_deferred_matrix import _lp as _matrix_lp
from test_gpu_dual import _dual_tableau
from test_gpu_select_only import MIN_BYTES, _open
from test_gpu_sweep_staged import TILE              # rows per block of a sweep wave at d >= 3

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "csrc")
SWITCHES = ("LPX_UPDATE_POLICY", "LPX_UPDATE_MIXMOD", "LPX_PIVOT_DEFER", "LPX_PIVOT_COMPACT", "LPX_GRAPH")


def _constants():
    """The thresholds of the default selection as the source has them."""
    env = {}
    with open(os.path.join(CSRC, "lpx_tile.h")) as f:
        text = f.read()
    for name in ("FUSED_CACHED_BYTES", "UPD_STREAM_BYTES"):
        m = re.search(r"%s\s*=\s*\(size_t\)\s*(\d+)\s*<<\s*20\s*;" % name, text)
        assert m, f"{name} not found as MiB << 20"
        env[name] = int(m.group(1)) << 20
    m = re.search(r"static\s+constexpr\s+int\s+UPDS_ROWS\s*=\s*(\d+)\s*;", text)
    assert m, "UPDS_ROWS not found as an integer literal"
    env["UPDS_ROWS"] = int(m.group(1))
    with open(os.path.join(CSRC, "lpx_tableau.cpp")) as f:
        text = f.read()
    m = re.search(r"static\s+constexpr\s+int\s+COMPACT_MIN_SWEEPS\s*=\s*(\d+)\s*;", text)
    assert m, "COMPACT_MIN_SWEEPS not found as an integer literal"
    env["COMPACT_MIN_SWEEPS"] = int(m.group(1))
    m = re.search(r"PIVOT_DEFER_STREAM\s*=\s*(\d+)\s*,\s*PIVOT_DEFER_LARGE\s*=\s*(\d+)\s*,", text)
    assert m, "the default depths not found as integer literals"
    env["DEPTH_STREAM"], env["DEPTH_LARGE"] = int(m.group(1)), int(m.group(2))
    return env


K = _constants()


def _ld(C):
    return (C + 15) // 16 * 16                       # lpx_tableau_create


def _bytes(step):
    """Tableau bytes of the handle an "alloc" step makes."""
    assert step[0] == "alloc"
    return 8 * step[1] * _ld(step[2])


def test_constants():
    assert (K["DEPTH_LARGE"], K["DEPTH_STREAM"], K["COMPACT_MIN_SWEEPS"]) == (12, 16, 8)
    assert MIN_BYTES == 64 << 20 < K["FUSED_CACHED_BYTES"] == 152 << 20 < K["UPD_STREAM_BYTES"] == 292 << 20


# ---------------------------------------------------------------------------------------------------------------------------
# B. nothing pending, the result in one buffer and in the other
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 8, 16])
def test_nothing_pending_in_either_buffer_vs_oracle(ref, oracle, d):
    """CR.MAIN to caps d, 2d and 3d: a sweep launch meets the cap, nothing is pending, and after 1, 2 and 3 sweeps the exit pass
    finds the result in either buffer of the pair.  Caps d + 1 and 2d - 1: 1 and d - 1 pivots pending after one sweep."""
    caps = CR.nothing_pending_caps(d, len(CR.oracle_trace(oracle, CR.MAIN)))
    ends = [CR.ended(CR.MAIN, d, cap) for cap in caps]
    assert [e[0] for e in ends] == caps
    assert [e[1:3] for e in ends] == [(1, 0), (2, 0), (3, 0), (1, 1), (1, d - 1)], ends
    assert ends[0][1] % 2 != ends[1][1] % 2 and ends[3][3]
    plan, want = _big(CR.MAIN), []
    for cap in caps:
        plan += [["restore"], _run(cap)]
        want.append(ref(CR.MAIN, cap))
    assert [w[1] for w in want] == caps
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER=str(d))), want, d)


# ---------------------------------------------------------------------------------------------------------------------------
# C. store policy and mix period: they never change a bit
# ---------------------------------------------------------------------------------------------------------------------------
# name -> (environment, the form the handle reports, LPX_UPDATE_MIXMOD or None).  The launcher rescales the period to the sweep
# wave's blocks (_period), so 2 and 3 both come out as 1 -- every block stores its last row through the cache, `rb % period` is
# never asked -- and 7 as 2; 8 and 19 give the odd periods 3 and 7
_STORES = {"all-nt": ({"LPX_UPDATE_POLICY": "1"}, 1, None), "cached": ({"LPX_UPDATE_POLICY": "0"}, 0, None)}
_STORES.update({"mixed-%d" % n: ({"LPX_UPDATE_POLICY": "2", "LPX_UPDATE_MIXMOD": str(n)}, 1, n) for n in (2, 3, 7, 8, 19)})
_PERIODS = {2: 1, 3: 1, 7: 2, 8: 3, 19: 7}          # LPX_UPDATE_MIXMOD -> the period lpx_pivot_fused_cm<12> is launched with


def _period(n):
    """launch_pivot_fused: `if (mixmod > 1) mixmod = std::max(1, mixmod * UPDS_ROWS / rows)`, rows = fp_rows(d) at d >= 3."""
    return max(1, n * K["UPDS_ROWS"] // TILE) if n > 1 else n


def test_mix_periods_reach_the_block_index():
    """The periods the children run with: above 1 they are distinct, one is even and two are odd, and each is far below the number
    of full row blocks of "dense", so that the block index takes every residue of every period several times over."""
    assert (K["UPDS_ROWS"], TILE) == (3, 8) and {n: _period(n) for n in _PERIODS} == _PERIODS
    blocks = _matrix_lp("dense")[0].shape[0] // TILE            # the blocks that go through tile_store (the tail block does not)
    above = sorted(p for p in _PERIODS.values() if p > 1)
    assert above == [2, 3, 7] and blocks == 37 and all(3 * p <= blocks for p in above)
    for p in above:
        assert {rb % p for rb in range(blocks)} == set(range(p))


@pytest.mark.parametrize("store", sorted(_STORES))
def test_store_policy_and_mix_period_vs_oracle(ref, store):
    """"dense" (302 rows, 37 full row blocks of a sweep wave) at d = 12, to cap 50 and to the end: every store nontemporal; the mixed
    form with LPX_UPDATE_MIXMOD = 2, 3, 7, 8 and 19, which reach the compact sweep as periods 1, 1, 2, 3 and 7 (asserted from the
    source's constants); and the default policy, which the compact form refuses (the full path then, asked of the handle) -- the
    oracle's bits each time."""
    env, compact, n = _STORES[store]
    R = _matrix_lp("dense")[0].shape[0]
    assert R >= 120
    if n is not None:
        assert _period(n) == _PERIODS[n] and (_period(n) == 1 or len({rb % _period(n) for rb in range(R // TILE)}) >= 2)
    plan, want = _open("dense"), []
    for cap in (50, FULL):
        plan += [["restore"], _run(cap)]
        want.append(ref("dense", cap))
    assert want[0][1] == 50 and want[1][1] > 8 * 12
    _check(_child(plan, dict(env, LPX_PIVOT_COMPACT="1", LPX_PIVOT_DEFER="12")), want, store, compact=compact)


# ---------------------------------------------------------------------------------------------------------------------------
# D. row edges of the _cm launches
# ---------------------------------------------------------------------------------------------------------------------------
_ROW_CASES = [(name, 12, 0) for name in sorted(CR.ROW_EDGES)] + [("rows257", 3, 0), ("rows64", 12, 80)]


@pytest.mark.parametrize("name,d,rcap", _ROW_CASES)
def test_row_edges_vs_oracle(ref, name, d, rcap):
    """R = 64, 65, 72 (two full blocks of a strip wave, one row into the next strip, the second block empty), 256 and 257 (one full
    workgroup of the column launch, one row into the second) in handles of as many rows, and R = 64 in a handle of 80 rows (the live
    rows end on a strip edge inside the capacity): to CR.ROW_EDGE_CAP (pivots pending after at least one sweep) and to the end."""
    (m, n, seed), pivots, (mod, res) = CR.ROW_EDGES[name]
    R, C = CR.lp(name)[0].shape
    assert (R, C) == (m + 1, m + n + 1) and R % mod == res
    _, sweeps, pending, _ = CR.ended(name, d, CR.ROW_EDGE_CAP)
    assert sweeps >= 1 and pending > 0
    plan = [["alloc", rcap, MIN_BYTES // (8 * rcap) + 32], ["shape", name]] if rcap else _big(name)
    assert plan[0][1] == (rcap or R) and _bytes(plan[0]) > MIN_BYTES and (not rcap or (rcap > R and R % 16 == 0))
    want = []
    for cap in (CR.ROW_EDGE_CAP, FULL):
        plan += [["restore"], _run(cap)]
        want.append(ref(name, cap))
    assert [w[1] for w in want] == [CR.ROW_EDGE_CAP, pivots] and want[1][0] == CR.OPTIMAL
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER=str(d))), want, (name, d, rcap))


# ---------------------------------------------------------------------------------------------------------------------------
# E. what runs next on the handle
# ---------------------------------------------------------------------------------------------------------------------------
_DUALS = ("dual:60:60:1:5", "dual:60:60:1:10")      # test_gpu_dual._dual_tableau at CR.MAIN's shape: 59 and 50 dual pivots
_DUAL_OPTS = {"fdf_guard": 0, "cleanup": 1}


@pytest.mark.parametrize("graph", ["1", "0"])
def test_full_path_and_dual_runs_after_a_compact_run(ref, oracle, monkeypatch, graph):
    """One handle, d = 3, the budget rule deciding the form (asked of the handle: [1, 0, 1, 1]).  CR.MAIN to cap 30 in the compact form;
    10 more pivots on the full path, from the compact run's result and with the compact tableau still in the second buffer; on to
    the end, compact again; restored and run to the end.  Then, twice: a dual tableau of the same shape uploaded and run by
    lpx_dual_run (a group of one, out of place into the second buffer: after an odd number of pivots the handle's buffers trade
    places, after an even number they do not -- both, asserted through the handle's device pointer), CR.MAIN uploaded again and
    run to the end in the compact form."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    trace = CR.oracle_trace(oracle, CR.MAIN)
    assert len(trace) == 66 and 30 >= K["COMPACT_MIN_SWEEPS"] * 3 > 10
    part = lambda a, b: _h(np.array(trace[a:b], np.int32).reshape(-1, 2), np.int32)
    whole, at40 = ref(CR.MAIN, FULL), ref(CR.MAIN, 40)
    assert at40[:2] == [CR.ITER_LIMIT, 40] and whole[:2] == [CR.OPTIMAL, 66]
    plan = _big(CR.MAIN) + [_run(30), _run(10), _run(FULL), ["restore"], _run(FULL)]
    want = [ref(CR.MAIN, 30), [CR.ITER_LIMIT, 10, part(30, 40)] + at40[3:], [CR.OPTIMAL, 26, part(40, 66)] + whole[3:], whole]
    forms, parities = [1, 0, 1, 1], []
    for name in _DUALS:
        T, basis = _dual_tableau(*[int(v) for v in name.split(":")[1:]])
        assert T.shape == CR.lp(CR.MAIN)[0].shape
        st, tr, _ = oracle.dual_tableau(T, basis, **_DUAL_OPTS)
        assert int(st) == CR.OPTIMAL
        parities.append(len(tr) % 2)
        plan += [["upload", name], ["dual", _DUAL_OPTS], ["upload", CR.MAIN], _run(FULL)]
        want += [[int(st), len(tr), _h(tr, np.int32), _h(basis, np.int32), _h(T, np.float64)], whole]
        forms += [len(tr) % 2, 1]                                # a dual record ends with "the buffers traded places"
    assert sorted(parities) == [0, 1] and [w[1] for w in want[4::2]] == [59, 50]
    env = {"LPX_UPDATE_POLICY": "2", "LPX_PIVOT_DEFER": "3"}
    _check(_child(plan, dict(env, LPX_GRAPH="0") if graph == "0" else env), want, graph, compact=forms)


# ---------------------------------------------------------------------------------------------------------------------------
# F. the defaults, with no switch set
# ---------------------------------------------------------------------------------------------------------------------------
_DEFAULTS = {"cached": (100 << 20, 0, 12), "large": (200 << 20, 1, 12), "streamed": (320 << 20, 1, 16)}


@pytest.mark.parametrize("tier", sorted(_DEFAULTS))
def test_default_selection_vs_oracle(ref, monkeypatch, tier):
    """CR.TALL in handles of 601 rows and about 100 MB, 200 MB and 320 MiB with no switch in the environment: the first, between 64
    MB and FUSED_CACHED_BYTES, keeps the default store policy and so the full path; the second runs the compact form at d = 12; the
    third, above UPD_STREAM_BYTES, at d = 16.  The depth is read off a profile run (its update_launches are its sweep launches:
    the run ends inside the first batch of 64 launches, where the count takes in every launch up to the last) and compared with the
    model's sweep count at that depth; the counts at 12 and 16 differ.  A budget of 60 pivots on the third handle is below 8 sweeps
    of 16: the full path."""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    size, compact, d = _DEFAULTS[tier]
    R, C = CR.lp(CR.TALL)[0].shape
    assert (R, C) == (601, 641)
    alloc = ["alloc", R, size // (8 * R) + 32]
    lo, hi = {"cached": (MIN_BYTES, K["FUSED_CACHED_BYTES"]), "large": (K["FUSED_CACHED_BYTES"], K["UPD_STREAM_BYTES"]),
              "streamed": (K["UPD_STREAM_BYTES"], 1 << 40)}[tier]
    assert lo < _bytes(alloc) <= hi and d == (K["DEPTH_STREAM"] if tier == "streamed" else K["DEPTH_LARGE"])
    want = ref(CR.TALL, FULL)
    pivots, sweeps, _, _ = CR.ended(CR.TALL, d)
    other = CR.ended(CR.TALL, 28 - d)[1]
    assert pivots == want[1] < 60 and sweeps != other and FULL >= K["COMPACT_MIN_SWEEPS"] * d > 60
    plan = [alloc, ["shape", CR.TALL], _run(FULL), ["restore"], _run(FULL, profile=1), ["restore"], _run(60)]
    got = _child(plan, {})
    _check(got, [want] * 3, tier, compact=[compact, compact, 0])
    if compact:
        assert got[1][1] < 64                                   # inside the first batch of launches (the default batch)
        assert got[1][3] == sweeps and got[1][3] != other, (tier, got[1][3], sweeps, other)
