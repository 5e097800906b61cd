"""The compact form of the primal loop (run_fused sweeping a tableau without its basic columns) pinned to the CPU
oracle: status, pivot count, trace, basis and the SHA-256 of the whole float64 tableau.  No tolerances.  Which form a run took is
asked of the handle (lpx_tableau_last_run_compact) and asserted for every run.

The environment switches are read once per process, hence one child process per setting, with the resident kernels off.  The
children run with LPX_UPDATE_POLICY=2, so that small tableaux take the strip sweeps, on handles above SELP_MIN_MB (the LP's own,
or a larger one the LP moves into through lpx_tableau_set_shape), and with LPX_PIVOT_COMPACT=1 unless a case says otherwise: the
budget threshold is a matter of speed, not of results.

The LPs and seeds are those of tests/test_compact_ref.py, which holds the scheme restated in NumPy and asserts, with the oracle,
that each trace holds the situation it is there for; the cases here assert the same before they run."""
import functools
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import test_compact_ref as CR
from test_gpu_deferred_matrix import FULL, _h, _same
from test_gpu_select_only import _lp, _open

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
STREAMING = {"LPX_UPDATE_POLICY": "2", "LPX_PIVOT_COMPACT": "1"}

# One child runs a list of steps on one handle and prints one record per "run" step (the steps of test_gpu_deferred_matrix.py's
# child; an LP is one of test_compact_ref.LPS or of the neighbouring files).  A record ends with the form the run took.  Two more
# steps serve tests/test_gpu_compact_edges.py:
#   ["upload", lp]               a tableau of the handle's live shape over what the last run left (no set_shape), its start kept
#   ["dual", opts]               dual_run(resident=-1, **opts); the record ends with whether the handle's buffers traded places
_CHILD = """
    import hashlib, json, sys, ctypes, numpy as np
    sys.path.insert(0, %r)
    import linear_programming_solver_lpr381_amd as L
    import test_compact_ref as CR
    from test_gpu_select_only import _lp
    lib = L._lib.lib()
    lib.lpx_tableau_last_run_compact.argtypes = [ctypes.c_void_p]
    lib.lpx_tableau_last_run_compact.restype = ctypes.c_int
    h = lambda a, dt: hashlib.sha256(np.ascontiguousarray(a, dtype=dt).view(np.uint8)).hexdigest()
    def get(name):
        if name.startswith("dual:"):                # "dual:m:n:seed:n_ge": test_gpu_dual._dual_tableau
            from test_gpu_dual import _dual_tableau
            return _dual_tableau(*[int(v) for v in name.split(":")[1:]])
        return CR.lp(name) if name in CR.LPS else _lp(name)
    out, dt = [], None
    for step in json.loads(sys.argv[1]):
        op = step[0]
        if op == "open":
            if dt is not None: dt.close()
            dt = L.DeviceTableau.from_host(*get(step[1]))
            dt.snapshot()
        elif op == "alloc":
            if dt is not None: dt.close()
            dt = L.DeviceTableau(step[1], step[2])
        elif op == "shape":
            T, basis = get(step[1])
            L._lib.check(lib.lpx_tableau_set_shape(dt._h, T.shape[0], T.shape[1]))
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
                        h(tr, np.int32), h(bg, np.int32), h(Tg, np.float64), int(lib.lpx_tableau_last_run_compact(dt._h))])
        elif op == "upload":                        # a tableau of the handle's live shape over whatever the last run left
            dt.upload(*get(step[1]))
            dt.snapshot()
        elif op == "dual":                          # dual_run; the record ends with: has the handle's tableau changed buffers
            at = dt.device_ptr()[0]
            status, st = dt.dual_run(L.default_opts(True, resident=-1, **step[1]))
            Tg, bg = dt.download()
            tr = dt.trace()
            out.append([int(status), int(st["pivots"]), int(st["launches"]), int(st["update_launches"]),
                        h(tr, np.int32), h(bg, np.int32), h(Tg, np.float64), int(dt.device_ptr()[0] != at)])
    dt.close()
    print(json.dumps(out))
""" % TESTS


def _child(plan, env, timeout=300):
    e = dict(os.environ, PYTHONPATH=ROOT, LPX_RESIDENT="0", **env)
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(_CHILD), json.dumps(plan)], env=e, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def _run(cap, **opts):
    return ["run", cap, opts]


def _get(name):
    return CR.lp(name) if name in CR.LPS else _lp(name)


def _big(name, taller=False):
    """Plan steps that put the LP on a handle above SELP_MIN_MB (test_gpu_select_only._open, for the LPs of both files)."""
    if name not in CR.LPS:
        return _open(name, taller)
    R, C = CR.lp(name)[0].shape
    if taller:                                                   # four times the rows as well (the pair's row cap bounds the height)
        return [["alloc", 4 * R, (64 << 20) // (8 * 4 * R) + 32], ["shape", name]]
    return [["alloc", R, (64 << 20) // (8 * R) + 32], ["shape", name]]


@pytest.fixture(scope="module")
def ref(oracle):
    @functools.lru_cache(maxsize=None)
    def get(name, cap):
        T, basis = _get(name)
        st, tr = oracle.primal_tableau(T, basis, max_iter=cap)
        return [int(st), len(tr), _h(tr, np.int32), _h(basis, np.int32), _h(T, np.float64)]
    return get


def _check(got, want, what, compact=1):
    assert len(got) == len(want)
    bad = [(i, g[:2], w[:2]) for i, (g, w) in enumerate(zip(got, want)) if not _same(g, w)]
    assert not bad, (what, bad)
    forms = [g[7] for g in got]
    assert forms == ([compact] * len(got) if isinstance(compact, int) else compact), (what, forms)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the cases of tests/test_compact_ref.py: depths, endings, re-entries, reversed ties, the tall LP
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 4, 8, 12, 16])
def test_endings_and_reentries_vs_oracle(ref, oracle, d):
    """CR.MAIN at depth d to the caps of CR.ending_caps: 0, 1 and d - 1 pivots pending, the newest pending pivot chosen at a sweep
    step, and to the end; its trace holds re-entries inside the window before and across a sweep (asserted)."""
    tr = CR.oracle_trace(oracle, CR.MAIN)
    kinds = CR.reentry_kinds(tr, CR.lp(CR.MAIN)[1], d)
    assert {"before", "across"} <= kinds, kinds
    caps = CR.ending_caps(d, len(tr))
    plan, want = _big(CR.MAIN), []
    for cap in caps + [FULL]:
        plan += [["restore"], _run(cap)]
        want.append(ref(CR.MAIN, cap))
    assert [w[1] for w in want[:-1]] == caps
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER=str(d))), want, d)


@pytest.mark.parametrize("d", [3, 4, 8, 16])
def test_reversed_ties_vs_oracle(ref, oracle, d):
    """CR.TIES: duplicated columns whose reduced costs tie on bits while the slot order of the two variables is the reverse of
    their variable order, one of them having reached its slot by way of a leaving variable (asserted on the oracle's trace)."""
    assert CR.reversed_tie_steps(oracle, CR.TIES), "no tie between slots in reversed order"
    plan = _big(CR.TIES) + [_run(FULL)]
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER=str(d))), [ref(CR.TIES, FULL)], d)


def test_tall_lp_vs_oracle(ref):
    """600 rows, 40 columns: 41 slots, one column window, a handful of lanes per select workgroup.  d = 12."""
    T, _ = CR.lp(CR.TALL)
    assert T.shape == (601, 641)
    plan, want = _big(CR.TALL), []
    for cap in (25, FULL):
        plan += [["restore"], _run(cap)]
        want.append(ref(CR.TALL, cap))
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER="12")), want, "tall")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. compact column edges: the slots end on a full 128-column window, on 8 live lanes, inside the first window
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge256", "edge272", "edge100"])
def test_compact_column_edges_vs_oracle(ref, oracle, name):
    """n + 1 = 256, 260 and 100 slots (compact ld 256, 272, 112) on 41, 21 and 51 rows.  The oracle's trace puts the entering slot on the
    first and on the last lane of a window and next to the RHS slot (asserted, by the model's slot bookkeeping).  d = 12, to cap
    25 (two sweeps, one pivot pending) and to the end."""
    T, basis = CR.lp(name)
    slots = T.shape[1] - T.shape[0] + 1
    assert (slots + 15) // 16 * 16 == {"edge256": 256, "edge272": 272, "edge100": 112}[name]
    seen = CR.entering_slots(oracle, name)
    want_slots = {0, slots - 2} | ({127, 128} if slots > 129 else set())
    assert want_slots <= seen, want_slots - seen
    plan, want = _big(name), []
    for cap in (25, FULL):
        plan += [["restore"], _run(cap)]
        want.append(ref(name, cap))
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER="12")), want, name)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. capacity and live shape
# ---------------------------------------------------------------------------------------------------------------------------
def test_capacity_other_than_live_shape(ref):
    """CR.MAIN in a wider handle, in a taller and wider one, and in a handle that held a larger LP ("dense", 302 x 589, run to its end in
    the compact form) before.  d = 16."""
    R, C = CR.lp(CR.MAIN)[0].shape
    want = ref(CR.MAIN, FULL)
    plan = _big(CR.MAIN) + [_run(FULL)] + _big(CR.MAIN, taller=True) + [_run(FULL)]
    plan += [["alloc", 400, (64 << 20) // (8 * 400) + 32], ["shape", "dense"], _run(FULL), ["shape", CR.MAIN], _run(FULL)]
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER="16")), [want, want, ref("dense", FULL), want], "capacity")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. how runs end
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 16])
def test_unbounded_optimal_and_resumed(ref, d):
    """"late-unbounded" ends UNBOUNDED after 500 pivots with pivots pending (the column launch had zeroed the slot of a pivot that
    is not taken: the exit pass puts it back); "dense" ends OPTIMAL; "dense" to cap 2d + 3 and then resumed on the same handle
    with no cap (the second run compacts the basis the first one left)."""
    wu, wo = ref("late-unbounded", FULL), ref("dense", FULL)
    assert wu[0] == CR.UNBOUNDED and wu[1] % d != 0 and wo[0] == 0
    plan = _open("late-unbounded") + [_run(FULL)] + _open("dense") + [_run(FULL), ["restore"], _run(2 * d + 3), _run(FULL)]
    got = _child(plan, dict(STREAMING, LPX_PIVOT_DEFER=str(d)))
    _check(got[:3], [wu, wo, ref("dense", 2 * d + 3)], d)
    # the resumed run: the trace restarts, the tableau and the basis are those of the whole solve
    assert got[3][0] == 0 and got[3][1] == wo[1] - (2 * d + 3) and got[3][5:7] == wo[3:5] and got[3][7] == 1


def test_graph_against_eager(ref):
    """The captured graph and LPX_GRAPH=0 give the oracle's bits alike (d = 12, "dense" to cap 50 and to the end)."""
    plan, want = _open("dense"), []
    for cap in (50, FULL):
        plan += [["restore"], _run(cap)]
        want.append(ref("dense", cap))
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER="12")), want, "graph")
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER="12", LPX_GRAPH="0")), want, "eager")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. fallbacks and the switch
# ---------------------------------------------------------------------------------------------------------------------------
def test_entry_check_falls_back_to_the_full_path(ref):
    """A -0.0 in a basic column, a 1.0 + ulp on its diagonal, and a basis entry naming a non-unit column: each takes the full
    path (asserted through the handle) and still matches the oracle on the same input."""
    plan, want = [], []
    for name in ("bad-negzero", "bad-ulp", "bad-basis"):
        plan += _big(name) + [_run(FULL)]
        want.append(ref(name, FULL))
    _check(_child(plan, dict(STREAMING, LPX_PIVOT_DEFER="12")), want, "fallback", compact=0)


def test_switch_off_same_bits(ref):
    """LPX_PIVOT_COMPACT=0 against the default (the budget rule: a long run compacts, a run of 25 pivots does not): same bits."""
    plan, want = _open("dense"), []
    for cap in (25, FULL):
        plan += [["restore"], _run(cap)]
        want.append(ref("dense", cap))
    env = {"LPX_UPDATE_POLICY": "2", "LPX_PIVOT_DEFER": "12"}
    _check(_child(plan, dict(env, LPX_PIVOT_COMPACT="0")), want, "off", compact=0)
    _check(_child(plan, env), want, "default", compact=[0, 1])
