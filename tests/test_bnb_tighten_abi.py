"""CPU checks of the entry points of reduced-cost bound tightening (lpx_bounded_node5, lpx_node_batch_run3,
lpx_solve_bnb_bounded10): exported and declared, mirrored in ctypes, C# and the command-line tool, struct sizes, argument errors
before device errors with their messages, the Python-level errors, the help and the refusals of the command-line tool, and no
CPU fallback."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_bounded_node5", "lpx_node_batch_run3", "lpx_solve_bnb_bounded10")
NINF = -np.inf


def _problem(lpx):
    c = np.array([3.0, 5.0, 2.0]); A = np.array([[1.0, 2.0, 2.0], [2.0, 4.0, 3.0]]); b = np.array([10.0, 15.0])
    rel = np.array([0, 0], dtype=np.int32)
    p = lpx._lib.Problem(0, 3, 2, c.ctypes.data_as(lpx._lib.dp), A.ctypes.data_as(lpx._lib.dp),
                         rel.ctypes.data_as(lpx._lib.ip), b.ctypes.data_as(lpx._lib.dp))
    return p, (c, A, b, rel)


def _fix(lpx, cap, hold):
    a = (np.zeros(max(cap, 1), dtype=np.int32), np.zeros(max(cap, 1)), np.zeros(max(cap, 1)))
    hold.append(a)
    return lpx._lib.FixList(cap, 7, a[0].ctypes.data_as(lpx._lib.ip), a[1].ctypes.data_as(lpx._lib.dp), a[2].ctypes.data_as(lpx._lib.dp))


def test_symbols_exported_declared_and_mirrored(lpx):
    L = lpx._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s          # a ctypes signature in _lib.py
        assert re.search(r"\b%s\(" % s, hdr), s
        assert (" %s(" % s) in native, s
    for cs, c in (("LpxFixList", "lpx_fix_list"), ("LpxBnbFixInfo", "lpx_bnb_fix_info")):
        assert "struct " + cs in native and "} %s;" % c in hdr
    assert L.lpx_abi_version() == 1
    assert C.sizeof(lpx._lib.FixList) == 32 and C.sizeof(lpx._lib.BnbFixInfo) == 24
    assert C.sizeof(lpx._lib.NodeRecord) == 64 and C.sizeof(lpx._lib.GuardRecord) == 8        # untouched
    assert len(L.lpx_bounded_node5.argtypes) == 17 and len(L.lpx_node_batch_run3.argtypes) == 19
    assert len(L.lpx_solve_bnb_bounded10.argtypes) == 18
    assert len(L.lpx_bounded_node4.argtypes) == 15 and len(L.lpx_node_batch_run2.argtypes) == 17        # the entries they extend
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "--tighten" in cli and "lpx_solve_bnb_bounded10(" in cli
    bench = open(os.path.join(ROOT, "tools", "bench_bnb_bounded.py")).read()
    assert "--compare-tighten" in bench and "tighten" in bench
    assert inspect.signature(lpx.DeviceTableau.bounded_node).parameters["fix_bound"].default is None
    assert inspect.signature(lpx.NodeBatch.run).parameters["fix_bounds"].default is None
    assert inspect.signature(lpx.LPSolver.SolveBnbBounded).parameters["tighten"].default is False


def test_cli_help_and_refusals(lpx):
    exe = os.path.join(os.path.dirname(lpx.__file__), "lpx_cli")

    def run(*args):
        return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)

    out = run("--help")
    assert out.returncode == 0 and "--tighten" in out.stdout and "lpx_solve_bnb_bounded10" in out.stdout
    r = run("--tighten", "x.txt")
    assert r.returncode == 64 and "--tighten needs --bnb-bounded --divers" in r.stderr
    r = run("--binary", "--bnb-bounded", "--tighten", "x.txt")
    assert r.returncode == 64 and "--tighten needs --bnb-bounded --divers" in r.stderr
    base = ("--binary", "--bnb-bounded", "--divers", "2", "--tighten")
    r = run(*base, "--plunge", "4", "x.txt")
    assert r.returncode == 64 and "have no tightening" in r.stderr
    r = run(*base, "--branching", "strong", "x.txt")
    assert r.returncode == 64 and "have no tightening" in r.stderr
    r = run(*base, "--stall-events", "50", "--root-cuts", "2", "no_such_file.txt")      # accepted: it gets as far as the input file
    assert r.returncode == 66


def test_node5_argument_errors_come_first(lpx):
    """Checked before any device is looked for: the same answers with and without a GPU.  No handle can be made without a
    device, so the checks that need none come in front of the null handle."""
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    rec, g = lpx._lib.NodeRecord(), lpx._lib.GuardRecord(7, 7)
    hold = []
    fx = _fix(lpx, 4, hold)
    nan = float("nan")

    def node5(flags=1, cutoff=0.0, S=0, fb=NINF, nint=0, form=1, out=C.byref(rec), guard=C.byref(g), fix=C.byref(fx)):
        return L.lpx_bounded_node5(None, 0, None, None, None, None, flags, cutoff, S, fb, nint, None, 1e-6, form, out, guard, fix)

    def err():
        return lpx._lib.last_error()

    for flags in (8, 16, -1):                                 # bit 8 is no flag: the bound is an argument
        assert node5(flags=flags) == EINVAL and "lpx_bounded_node5: unknown flag" in err()
    assert node5(flags=1 | 4, cutoff=nan) == EINVAL and "lpx_bounded_node5: cutoff is NaN" in err()
    for form in (-1, 3):
        assert node5(form=form) == EINVAL and "lpx_bounded_node5: unknown form" in err()
    for S in (-1, -50):
        assert node5(S=S, fb=1.0) == EINVAL and "lpx_bounded_node5: stall_events is negative" in err()
    for form in (0, 1, 2):
        assert node5(fb=nan, form=form) == EINVAL and "lpx_bounded_node5: fix_bound is NaN" in err()
    for fb in (NINF, 0.0, 12.5):                              # the capacity is checked whatever the bound
        assert node5(fb=fb, nint=5) == EINVAL and "lpx_bounded_node5: fix->cap is below nint" in err()
    assert node5(fb=0.0, fix=None) == EINVAL and "lpx_bounded_node5: null fix" in err()
    assert node5(S=1, form=0) == EINVAL and "lpx_bounded_node5: the stall guard has no launches form" in err()
    for fb in (0.0, -1e300, np.inf):
        assert node5(fb=fb, form=0) == EINVAL and "lpx_bounded_node5: reduced-cost tightening has no launches form" in err()
    # with -inf every form goes on to the checks of lpx_bounded_node4, and so do the on-chip forms with a bound; fix may be NULL then
    for fb, form, fix in ((NINF, 0, None), (NINF, 1, None), (NINF, 2, C.byref(fx)), (3.0, 1, C.byref(fx)), (3.0, 2, C.byref(fx))):
        assert node5(fb=fb, form=form, fix=fix) == EINVAL and "lpx_bounded_node5: null handle" in err(), (fb, form)
    assert (g.bland_events, g.first_bland) == (0, -1) and fx.n == 0     # reset where the call gets that far
    # the entry it is built on keeps its own name
    assert L.lpx_bounded_node4(None, 0, None, None, None, None, 1, 0.0, 0, 0, None, 1e-6, 1, C.byref(rec), None) == EINVAL
    assert "lpx_bounded_node4: null handle" in err()


def test_run3_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL, ip, dp = lpx._lib.EINVAL, lpx._lib.ip, lpx._lib.dp
    slot = np.zeros(2, dtype=np.int32); K = np.zeros(2, dtype=np.int32); rc = np.zeros(2, dtype=np.int32)
    recs = (lpx._lib.NodeRecord * 2)()
    guards = (lpx._lib.GuardRecord * 2)()
    hold = []
    fixes = (lpx._lib.FixList * 2)(_fix(lpx, 4, hold), _fix(lpx, 4, hold))
    cut = np.array([0.0, float("nan")])
    fb = np.array([NINF, 2.0]); fbnan = np.array([1.0, float("nan")]); fboff = np.array([NINF, NINF])
    sp, kp, rp, cp = slot.ctypes.data_as(ip), K.ctypes.data_as(ip), rc.ctypes.data_as(ip), cut.ctypes.data_as(dp)

    def run(batch=None, B=1, slot=sp, K=kp, flags=1, cutoff=None, S=0, fb=fb, nint=0, out=recs, guard=guards, fix=fixes, rc=rp):
        return L.lpx_node_batch_run3(batch, B, slot, K, None, None, None, None, flags, cutoff, S, None if fb is None else fb.ctypes.data_as(dp),
                                     nint, None, 1e-6, out, guard, fix, rc)

    def err():
        return lpx._lib.last_error()

    for S in (0, 50):
        assert run(S=S) == EINVAL and "lpx_node_batch_run3: null batch" in err()
        assert run(S=S, guard=None) == EINVAL and "lpx_node_batch_run3: null batch" in err()      # guard may be NULL
    assert run(fb=fboff, fix=None) == EINVAL and "lpx_node_batch_run3: null batch" in err()       # fix may be NULL when all are -inf
    for name in ("out", "rc", "K", "slot"):
        assert run(**{name: None}) == EINVAL and "lpx_node_batch_run3: null " + name in err(), name
    assert run(S=-1) == EINVAL and "lpx_node_batch_run3: stall_events is negative" in err()
    for B in (0, -1):
        assert run(B=B) == EINVAL and "lpx_node_batch_run3: B is outside [1, W]" in err()
    for flags in (8, 16, -1):
        assert run(flags=flags) == EINVAL and "lpx_node_batch_run3: unknown flag" in err()
    assert run(B=2, flags=1 | 4, cutoff=cp) == EINVAL and "lpx_node_batch_run3: entry 1: cutoff is NaN" in err()
    assert run(fb=None) == EINVAL and "lpx_node_batch_run3: null fix_bound" in err()
    assert run(B=2, fb=fbnan) == EINVAL and "lpx_node_batch_run3: entry 1: fix_bound is NaN" in err()
    assert run(B=2, nint=5) == EINVAL and "lpx_node_batch_run3: entry 0: fix->cap is below nint" in err()
    assert run(B=2, fix=None) == EINVAL and "lpx_node_batch_run3: entry 1: null fix" in err()
    assert L.lpx_node_batch_run2(None, 1, sp, kp, None, None, None, None, 1, None, 0, 0, None, 1e-6, recs, guards, rp) == EINVAL
    assert "lpx_node_batch_run2: null batch" in err()


def test_python_level_errors(lpx):
    nb = object.__new__(lpx.NodeBatch)          # no handles are needed to reach the checks
    nb._handles, nb._W, nb._h = [], 2, None
    with pytest.raises(ValueError, match="NaN"):
        nb.run([0], [([], [], [])], 4, fix_bounds=[float("nan")])
    with pytest.raises(ValueError, match=r"B must be in \[1, W\]"):
        nb.run([0, 1, 2], [([], [], [])] * 3, 4, fix_bounds=0.0)
    dt = object.__new__(lpx.DeviceTableau)
    dt._h = None
    with pytest.raises(ValueError, match="fix_bound is NaN"):
        dt.bounded_node([], [], [], 4, fix_bound=float("nan"))
    with pytest.raises(ValueError, match="no launches form"):
        dt.bounded_node([], [], [], 4, fix_bound=1.0, form="launches")
    with pytest.raises(ValueError, match="stall_events must not be negative"):
        dt.bounded_node([], [], [], 4, fix_bound=1.0, stall_events=-1)
    with pytest.raises(ValueError, match="unknown node form"):
        dt.bounded_node([], [], [], 4, fix_bound=1.0, form="resident")
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    S = lpx.LPSolver()
    with pytest.raises(ValueError, match="launches"):
        S.SolveBnbBounded(prob, [4, 3, 3], tighten=True, node_form="launches")
    with pytest.raises(ValueError, match="plunge"):
        S.SolveBnbBounded(prob, [4, 3, 3], tighten=True, plunge=4)
    for rule in ("strong", "most_fractional"):
        with pytest.raises(ValueError, match="branching"):
            S.SolveBnbBounded(prob, [4, 3, 3], tighten=True, branching=rule)
    with pytest.raises(lpx.SolverException) as e:
        S.SolveBnbBounded(prob, [4, 3, 3], tighten=True, divers=0)
    assert e.value.code == lpx._lib.EINVAL and "lpx_solve_bnb_bounded10: divers is outside" in str(e.value)


def test_driver_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r, info, dinfo, ginfo = lpx._lib.Result(), lpx._lib.BnbBoundedInfo(), lpx._lib.BnbDiversInfo(), lpx._lib.BnbGuardInfo()
    cinfo, finfo = lpx._lib.BnbCutInfo(), lpx._lib.BnbFixInfo(5, 5, 5)
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)

    def solve(max_nodes=0, flags=0, divers=2, S=0, root_form=0, tighten=1, out=C.byref(r)):
        return L.lpx_solve_bnb_bounded10(C.byref(p), None, upp, None, None, max_nodes, flags, divers, S, root_form, None, tighten, out,
                                         C.byref(info), C.byref(dinfo), C.byref(ginfo), C.byref(cinfo), C.byref(finfo))

    def err():
        return lpx._lib.last_error()

    for W in (0, 1025, -3):
        assert solve(divers=W) == EINVAL and "lpx_solve_bnb_bounded10: divers is outside [1, 1024]" in err()
    assert solve(S=-1) == EINVAL and "lpx_solve_bnb_bounded10: stall_events is negative" in err()
    for form in (-1, 3):
        assert solve(root_form=form) == EINVAL and "lpx_solve_bnb_bounded10: unknown root_form" in err()
    for t in (-1, 2, 7):
        assert solve(tighten=t) == EINVAL and "lpx_solve_bnb_bounded10: tighten is neither 0 nor 1" in err()
    for t in (0, 1):
        for flags in (1, 8, 2 | 16):
            assert solve(flags=flags, tighten=t) == EINVAL and "search_flags" in err()
        assert solve(max_nodes=-1, tighten=t) == EINVAL and "max_nodes is negative" in err()
    assert solve(out=None) == EINVAL and "lpx_solve_bnb_bounded10: null argument" in err()
    frac = np.array([4.0, 2.5, 3.0])
    rc = L.lpx_solve_bnb_bounded10(C.byref(p), None, frac.ctypes.data_as(lpx._lib.dp), None, None, 0, 0, 2, 0, 0, None, 1, C.byref(r),
                                   None, None, None, None, C.byref(finfo))
    assert rc == EINVAL and "needs finite, integral lower and upper bounds" in err()
    assert (finfo.tightened_nodes, finfo.tightened_cols, finfo.max_per_node) == (0, 0, 0)       # zeroed where the call gets that far


@pytest.mark.parametrize("tighten", [0, 1])
def test_no_cpu_fallback(lpx, tighten):
    """Without a device the driver is LPX_EDEVICE; with one it solves."""
    L = lpx._lib.lib()
    p, hold = _problem(lpx)
    r, info, dinfo, ginfo = lpx._lib.Result(), lpx._lib.BnbBoundedInfo(), lpx._lib.BnbDiversInfo(), lpx._lib.BnbGuardInfo()
    finfo = lpx._lib.BnbFixInfo()
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)
    rc = L.lpx_solve_bnb_bounded10(C.byref(p), None, upp, None, None, 0, 0, 2, 0, 0, None, tighten, C.byref(r), C.byref(info),
                                   C.byref(dinfo), C.byref(ginfo), None, C.byref(finfo))
    if L.lpx_device_count() > 0:
        assert rc == 0 and info.nodes >= 1 and dinfo.rounds >= 1 and finfo.max_per_node >= 0
        L.lpx_bnb_bounded_info_free(C.byref(info)); L.lpx_bnb_divers_info_free(C.byref(dinfo))
        L.lpx_result_free(C.byref(r))
    else:
        assert rc == lpx._lib.EDEVICE and "no HIP device" in lpx._lib.last_error()
