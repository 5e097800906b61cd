"""CPU checks of the entry points of the stall guard (lpx_bounded_node4, lpx_node_batch_run2, lpx_solve_bnb_bounded7): exported and
declared, mirrored in ctypes, C# and the command-line tool, struct sizes, argument errors before device errors with their
messages, the Python-level errors, the help and the refusals of the command-line tool, and no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_bounded_node4", "lpx_node_batch_run2", "lpx_solve_bnb_bounded7")


def _problem(lpx):
    c = np.array([3.0, 5.0, 2.0]); A = np.array([[1.0, 2.0, 2.0], [2.0, 4.0, 3.0]]); b = np.array([10.0, 15.0])
    rel = np.array([0, 0], dtype=np.int32)
    p = lpx._lib.Problem(0, 3, 2, c.ctypes.data_as(lpx._lib.dp), A.ctypes.data_as(lpx._lib.dp),
                         rel.ctypes.data_as(lpx._lib.ip), b.ctypes.data_as(lpx._lib.dp))
    return p, (c, A, b, rel)


def test_symbols_exported_declared_and_mirrored(lpx):
    L = lpx._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s          # a ctypes signature in _lib.py
        assert re.search(r"\b%s\(" % s, hdr), s
        assert (" %s(" % s) in native, s
    for cs, c in (("LpxGuardRecord", "lpx_guard_record"), ("LpxBnbGuardInfo", "lpx_bnb_guard_info")):
        assert "struct " + cs in native and "} %s;" % c in hdr
    assert L.lpx_abi_version() == 1
    assert C.sizeof(lpx._lib.GuardRecord) == 8 and C.sizeof(lpx._lib.BnbGuardInfo) == 24
    assert C.sizeof(lpx._lib.NodeRecord) == 64                 # untouched
    assert len(L.lpx_bounded_node4.argtypes) == 15 and len(L.lpx_node_batch_run2.argtypes) == 17
    assert len(L.lpx_solve_bnb_bounded7.argtypes) == 13
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "--stall-events" in cli and "lpx_solve_bnb_bounded7(" in cli
    bench = open(os.path.join(ROOT, "tools", "bench_bnb_bounded.py")).read()
    assert "--compare-guard" in bench and "stall_events" in bench
    import inspect
    for f in (lpx.DeviceTableau.bounded_node, lpx.NodeBatch.run, lpx.LPSolver.SolveBnbBounded):
        assert inspect.signature(f).parameters["stall_events"].default is None, f


def test_cli_help_and_refusals(lpx):
    exe = os.path.join(os.path.dirname(lpx.__file__), "lpx_cli")

    def run(*args):
        return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)

    out = run("--help")
    assert out.returncode == 0 and "--stall-events S" in out.stdout and "lpx_solve_bnb_bounded7" in out.stdout
    base = ("--binary", "--bnb-bounded", "--stall-events")
    for bad in ("-1", "x", "5x"):
        r = run(*base, bad, "x.txt")
        assert r.returncode == 64 and "--stall-events takes a non-negative pivot count" in r.stderr, bad
    r = run("--stall-events", "50", "x.txt")
    assert r.returncode == 64 and "--stall-events needs --bnb-bounded" in r.stderr
    r = run(*base, "50", "--node-form", "launches", "x.txt")
    assert r.returncode == 64 and "the stall guard has no launches form" in r.stderr
    r = run(*base, "50", "--plunge", "4", "x.txt")
    assert r.returncode == 64 and "not with --plunge above 1" in r.stderr
    r = run(*base, "50", "--branching", "strong", "x.txt")
    assert r.returncode == 64 and "not with --branching" in r.stderr
    r = run(*base, "50", "--plunge", "1", "--divers", "2", "no_such_file.txt")     # accepted: it gets as far as the input file
    assert r.returncode == 66


def test_node4_argument_errors_come_first(lpx):
    """Checked before any device is looked for: the same answers with and without a GPU.  No handle can be made without a
    device, so the checks that need none come in front of the null handle."""
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    rec, g = lpx._lib.NodeRecord(), lpx._lib.GuardRecord(7, 7)
    nan = float("nan")

    def node4(flags=1, cutoff=0.0, S=0, form=1, out=C.byref(rec), guard=C.byref(g)):
        return L.lpx_bounded_node4(None, 0, None, None, None, None, flags, cutoff, S, 0, None, 1e-6, form, out, guard)

    def err():
        return lpx._lib.last_error()

    for flags in (8, 16, -1):                                 # bit 8 is no flag: the guard is an argument
        assert node4(flags=flags) == EINVAL and "lpx_bounded_node4: unknown flag" in err()
    assert node4(flags=1 | 4, cutoff=nan) == EINVAL and "lpx_bounded_node4: cutoff is NaN" in err()
    for form in (-1, 3):
        assert node4(form=form) == EINVAL and "lpx_bounded_node4: unknown form" in err()
    for S in (-1, -50):
        for form in (0, 1, 2):
            assert node4(S=S, form=form) == EINVAL and "lpx_bounded_node4: stall_events is negative" in err()
    assert node4(S=1, form=0) == EINVAL and "lpx_bounded_node4: the stall guard has no launches form" in err()
    assert node4(S=50, form=0, guard=None) == EINVAL and "the stall guard has no launches form" in err()
    # with S = 0 every form goes on to the checks of lpx_bounded_node3, and so do the on-chip forms with S > 0
    for S, form in ((0, 0), (0, 1), (0, 2), (50, 1), (50, 2)):
        assert node4(S=S, form=form) == EINVAL and "lpx_bounded_node4: null handle" in err(), (S, form)
    assert (g.bland_events, g.first_bland) == (0, -1)         # the guard record is reset where the call gets that far
    # the entry it is built on keeps its own name
    assert L.lpx_bounded_node3(None, 0, None, None, None, None, 1, 0.0, 0, None, 1e-6, 1, C.byref(rec)) == EINVAL
    assert "lpx_bounded_node3: null handle" in err()


def test_run2_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL, ip, dp = lpx._lib.EINVAL, lpx._lib.ip, lpx._lib.dp
    slot = np.zeros(2, dtype=np.int32); K = np.zeros(2, dtype=np.int32); rc = np.zeros(2, dtype=np.int32)
    recs = (lpx._lib.NodeRecord * 2)()
    guards = (lpx._lib.GuardRecord * 2)()
    cut = np.array([0.0, float("nan")])
    sp, kp, rp, cp = slot.ctypes.data_as(ip), K.ctypes.data_as(ip), rc.ctypes.data_as(ip), cut.ctypes.data_as(dp)

    def run(batch=None, B=1, slot=sp, K=kp, flags=1, cutoff=None, S=50, out=recs, guard=guards, rc=rp):
        return L.lpx_node_batch_run2(batch, B, slot, K, None, None, None, None, flags, cutoff, S, 0, None, 1e-6, out, guard, rc)

    def err():
        return lpx._lib.last_error()

    for S in (0, 50):
        assert run(S=S) == EINVAL and "lpx_node_batch_run2: null batch" in err()
        assert run(S=S, guard=None) == EINVAL and "lpx_node_batch_run2: null batch" in err()      # guard may be NULL
    for name in ("out", "rc", "K", "slot"):
        assert run(**{name: None}) == EINVAL and "lpx_node_batch_run2: null " + name in err(), name
    for S in (-1, -7):
        assert run(S=S) == EINVAL and "lpx_node_batch_run2: stall_events is negative" in err()
    for B in (0, -1):
        assert run(B=B) == EINVAL and "lpx_node_batch_run2: B is outside [1, W]" in err()
    for flags in (8, 16, -1):
        assert run(flags=flags) == EINVAL and "lpx_node_batch_run2: unknown flag" in err()
    assert run(B=2, flags=1 | 4, cutoff=cp) == EINVAL and "lpx_node_batch_run2: entry 1: cutoff is NaN" in err()
    assert run(B=2, flags=1 | 4) == EINVAL and "null cutoff" in err()
    assert run(B=2, flags=1, cutoff=cp) == EINVAL and "null batch" in err()          # not read without the flag
    assert L.lpx_node_batch_run(None, 1, sp, kp, None, None, None, None, 1, None, 0, None, 1e-6, recs, rp) == EINVAL
    assert "lpx_node_batch_run: null batch" in err()


def test_python_level_errors(lpx):
    nb = object.__new__(lpx.NodeBatch)          # no handles are needed to reach the checks
    nb._handles, nb._W, nb._h = [], 2, None
    with pytest.raises(ValueError, match="stall_events must not be negative"):
        nb.run([0], [([], [], [])], 4, stall_events=-1)
    with pytest.raises(ValueError, match=r"B must be in \[1, W\]"):
        nb.run([0, 1, 2], [([], [], [])] * 3, 4, stall_events=50)
    dt = object.__new__(lpx.DeviceTableau)
    dt._h = None
    with pytest.raises(ValueError, match="stall_events must not be negative"):
        dt.bounded_node([], [], [], 4, stall_events=-1)
    with pytest.raises(ValueError, match="no launches form"):
        dt.bounded_node([], [], [], 4, stall_events=50, form="launches")
    with pytest.raises(ValueError, match="unknown node form"):
        dt.bounded_node([], [], [], 4, stall_events=50, form="resident")
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    S = lpx.LPSolver()
    with pytest.raises(ValueError, match="launches"):
        S.SolveBnbBounded(prob, [4, 3, 3], stall_events=50, node_form="launches")
    with pytest.raises(ValueError, match="plunge"):
        S.SolveBnbBounded(prob, [4, 3, 3], stall_events=50, plunge=4)
    for rule in ("strong", "most_fractional"):
        with pytest.raises(ValueError, match="branching"):
            S.SolveBnbBounded(prob, [4, 3, 3], stall_events=50, branching=rule)
    with pytest.raises(ValueError, match="stall_events must not be negative"):
        S.SolveBnbBounded(prob, [4, 3, 3], stall_events=-1)
    with pytest.raises(lpx.SolverException) as e:
        S.SolveBnbBounded(prob, [4, 3, 3], stall_events=50, divers=0)
    assert e.value.code == lpx._lib.EINVAL and "lpx_solve_bnb_bounded7: divers is outside" in str(e.value)


def test_driver_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r, info, dinfo, ginfo = lpx._lib.Result(), lpx._lib.BnbBoundedInfo(), lpx._lib.BnbDiversInfo(), lpx._lib.BnbGuardInfo()
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)

    def solve(max_nodes=0, flags=0, divers=2, S=50, out=C.byref(r)):
        return L.lpx_solve_bnb_bounded7(C.byref(p), None, upp, None, None, max_nodes, flags, divers, S, out, C.byref(info),
                                        C.byref(dinfo), C.byref(ginfo))

    for W in (0, 1025, -3):
        assert solve(divers=W) == EINVAL and "lpx_solve_bnb_bounded7: divers is outside [1, 1024]" in lpx._lib.last_error()
    for S in (-1, -50):
        assert solve(S=S) == EINVAL and "lpx_solve_bnb_bounded7: stall_events is negative" in lpx._lib.last_error()
    for S in (0, 50):
        for flags in (1, 8, 2 | 16):                            # bit 8 stays unknown: the guard is no flag
            assert solve(flags=flags, S=S) == EINVAL and "search_flags" in lpx._lib.last_error()
        assert solve(max_nodes=-1, S=S) == EINVAL and "max_nodes is negative" in lpx._lib.last_error()
    assert solve(out=None) == EINVAL and "lpx_solve_bnb_bounded7: null argument" in lpx._lib.last_error()
    frac = np.array([4.0, 2.5, 3.0])
    rc = L.lpx_solve_bnb_bounded7(C.byref(p), None, frac.ctypes.data_as(lpx._lib.dp), None, None, 0, 0, 2, 50, C.byref(r), None, None, None)
    assert rc == EINVAL and "needs finite, integral lower and upper bounds" in lpx._lib.last_error()


@pytest.mark.parametrize("S", [0, 50])
def test_no_cpu_fallback(lpx, S):
    """Without a device the driver is LPX_EDEVICE; with one it solves."""
    L = lpx._lib.lib()
    p, hold = _problem(lpx)
    r, info, dinfo, ginfo = lpx._lib.Result(), lpx._lib.BnbBoundedInfo(), lpx._lib.BnbDiversInfo(), lpx._lib.BnbGuardInfo()
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)
    rc = L.lpx_solve_bnb_bounded7(C.byref(p), None, upp, None, None, 0, 0, 2, S, C.byref(r), C.byref(info), C.byref(dinfo),
                                  C.byref(ginfo))
    if L.lpx_device_count() > 0:
        assert rc == 0 and info.nodes >= 1 and dinfo.rounds >= 1 and ginfo.max_events >= 0
        L.lpx_bnb_bounded_info_free(C.byref(info)); L.lpx_bnb_divers_info_free(C.byref(dinfo))
        L.lpx_result_free(C.byref(r))
    else:
        assert rc == lpx._lib.EDEVICE and "no HIP device" in lpx._lib.last_error()
