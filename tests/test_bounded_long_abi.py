"""CPU checks of the entry points of the long-step ratio test, the objective cutoff and the dual start (lpx_bounded_dual_run3,
lpx_bounded_node2, lpx_solve_bnb_bounded2, lpx_solve_bounded_dual): exported and declared, mirrored in C# and Python, ABI version
unchanged, the new status and flags as documented, old structs untouched, argument errors before device errors with their
messages, and no CPU fallback without a GPU.  The argument errors that need a live handle are in tests/test_gpu_bounded_long.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_integration_files import _c_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_bounded_dual_run3", "lpx_bounded_node2", "lpx_solve_bnb_bounded2", "lpx_solve_bounded_dual")
NAN = float("nan")


def _problem(lpx, c=(3.0, 5.0, 2.0), rel=(0, 0), b=(10.0, 15.0), sense=0):
    c = np.array(c); A = np.array([[1.0, 2.0, 2.0], [2.0, 4.0, 3.0]]); b = np.array(b)
    rel = np.array(rel, dtype=np.int32)
    p = lpx._lib.Problem(sense, 3, 2, c.ctypes.data_as(lpx._lib.dp), A.ctypes.data_as(lpx._lib.dp),
                         rel.ctypes.data_as(lpx._lib.ip), b.ctypes.data_as(lpx._lib.dp))
    return p, (c, A, b, rel)


def _vec(lpx, v):
    a = np.array(v, dtype=np.float64)
    return a, a.ctypes.data_as(lpx._lib.dp)


def test_symbols_exported_declared_mirrored_and_abi_version_unchanged(lpx):
    L = lpx._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s          # a ctypes signature in _lib.py
        assert re.search(r"\b%s\(" % s, hdr), s
        assert (" %s(" % s) in native, s
    assert re.search(r"#define LPX_BDUAL_LONG_STEP 2\b", hdr) and lpx._lib.BDUAL_LONG_STEP == 2
    assert re.search(r"#define LPX_BDUAL_CUTOFF 4\b", hdr) and lpx._lib.BDUAL_CUTOFF == 4
    assert re.search(r"#define LPX_BDUAL_SKIP_FIXED 1\b", hdr) and lpx._lib.BDUAL_SKIP_FIXED == 1
    assert "LPX_BDUAL_LONG_STEP = 2" in native and "LPX_BDUAL_CUTOFF = 4" in native
    assert L.lpx_abi_version() == 1 and re.search(r"#define LPX_ABI_VERSION 1\b", hdr)
    assert hasattr(lpx.LPSolver, "SolveBoundedDual")
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "--long-step" in cli and "--cutoff" in cli and "lpx_solve_bnb_bounded2(" in cli


def test_cutoff_status_is_the_next_free_value_and_is_named(lpx):
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    assert re.search(r"LPX_RUNNING\s*=\s*4,", hdr) and re.search(r"LPX_CUTOFF\s*=\s*5,", hdr)
    assert lpx._lib.CUTOFF == 5 and lpx._lib.STATUS_NAMES[lpx._lib.CUTOFF] == "CUTOFF"
    assert "CUTOFF = 5" in native
    assert lpx._lib.STATUS_NAMES[lpx._lib.OPTIMAL] == "OPTIMAL" and lpx._lib.RUNNING == 4


def test_old_structs_are_unchanged(lpx):
    assert _c_fields("lpx_node_record") == ["status", "events", "kind0", "kind1", "flips", "unrepairable", "pick"] \
        == [f for f, _ in lpx._lib.NodeRecord._fields_]
    assert _c_fields("lpx_bnb_node_log") == ["depth", "K", "status", "events", "flips", "var", "z"]
    assert _c_fields("lpx_bnb_bounded_info") == ["nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible",
                                                 "max_K", "constant", "n_log", "log"]
    assert _c_fields("lpx_bounded_info") == ["ncols", "n", "flip", "ub", "lower"]
    assert C.sizeof(lpx._lib.NodeRecord) == 64 and C.sizeof(lpx._lib.BnbNodeLog) == 32
    assert [f for f, _ in lpx._lib.RunOpts._fields_] == _c_fields("lpx_run_opts")


def test_handle_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    cb = lpx._lib.NULL_CB
    assert L.lpx_bounded_dual_run3(None, None, 8, 0.0, cb, None, None) == EINVAL
    assert "lpx_bounded_dual_run3: unknown flag" in lpx._lib.last_error()
    assert L.lpx_bounded_dual_run3(None, None, -1, 0.0, cb, None, None) == EINVAL
    assert "unknown flag" in lpx._lib.last_error()
    assert L.lpx_bounded_dual_run3(None, None, 4, NAN, cb, None, None) == EINVAL
    assert "cutoff is NaN" in lpx._lib.last_error()
    assert L.lpx_bounded_dual_run3(None, None, 6, 0.0, cb, None, None) == EINVAL
    assert "null tableau" in lpx._lib.last_error()
    assert L.lpx_bounded_dual_run3(None, None, 2, NAN, cb, None, None) == EINVAL        # without CUTOFF the value is not read
    assert "null tableau" in lpx._lib.last_error()
    assert L.lpx_bounded_dual_run3(None, None, 1, 0.0, cb, None, None) == EINVAL
    assert "null tableau" in lpx._lib.last_error()
    cols = np.array([0], dtype=np.int32); lo, lop = _vec(lpx, [0.0]); up, upp = _vec(lpx, [1.0])
    rec = lpx._lib.NodeRecord()
    cp = cols.ctypes.data_as(lpx._lib.ip)
    assert L.lpx_bounded_node2(None, 1, cp, lop, upp, None, 16, 0.0, 1, None, 1e-6, C.byref(rec)) == EINVAL
    assert "lpx_bounded_node2: unknown flag" in lpx._lib.last_error()
    assert L.lpx_bounded_node2(None, 1, cp, lop, upp, None, 5, NAN, 1, None, 1e-6, C.byref(rec)) == EINVAL
    assert "cutoff is NaN" in lpx._lib.last_error()
    assert L.lpx_bounded_node2(None, 1, cp, lop, upp, None, 7, 0.0, 1, None, 1e-6, C.byref(rec)) == EINVAL
    assert "lpx_bounded_node2: null handle" in lpx._lib.last_error()
    # the old entry point keeps refusing the new bits
    assert L.lpx_bounded_dual_run2(None, None, 2, cb, None, None) == EINVAL
    assert "lpx_bounded_dual_run2: unknown flag" in lpx._lib.last_error()


def test_model_argument_errors_come_first(lpx):
    """Checked before any device is looked for: the same answers with and without a GPU."""
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r, info, binfo = lpx._lib.Result(), lpx._lib.BnbBoundedInfo(), lpx._lib.BoundedInfo()
    up, upp = _vec(lpx, [4.0, 3.0, 3.0])
    assert L.lpx_solve_bnb_bounded2(None, None, upp, None, None, 0, 2, C.byref(r), None) == EINVAL
    assert L.lpx_solve_bnb_bounded2(C.byref(p), None, upp, None, None, 0, 2, None, None) == EINVAL
    assert "lpx_solve_bnb_bounded2: null argument" in lpx._lib.last_error()
    for bad in (1, 8, 7, -2):
        assert L.lpx_solve_bnb_bounded2(C.byref(p), None, upp, None, None, 0, bad, C.byref(r), C.byref(info)) == EINVAL
        assert "search_flags" in lpx._lib.last_error()
        assert info.n_log == 0 and not info.log
    assert L.lpx_solve_bnb_bounded2(C.byref(p), None, upp, None, None, -1, 6, C.byref(r), None) == EINVAL
    assert "max_nodes is negative" in lpx._lib.last_error()
    up2, upp2 = _vec(lpx, [4.0, 2.5, 3.0])
    assert L.lpx_solve_bnb_bounded2(C.byref(p), None, upp2, None, None, 0, 6, C.byref(r), None) == EINVAL
    assert "integer variable x2 needs finite, integral" in lpx._lib.last_error()
    pg, hold_g = _problem(lpx, rel=(0, 1))                      # the root is still the primal loop
    assert L.lpx_solve_bnb_bounded2(C.byref(pg), None, upp, None, None, 0, 6, C.byref(r), None) == lpx._lib.E_GE_PRESENT

    assert L.lpx_solve_bounded_dual(None, None, upp, 2, None, C.byref(r), None) == EINVAL
    assert L.lpx_solve_bounded_dual(C.byref(p), None, upp, 2, None, None, None) == EINVAL
    assert "lpx_solve_bounded_dual: null argument" in lpx._lib.last_error()
    for bad in (4, 6, 8, -1):
        assert L.lpx_solve_bounded_dual(C.byref(p), None, upp, bad, None, C.byref(r), C.byref(binfo)) == EINVAL
        assert "flags" in lpx._lib.last_error()
    for lower, upper, what in (([5.0, 0, 0], [4.0, 3, 3], "below its lower bound"), (None, [4.0, NAN, 3], "NaN"),
                               ([float("-inf"), 0, 0], [4.0, 3, 3], "not finite")):
        lo, lop = _vec(lpx, lower) if lower is not None else (None, None)
        u, upv = _vec(lpx, upper)
        assert L.lpx_solve_bounded_dual(C.byref(p), lop, upv, 2, None, C.byref(r), C.byref(binfo)) == EINVAL
        assert what in lpx._lib.last_error()
        assert not binfo.flip and not binfo.ub
    # Max 3 x1 + 5 x2 + 2 x3: every variable improves.  x2 is the first one without an upper bound.
    u, upv = _vec(lpx, [4.0, float("inf"), float("inf")])
    assert L.lpx_solve_bounded_dual(C.byref(pg), None, upv, 2, None, C.byref(r), None) == EINVAL
    assert "x2 improves the objective and has no upper bound" in lpx._lib.last_error()
    assert L.lpx_solve_bounded_dual(C.byref(p), None, None, 0, None, C.byref(r), None) == EINVAL
    assert "x1 improves the objective and has no upper bound" in lpx._lib.last_error()
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 1], [10, 15])
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().SolveBoundedDual(prob, [4, np.inf, 3])
    assert e.value.code == EINVAL and "x2 improves" in str(e.value)


def test_no_cpu_fallback_without_a_gpu(lpx):
    L = lpx._lib.lib()
    if L.lpx_device_count() > 0:
        pytest.skip("a GPU is visible")
    r = lpx._lib.Result()
    up, upp = _vec(lpx, [4.0, 3.0, 3.0])
    p, hold = _problem(lpx)
    for flags in (2, 4, 6):
        assert L.lpx_solve_bnb_bounded2(C.byref(p), None, upp, None, None, 0, flags, C.byref(r), None) == lpx._lib.EDEVICE
    # what lpx_solve_bounded refuses gets to the device check here: a >= row, a negative right-hand side
    pg, hold_g = _problem(lpx, rel=(0, 1), b=(10.0, -1.0))
    for flags in (0, 1, 2, 3):
        assert L.lpx_solve_bounded_dual(C.byref(pg), None, upp, flags, None, C.byref(r), None) == lpx._lib.EDEVICE
    # a Min of positive costs needs no upper bound at all
    pm, hold_m = _problem(lpx, rel=(1, 1), sense=1)
    assert L.lpx_solve_bounded_dual(C.byref(pm), None, None, 2, None, C.byref(r), None) == lpx._lib.EDEVICE
    prob = lpx.LPProblem.from_arrays(1, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [1, 1], [10, 15])
    for kw in ({}, {"long_step": False}):
        with pytest.raises(lpx.SolverException) as e:
            lpx.LPSolver().SolveBoundedDual(prob, [4, 3, 3], **kw)
        assert e.value.code == lpx._lib.EDEVICE
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    for kw in ({"long_step": True}, {"cutoff": True}, {"long_step": True, "cutoff": True}):
        with pytest.raises(lpx.SolverException) as e:
            lpx.LPSolver().SolveBnbBounded(prob, [4, 3, 3], **kw)
        assert e.value.code == lpx._lib.EDEVICE
