"""CPU checks of the bounded dual simplex entry points (lpx_tableau_bound_state / _change_bounds, lpx_bounded_dual_run,
lpx_bounded_open / _set_bounds / _close): exported and declared, mirrored in C# and Python, ABI version unchanged, existing
structs untouched, argument errors before device errors with their messages, and no CPU fallback without a GPU.  The argument
errors of lpx_tableau_change_bounds that need a live handle are in tests/test_gpu_bounded_dual.py (a handle needs a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_integration_files import _c_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_tableau_bound_state", "lpx_tableau_change_bounds", "lpx_bounded_dual_run", "lpx_bounded_open",
           "lpx_bounded_set_bounds", "lpx_bounded_close")


def _problem(lpx, rel=(0, 0), b=(10.0, 15.0), sense=0):
    c = np.array([3.0, 5.0, 2.0]); A = np.array([[1.0, 2.0, 2.0], [2.0, 4.0, 3.0]]); b = np.array(b)
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
    assert "typedef struct lpx_bounded_session lpx_bounded_session;" in hdr
    assert L.lpx_abi_version() == 1 and re.search(r"#define LPX_ABI_VERSION 1\b", hdr)
    for m in ("change_bounds", "bounded_dual_run", "bound_state"):
        assert hasattr(lpx.DeviceTableau, m), m
    assert hasattr(lpx.LPSolver, "OpenBounded")
    for m in ("set_bounds", "close", "__enter__", "__exit__"):
        assert hasattr(lpx.BoundedSession, m), m


def test_existing_structs_keep_their_fields(lpx):
    assert [f for f, _ in lpx._lib.Stats._fields_] == _c_fields("lpx_stats")
    assert [f for f, _ in lpx._lib.Result._fields_] == _c_fields("lpx_result")
    assert [f for f, _ in lpx._lib.SolveOpts._fields_] == _c_fields("lpx_solve_opts")
    assert [f for f, _ in lpx._lib.Problem._fields_] == _c_fields("lpx_problem")
    assert [f for f, _ in lpx._lib.RunOpts._fields_] == _c_fields("lpx_run_opts")
    assert _c_fields("lpx_bounded_info") == ["ncols", "n", "flip", "ub", "lower"]


def test_handle_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    cols = np.array([0], dtype=np.int32); lo, lop = _vec(lpx, [0.0]); up, upp = _vec(lpx, [1.0])
    assert L.lpx_tableau_change_bounds(None, 1, cols.ctypes.data_as(lpx._lib.ip), lop, upp) == EINVAL
    assert "null handle" in lpx._lib.last_error()
    assert L.lpx_tableau_change_bounds(None, 0, None, None, None) == EINVAL
    assert L.lpx_tableau_bound_state(None, None, None, None) == EINVAL
    assert "null handle" in lpx._lib.last_error()
    assert L.lpx_bounded_dual_run(None, None, lpx._lib.NULL_CB, None, None) == EINVAL
    assert "null tableau" in lpx._lib.last_error()


def test_session_argument_errors_come_first(lpx):
    """Checked before any device is looked for: the same answers with and without a GPU."""
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    h = C.c_void_p()
    assert L.lpx_bounded_open(None, None, None, None, C.byref(h), C.byref(r)) == EINVAL
    assert L.lpx_bounded_open(C.byref(p), None, None, None, None, C.byref(r)) == EINVAL
    assert L.lpx_bounded_open(C.byref(p), None, None, None, C.byref(h), None) == EINVAL
    assert "null argument" in lpx._lib.last_error()
    for lower, upper, what in (([5.0, 0, 0], [4.0, 3, 3], "below its lower bound"),
                               (None, [4.0, float("nan"), 3], "NaN"),
                               (None, [4.0, -1.0, 3], "below its lower bound"),
                               ([float("-inf"), 0, 0], None, "not finite"),
                               ([float("nan"), 0, 0], None, "not finite"),
                               ([float("inf"), 0, 0], None, "not finite")):
        lo, lop = _vec(lpx, lower) if lower is not None else (None, None)
        up, upp = _vec(lpx, upper) if upper is not None else (None, None)
        h = C.c_void_p(1)
        assert L.lpx_bounded_open(C.byref(p), lop, upp, None, C.byref(h), C.byref(r)) == EINVAL, (lower, upper)
        assert what in lpx._lib.last_error(), lpx._lib.last_error()
        assert not h.value                                      # no session is handed out
    p, hold = _problem(lpx, rel=(0, 1))                         # the preconditions of lpx_solve_bounded, with its messages
    assert L.lpx_bounded_open(C.byref(p), None, None, None, C.byref(h), C.byref(r)) == lpx._lib.E_GE_PRESENT
    assert lpx._lib.last_error().startswith("Constraint contains '>=' sign.")
    p, hold = _problem(lpx, b=(10.0, -1.0))
    assert L.lpx_bounded_open(C.byref(p), None, None, None, C.byref(h), C.byref(r)) == lpx._lib.E_NEG_RHS
    cols = np.array([0], dtype=np.int32); lo, lop = _vec(lpx, [0.0]); up, upp = _vec(lpx, [1.0])
    assert L.lpx_bounded_set_bounds(None, 1, cols.ctypes.data_as(lpx._lib.ip), lop, upp, C.byref(r)) == EINVAL
    assert "null argument" in lpx._lib.last_error()
    L.lpx_bounded_close(None)
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().OpenBounded(prob, upper=[4, 3, 3], lower=[5, 0, 0])
    assert e.value.code == EINVAL and "below its lower bound" in str(e.value)


def test_no_cpu_fallback_without_a_gpu(lpx):
    L = lpx._lib.lib()
    if L.lpx_device_count() > 0:
        pytest.skip("a GPU is visible")
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    h = C.c_void_p()
    up, upp = _vec(lpx, [4.0, 3.0, 3.0])
    assert L.lpx_bounded_open(C.byref(p), None, upp, None, C.byref(h), C.byref(r)) == lpx._lib.EDEVICE
    assert not h.value
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().OpenBounded(prob, upper=[4, 3, 3])
    assert e.value.code == lpx._lib.EDEVICE
    with pytest.raises(lpx.LpxError) as e:
        lpx.DeviceTableau(3, 6)
    assert e.value.code == lpx._lib.EDEVICE
