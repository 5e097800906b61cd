"""CPU checks of the bounded-variable primal simplex entry points (lpx_tableau_set_bounds / _bound_flags / _bounded_solution,
lpx_bounded_run / _counts, lpx_solve_bounded / lpx_bounded_info_free): exported and declared, ABI version unchanged, the C# and
Python mirrors of lpx_bounded_info field by field, argument errors before device errors with nothing touched, the
preconditions of the model-level solve with the reference's messages, and no CPU fallback without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_integration_files import _c_fields, _cs_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
EXAMPLE = os.path.join(ROOT, "integration", "Input", "example_bounded.txt")
SYMBOLS = ("lpx_tableau_set_bounds", "lpx_tableau_bound_flags", "lpx_bounded_run", "lpx_bounded_counts",
           "lpx_tableau_bounded_solution", "lpx_solve_bounded", "lpx_bounded_info_free")
u8p = C.POINTER(C.c_uint8)


def _problem(lpx, rel=(0, 0), b=(10.0, 15.0), sense=0):
    c = np.array([3.0, 5.0, 2.0]); A = np.array([[1.0, 2.0, 2.0], [2.0, 4.0, 3.0]]); b = np.array(b)
    rel = np.array(rel, dtype=np.int32)
    p = lpx._lib.Problem(sense, 3, 2, c.ctypes.data_as(lpx._lib.dp), A.ctypes.data_as(lpx._lib.dp),
                         rel.ctypes.data_as(lpx._lib.ip), b.ctypes.data_as(lpx._lib.dp))
    return p, (c, A, b, rel)


def _vec(lpx, v):
    a = np.array(v, dtype=np.float64)
    return a, a.ctypes.data_as(lpx._lib.dp)


def test_symbols_exported_declared_and_abi_version_unchanged(lpx):
    L = lpx._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert re.search(r"\b%s\(" % s, hdr), s
        assert (" %s(" % s) in native, s
    assert L.lpx_abi_version() == 1
    for m in ("set_bounds", "bound_flags", "bounded_run", "bounded_counts", "bounded_solution"):
        assert hasattr(lpx.DeviceTableau, m), m
    assert hasattr(lpx.LPSolver, "SolveBounded")


def test_bounded_info_mirrors(lpx):
    fields = _c_fields("lpx_bounded_info")
    assert fields == ["ncols", "n", "flip", "ub", "lower"]
    assert _cs_fields("LpxBoundedInfo") == fields
    assert [f for f, _ in lpx._lib.BoundedInfo._fields_] == fields


def test_existing_structs_keep_their_fields(lpx):
    assert [f for f, _ in lpx._lib.Stats._fields_] == _c_fields("lpx_stats")
    assert [f for f, _ in lpx._lib.Result._fields_] == _c_fields("lpx_result")
    assert [f for f, _ in lpx._lib.SolveOpts._fields_] == _c_fields("lpx_solve_opts")
    assert [f for f, _ in lpx._lib.Problem._fields_] == _c_fields("lpx_problem")


def test_handle_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    ub, ubp = _vec(lpx, [1.0, 2.0])
    flags = (C.c_uint8 * 4)()
    assert L.lpx_tableau_set_bounds(None, 2, ubp) == EINVAL
    assert "null handle" in lpx._lib.last_error()
    assert L.lpx_tableau_set_bounds(None, 0, None) == EINVAL
    assert L.lpx_tableau_bound_flags(None, flags) == EINVAL
    assert L.lpx_bounded_run(None, None, lpx._lib.NULL_CB, None, None) == EINVAL
    assert "null tableau" in lpx._lib.last_error()
    k = (C.c_int64 * 3)()
    assert L.lpx_bounded_counts(None, k) == EINVAL
    x = (C.c_double * 2)(); z = C.c_double()
    assert L.lpx_tableau_bounded_solution(None, 2, x, C.byref(z), None) == EINVAL


def test_solve_bounded_argument_errors_come_first(lpx):
    """Checked before any device is looked for: the same answers with and without a GPU."""
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    assert L.lpx_solve_bounded(None, None, None, None, C.byref(r), None) == EINVAL
    assert L.lpx_solve_bounded(C.byref(p), None, None, None, None, None) == EINVAL
    for lower, upper, what in (([5.0, 0, 0], [4.0, 3, 3], "below its lower bound"),      # u < l
                               (None, [4.0, float("nan"), 3], "NaN"),
                               (None, [4.0, -1.0, 3], "below its lower bound"),           # u < l = 0
                               ([float("-inf"), 0, 0], None, "not finite"),
                               ([float("nan"), 0, 0], None, "not finite"),
                               ([float("inf"), 0, 0], None, "not finite")):
        lo, lop = _vec(lpx, lower) if lower is not None else (None, None)
        up, upp = _vec(lpx, upper) if upper is not None else (None, None)
        info = lpx._lib.BoundedInfo()
        assert L.lpx_solve_bounded(C.byref(p), lop, upp, None, C.byref(r), C.byref(info)) == EINVAL, (lower, upper)
        assert what in lpx._lib.last_error(), lpx._lib.last_error()
        assert not info.flip and not info.ub and info.ncols == 0
    L.lpx_bounded_info_free(None)


def test_solve_bounded_preconditions_with_the_reference_messages(lpx):
    L = lpx._lib.lib()
    r = lpx._lib.Result()
    p, hold = _problem(lpx, rel=(0, 1))                        # a >= row: Models/PrimalSimplex.cs:70
    assert L.lpx_solve_bounded(C.byref(p), None, None, None, C.byref(r), None) == lpx._lib.E_GE_PRESENT
    assert lpx._lib.last_error().startswith("Constraint contains '>=' sign. The Primal Simplex method cannot handle this.")
    p, hold = _problem(lpx, b=(10.0, -1.0))                    # negative RHS as given: :75
    assert L.lpx_solve_bounded(C.byref(p), None, None, None, C.byref(r), None) == lpx._lib.E_NEG_RHS
    assert lpx._lib.last_error().startswith("Constraint has a negative RHS value. The Primal Simplex method cannot handle this.")
    p, hold = _problem(lpx)                                    # negative RHS after the shift: 10 - (1*3 + 2*3 + 2*1) = -1
    lo, lop = _vec(lpx, [3.0, 3.0, 1.0])
    assert L.lpx_solve_bounded(C.byref(p), lop, None, None, C.byref(r), None) == lpx._lib.E_NEG_RHS
    assert lpx._lib.last_error().startswith("Constraint has a negative RHS value.")
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().SolveBounded(prob, upper=[4, 3, 3], lower=[5, 0, 0])
    assert e.value.code == lpx._lib.EINVAL


def test_unknown_algorithm_behaviour_is_unchanged(lpx):
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().Solve(prob, "Bounded Dual Simplex")
    assert e.value.code == lpx._lib.E_UNKNOWN_ALGO and "Algorithm not supported: 'Bounded Dual Simplex'" in str(e.value)


def test_cli_bound_options(lpx):
    assert os.path.exists(CLI) and os.path.exists(EXAMPLE)
    help_ = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert help_.returncode == 0 and "--upper J=V" in help_.stdout and "--binary" in help_.stdout
    for extra in (["--ranging"], ["--cut-rounds", "3", "--algorithm", "gmi"], ["--algorithm", "Dual Simplex"]):
        r = subprocess.run([CLI, "--binary"] + extra + [EXAMPLE], capture_output=True, text=True)
        assert r.returncode == 64 and "--upper / --lower / --binary" in r.stderr, (extra, r.stderr)
    for bad in ("0=1", "x=1", "2", "2=abc"):
        r = subprocess.run([CLI, "--upper", bad, EXAMPLE], capture_output=True, text=True)
        assert r.returncode == 64, bad
    r = subprocess.run([CLI, "--upper", "4=1", EXAMPLE], capture_output=True, text=True)
    assert r.returncode == 64 and "index out of range" in r.stderr


def test_no_cpu_fallback_without_a_gpu(lpx):
    L = lpx._lib.lib()
    if L.lpx_device_count() > 0:
        pytest.skip("a GPU is visible")
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    up, upp = _vec(lpx, [4.0, 3.0, 3.0])
    assert L.lpx_solve_bounded(C.byref(p), None, upp, None, C.byref(r), None) == lpx._lib.EDEVICE
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().SolveBounded(prob, upper=[4, 3, 3])
    assert e.value.code == lpx._lib.EDEVICE
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().Solve(prob, "Bounded Primal Simplex")
    assert e.value.code == lpx._lib.EDEVICE
    r = subprocess.run([CLI, "--binary", EXAMPLE], capture_output=True, text=True)
    assert r.returncode == 69 and "no CPU fallback" in r.stderr
