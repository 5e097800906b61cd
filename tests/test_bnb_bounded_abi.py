"""CPU checks of the entry points of branch and bound by bound changes (lpx_tableau_dualize, lpx_bounded_dual_run2,
lpx_tableau_branch_pick, lpx_bounded_node, lpx_solve_bnb_bounded / lpx_bnb_bounded_info_free): exported and declared, mirrored in
C# and Python, ABI version unchanged, new structs as documented and old ones untouched, argument errors before device errors
with their messages, and no CPU fallback without a GPU.  The argument errors that need a live handle are in
tests/test_gpu_bnb_bounded.py (a handle needs a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_integration_files import _c_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_tableau_dualize", "lpx_bounded_dual_run2", "lpx_tableau_branch_pick", "lpx_bounded_node",
           "lpx_solve_bnb_bounded", "lpx_bnb_bounded_info_free")


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
    assert re.search(r"#define LPX_BDUAL_SKIP_FIXED 1\b", hdr) and lpx._lib.BDUAL_SKIP_FIXED == 1
    assert "LPX_BDUAL_SKIP_FIXED = 1" in native
    assert L.lpx_abi_version() == 1 and re.search(r"#define LPX_ABI_VERSION 1\b", hdr)
    for m in ("dualize", "bounded_dual_run", "branch_pick", "bounded_node"):
        assert hasattr(lpx.DeviceTableau, m), m
    assert hasattr(lpx.LPSolver, "SolveBnbBounded")
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "--bnb-bounded" in cli and "lpx_solve_bnb_bounded(" in cli


def test_new_structs_are_documented_and_old_ones_unchanged(lpx):
    assert _c_fields("lpx_branch_pick") == ["var", "candidates", "x_var", "z"] == [f for f, _ in lpx._lib.BranchPick._fields_]
    assert _c_fields("lpx_node_record") == ["status", "events", "kind0", "kind1", "flips", "unrepairable", "pick"] \
        == [f for f, _ in lpx._lib.NodeRecord._fields_]
    assert _c_fields("lpx_bnb_node_log") == ["depth", "K", "status", "events", "flips", "var", "z"] \
        == [f for f, _ in lpx._lib.BnbNodeLog._fields_]
    assert _c_fields("lpx_bnb_bounded_info") == ["nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible",
                                                 "max_K", "constant", "n_log", "log"] == [f for f, _ in lpx._lib.BnbBoundedInfo._fields_]
    assert C.sizeof(lpx._lib.BranchPick) == 24 and C.sizeof(lpx._lib.NodeRecord) == 64 and C.sizeof(lpx._lib.BnbNodeLog) == 32
    from linear_programming_solver_lpr381_amd import solver
    assert solver.BNB_LOG_DTYPE.itemsize == C.sizeof(lpx._lib.BnbNodeLog)
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
    k = (C.c_int64 * 2)()
    pick, rec = lpx._lib.BranchPick(), lpx._lib.NodeRecord()
    assert L.lpx_tableau_dualize(None, 1e-9, k) == EINVAL
    assert "null handle" in lpx._lib.last_error()
    assert L.lpx_tableau_branch_pick(None, 0, None, 1e-6, C.byref(pick)) == EINVAL
    assert "null handle" in lpx._lib.last_error()
    assert L.lpx_bounded_dual_run2(None, None, 1, lpx._lib.NULL_CB, None, None) == EINVAL
    assert "null tableau" in lpx._lib.last_error()
    assert L.lpx_bounded_dual_run2(None, None, 6, lpx._lib.NULL_CB, None, None) == EINVAL
    assert "unknown flag" in lpx._lib.last_error()
    assert L.lpx_bounded_node(None, 1, cols.ctypes.data_as(lpx._lib.ip), lop, upp, None, 1, None, 1e-6, C.byref(rec)) == EINVAL
    assert "lpx_bounded_node: null handle" in lpx._lib.last_error()


def test_model_argument_errors_come_first(lpx):
    """Checked before any device is looked for: the same answers with and without a GPU."""
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r, info = lpx._lib.Result(), lpx._lib.BnbBoundedInfo()
    up, upp = _vec(lpx, [4.0, 3.0, 3.0])
    assert L.lpx_solve_bnb_bounded(None, None, upp, None, None, 0, C.byref(r), None) == EINVAL
    assert L.lpx_solve_bnb_bounded(C.byref(p), None, upp, None, None, 0, None, None) == EINVAL
    assert "null argument" in lpx._lib.last_error()
    for lower, upper, mask, what in (([5.0, 0, 0], [4.0, 3, 3], None, "below its lower bound"),
                                     (None, [4.0, float("nan"), 3], None, "NaN"),
                                     ([float("-inf"), 0, 0], [4.0, 3, 3], None, "not finite"),
                                     (None, [4.0, float("inf"), 3], None, "integer variable x2 needs finite, integral"),
                                     (None, None, None, "integer variable x1 needs finite, integral"),
                                     (None, [4.0, 2.5, 3], None, "integer variable x2 needs finite, integral"),
                                     ([0.0, 0.0, 0.5], [4.0, 3, 3], None, "integer variable x3 needs finite, integral"),
                                     ([0.0, 0.0, 0.5], [4.0, float("inf"), 3], [1, 0, 1], "integer variable x3 needs finite, integral")):
        lo, lop = _vec(lpx, lower) if lower is not None else (None, None)
        up, upp = _vec(lpx, upper) if upper is not None else (None, None)
        m = np.array(mask, dtype=np.uint8) if mask is not None else None
        mp = m.ctypes.data_as(C.POINTER(C.c_uint8)) if m is not None else None
        assert L.lpx_solve_bnb_bounded(C.byref(p), lop, upp, mp, None, 0, C.byref(r), C.byref(info)) == EINVAL, (lower, upper)
        assert what in lpx._lib.last_error(), lpx._lib.last_error()
        assert info.n_log == 0 and not info.log
    up, upp = _vec(lpx, [4.0, 3.0, 3.0])
    assert L.lpx_solve_bnb_bounded(C.byref(p), None, upp, None, None, -1, C.byref(r), None) == EINVAL
    assert "max_nodes is negative" in lpx._lib.last_error()
    p, hold = _problem(lpx, rel=(0, 1))                         # the preconditions of lpx_solve_bounded, with its messages
    assert L.lpx_solve_bnb_bounded(C.byref(p), None, upp, None, None, 0, C.byref(r), None) == lpx._lib.E_GE_PRESENT
    assert lpx._lib.last_error().startswith("Constraint contains '>=' sign.")
    p, hold = _problem(lpx, b=(10.0, -1.0))
    assert L.lpx_solve_bnb_bounded(C.byref(p), None, upp, None, None, 0, C.byref(r), None) == lpx._lib.E_NEG_RHS
    L.lpx_bnb_bounded_info_free(None)
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().SolveBnbBounded(prob, [4, 2.5, 3])
    assert e.value.code == EINVAL and "integer variable x2" in str(e.value)


def test_no_cpu_fallback_without_a_gpu(lpx):
    L = lpx._lib.lib()
    if L.lpx_device_count() > 0:
        pytest.skip("a GPU is visible")
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    up, upp = _vec(lpx, [4.0, 3.0, 3.0])
    assert L.lpx_solve_bnb_bounded(C.byref(p), None, upp, None, None, 0, C.byref(r), None) == lpx._lib.EDEVICE
    m = np.array([1, 0, 1], dtype=np.uint8)
    up2, upp2 = _vec(lpx, [4.0, float("inf"), 3.0])             # a continuous variable may be unbounded: it gets to the device check
    assert L.lpx_solve_bnb_bounded(C.byref(p), None, upp2, m.ctypes.data_as(C.POINTER(C.c_uint8)), None, 0, C.byref(r), None) \
        == lpx._lib.EDEVICE
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().SolveBnbBounded(prob, [4, 3, 3])
    assert e.value.code == lpx._lib.EDEVICE
    with pytest.raises(lpx.LpxError) as e:
        lpx.DeviceTableau(3, 6)
    assert e.value.code == lpx._lib.EDEVICE
