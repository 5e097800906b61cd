"""CPU checks of the entry points of the on-chip node (lpx_bounded_node_fits, lpx_bounded_node3, lpx_solve_bnb_bounded3):
exported and declared, mirrored in C# and Python, the fit rule at its stated points, argument errors before device errors with
their messages.  The argument errors that need a live handle (nint, tol, a repeated column, a NULL out) are in the one test of
this file that is marked gpu: a handle needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_bounded_node_fits", "lpx_bounded_node3", "lpx_solve_bnb_bounded3")


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
    for name, value in (("LAUNCHES", 0), ("ONCHIP", 1), ("AUTO", 2)):
        assert re.search(r"#define LPX_NODE_%s %d\b" % (name, value), hdr)
        assert getattr(lpx._lib, "NODE_" + name) == value and "LPX_NODE_%s = %d" % (name, value) in native
    assert lpx._lib.NODE_FORMS == {"launches": 0, "onchip": 1, "auto": 2}
    assert L.lpx_abi_version() == 1
    assert hasattr(lpx.DeviceTableau, "bounded_node_fits")
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "--node-form" in cli and "lpx_solve_bnb_bounded3(" in cli
    bench = open(os.path.join(ROOT, "tools", "bench_bnb_bounded.py")).read()
    assert "--node-form" in bench


def test_fit_rule(lpx):
    fits = lpx._lib.lib().lpx_bounded_node_fits
    for R, Cc in ((65, 193), (130, 134), (66, 256), (9, 1026), (2, 5), (3, 4), (13, 73)):
        assert fits(R, Cc) == 1, (R, Cc)
    for R, Cc in ((257, 769), (1, 5), (769, 1281), (0, 10), (-3, 4), (5, 0)):
        assert fits(R, Cc) == 0, (R, Cc)
    # the stated guarantee: 1 whenever R >= 2 and R*C + 2*(R + C) <= 18000 doubles -- along its edge for a sweep of widths
    for Cc in (1, 2, 3, 5, 17, 64, 65, 193, 255, 256, 1024, 1025, 4095, 4497):
        R = (18000 - 2 * Cc) // (Cc + 2)
        if R >= 2:
            assert R * Cc + 2 * (R + Cc) <= 18000 and fits(R, Cc) == 1, (R, Cc)
    # the tile alone beyond the LDS of one compute unit
    for R, Cc in ((128, 160), (161, 128), (2, 10240), (20481, 1)):
        assert R * Cc * 8 >= 160 * 1024 and fits(R, Cc) == 0, (R, Cc)
    # monotone in R at a fixed C
    for Cc in (5, 64, 193, 1026):
        seen = [fits(R, Cc) for R in range(2, 4000)]
        assert seen[0] == 1 and seen[-1] == 0 and sorted(seen, reverse=True) == seen, Cc


def test_argument_errors_come_first(lpx):
    """Checked before any device is looked for: the same answers with and without a GPU."""
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    cols = np.array([0], dtype=np.int32); lo = np.array([0.0]); up = np.array([1.0])
    args = (1, cols.ctypes.data_as(lpx._lib.ip), lo.ctypes.data_as(lpx._lib.dp), up.ctypes.data_as(lpx._lib.dp), None)
    rec = lpx._lib.NodeRecord()
    for form in (0, 1, 2):
        assert L.lpx_bounded_node3(None, *args, 1, 0.0, 1, None, 1e-6, form, C.byref(rec)) == EINVAL
        assert "lpx_bounded_node3: null handle" in lpx._lib.last_error()
    for form in (-1, 3, 99):
        assert L.lpx_bounded_node3(None, *args, 1, 0.0, 1, None, 1e-6, form, C.byref(rec)) == EINVAL
        assert "lpx_bounded_node3: unknown form" in lpx._lib.last_error()
    for flags in (8, 16, -1):
        assert L.lpx_bounded_node3(None, *args, flags, 0.0, 1, None, 1e-6, 1, C.byref(rec)) == EINVAL
        assert "lpx_bounded_node3: unknown flag" in lpx._lib.last_error()
    assert L.lpx_bounded_node3(None, *args, 1 | 4, float("nan"), 1, None, 1e-6, 1, C.byref(rec)) == EINVAL
    assert "lpx_bounded_node3: cutoff is NaN" in lpx._lib.last_error()
    assert L.lpx_bounded_node3(None, *args, 1, float("nan"), 1, None, 1e-6, 1, C.byref(rec)) == EINVAL      # not read without the flag
    assert "null handle" in lpx._lib.last_error()


def test_driver_rejects_bad_flags_and_forms(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r, info = lpx._lib.Result(), lpx._lib.BnbBoundedInfo()
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)
    for form in (-1, 3):
        assert L.lpx_solve_bnb_bounded3(C.byref(p), None, upp, None, None, 0, 0, form, C.byref(r), C.byref(info)) == EINVAL
        assert "lpx_solve_bnb_bounded3: unknown node_form" in lpx._lib.last_error()
    for form in (0, 1, 2):
        for flags in (1, 8, 2 | 16):
            assert L.lpx_solve_bnb_bounded3(C.byref(p), None, upp, None, None, 0, flags, form, C.byref(r), C.byref(info)) == EINVAL
            assert "search_flags" in lpx._lib.last_error()
        assert L.lpx_solve_bnb_bounded3(C.byref(p), None, upp, None, None, 0, 0, form, None, None) == EINVAL
        assert "lpx_solve_bnb_bounded3: null argument" in lpx._lib.last_error()
        assert L.lpx_solve_bnb_bounded3(C.byref(p), None, upp, None, None, -1, 0, form, C.byref(r), None) == EINVAL
        assert "max_nodes is negative" in lpx._lib.last_error()
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    with pytest.raises(ValueError):
        lpx.LPSolver().SolveBnbBounded(prob, [4, 3, 3], node_form="fast")


def test_no_cpu_fallback_without_a_gpu(lpx):
    L = lpx._lib.lib()
    if L.lpx_device_count() > 0:
        pytest.skip("a GPU is visible")
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)
    for form in (0, 1, 2):
        assert L.lpx_solve_bnb_bounded3(C.byref(p), None, upp, None, None, 0, 0, form, C.byref(r), None) == lpx._lib.EDEVICE


@pytest.mark.gpu
def test_handle_argument_errors_leave_the_handle_alone(gpu):
    """nint outside [0, Cm], tol outside [0, 0.5), a repeated column, a NULL out, resident = 1: LPX_EINVAL with the messages of
    lpx_bounded_node2 under the new name, in every form, with the handle untouched."""
    import _bounded_ref as B
    L = gpu._lib.lib()
    T, basis, ub, _ = B.binary_bounded(12, 6, 1)
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        before = dt.download()[0].copy()
        for form in ("launches", "onchip", "auto"):
            for kw, what in (({"nint": 99}, "lpx_bounded_node3: nint is outside [0, C-1]"),
                             ({"nint": 12, "tol": 0.5}, "lpx_bounded_node3: tol is not in [0, 0.5)"),
                             ({"nint": 12, "resident": 1}, "lpx_bounded_node3: there is no resident form")):
                with pytest.raises(gpu.LpxError) as e:
                    dt.bounded_node([0], [0.0], [1.0], form=form, **kw)
                assert e.value.code == gpu._lib.EINVAL and what in str(e.value), str(e.value)
            with pytest.raises(gpu.LpxError) as e:
                dt.bounded_node([0, 0], [0.0, 0.0], [1.0, 1.0], 12, form=form)
            assert "lpx_bounded_node3: cols[1] repeats a column" in str(e.value)
            cols = np.array([0], dtype=np.int32); lo = np.array([0.0]); up = np.array([1.0])
            assert L.lpx_bounded_node3(dt._h, 1, cols.ctypes.data_as(gpu._lib.ip), lo.ctypes.data_as(gpu._lib.dp),
                                       up.ctypes.data_as(gpu._lib.dp), None, 1, 0.0, 12, None, 1e-6, gpu._lib.NODE_FORMS[form],
                                       None) == gpu._lib.EINVAL
            assert "lpx_bounded_node3: null out" in gpu._lib.last_error()
        assert np.array_equal(dt.download()[0].view(np.uint64), before.view(np.uint64))
