"""CPU checks of the post-optimal entry points (lpx_tableau_rhs_update / _objective_update / _add_column / _add_row and
lpx_session_*): exported, ABI version unchanged, the C# and Python mirrors of lpx_session_opts field by field, argument
errors before device errors, and no CPU fallback without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_gmi_abi import _c_fields, _cs_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_tableau_rhs_update", "lpx_tableau_objective_update", "lpx_tableau_add_column", "lpx_tableau_add_row",
           "lpx_default_session_opts", "lpx_session_open", "lpx_session_set_rhs", "lpx_session_set_cost",
           "lpx_session_add_variable", "lpx_session_add_constraint", "lpx_session_ranging", "lpx_session_shape",
           "lpx_session_close")


def _problem(lpx):
    c = np.array([3.0, 5.0]); A = np.array([[1.0, 0.0], [0.0, 2.0], [3.0, 2.0]]); b = np.array([4.0, 12.0, 18.0])
    rel = np.zeros(3, dtype=np.int32)
    p = lpx._lib.Problem(0, 2, 3, c.ctypes.data_as(lpx._lib.dp), A.ctypes.data_as(lpx._lib.dp),
                         rel.ctypes.data_as(lpx._lib.ip), b.ctypes.data_as(lpx._lib.dp))
    return p, (c, A, b, rel)


def test_symbols_exported_and_abi_version_unchanged(lpx):
    L = lpx._lib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
    assert L.lpx_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, hdr), s
    seg = int(re.search(r"#define LPX_POSTOPT_SEG (\d+)", hdr).group(1))
    assert seg in (32, 64)
    import _postopt_ref as P
    assert P.SEG == seg


def test_session_opts_mirrors_and_defaults(lpx):
    fields = _c_fields("lpx_session_opts")
    assert fields == ["extra_rows", "extra_cols", "max_iter", "batch", "want_tableau"]
    assert _cs_fields("LpxSessionOpts") == fields
    assert [f for f, _ in lpx._lib.SessionOpts._fields_] == fields
    o = lpx._lib.SessionOpts()
    lpx._lib.lib().lpx_default_session_opts(C.byref(o))
    assert (o.extra_rows, o.extra_cols, o.max_iter, o.batch, o.want_tableau) == (16, 16, 10000, 0, 0)
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    for s in SYMBOLS:
        assert (" %s(" % s) in native, s


def test_tableau_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    cols = (C.c_int32 * 1)(0)
    v = (C.c_double * 1)(1.0)
    assert L.lpx_tableau_rhs_update(None, 1, cols, v) == EINVAL
    assert "null handle" in lpx._lib.last_error()
    assert L.lpx_tableau_objective_update(None, 0, None, None, 0, None, None) == EINVAL
    assert L.lpx_tableau_add_column(None, 1, cols, v, 0.0) == EINVAL
    assert L.lpx_tableau_add_row(None, 0, None, None, v) == EINVAL


def test_session_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    h = C.c_void_p()
    assert L.lpx_session_open(None, None, C.byref(h), C.byref(r)) == EINVAL
    assert L.lpx_session_open(C.byref(p), None, None, C.byref(r)) == EINVAL
    o = lpx._lib.SessionOpts()
    L.lpx_default_session_opts(C.byref(o))
    o.extra_rows = -1
    assert L.lpx_session_open(C.byref(p), C.byref(o), C.byref(h), C.byref(r)) == EINVAL
    bad = np.array([0, 0, 7], dtype=np.int32)
    p.rel = bad.ctypes.data_as(lpx._lib.ip)
    assert L.lpx_session_open(C.byref(p), None, C.byref(h), C.byref(r)) == EINVAL
    i = (C.c_int32 * 1)(0)
    v = (C.c_double * 1)(1.0)
    assert L.lpx_session_set_rhs(None, 1, i, v, C.byref(r)) == EINVAL
    assert L.lpx_session_set_cost(None, 1, i, v, C.byref(r)) == EINVAL
    assert L.lpx_session_add_variable(None, 1.0, v, C.byref(r)) == EINVAL
    assert L.lpx_session_add_constraint(None, v, 0, 1.0, C.byref(r)) == EINVAL
    g = lpx._lib.Ranging()
    assert L.lpx_session_ranging(None, C.byref(g)) == EINVAL
    assert L.lpx_session_shape(None, None, None) == EINVAL
    L.lpx_session_close(None)


def test_no_cpu_fallback_without_a_gpu(lpx):
    L = lpx._lib.lib()
    if L.lpx_device_count() > 0:
        pytest.skip("a GPU is visible")
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    h = C.c_void_p()
    assert L.lpx_session_open(C.byref(p), None, C.byref(h), C.byref(r)) == lpx._lib.EDEVICE
    assert not h.value
    prob = lpx.LPProblem.from_arrays(0, [3, 5], [[1, 0], [0, 2], [3, 2]], [0, 0, 0], [4, 12, 18])
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().Open(prob)
    assert e.value.code == lpx._lib.EDEVICE
