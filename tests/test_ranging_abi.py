"""CPU checks of the ranging entry points (lpx_tableau_ranging, lpx_tableau_ranging_pairs, lpx_solve_ranging,
lpx_ranging_free): exported, ABI version unchanged, the C# mirror of lpx_ranging field by field, argument errors before
device errors, and no CPU fallback without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_tableau_ranging", "lpx_tableau_ranging_pairs", "lpx_solve_ranging", "lpx_ranging_free")


# the same member-name extraction as tests/test_integration_files.py
def _names(decls):
    names = []
    for decl in decls.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        fp = re.match(r".*\(\*\s*(\w+)\)\s*\(", decl)
        if fp:
            names.append(fp.group(1))
            continue
        for part in decl.split(","):
            m = re.search(r"(\w+)\s*(\[\w*\])?\s*$", part)
            if m:
                names.append(m.group(1))
    return names


def _c_fields(struct):
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
    return _names(re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def _cs_fields(struct):
    src = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    body = re.search(r"struct %s[^\{]*\{(.*?)\n    \}" % struct, src, re.S).group(1)
    return _names(re.sub(r"//[^\n]*", "", body))


def _problem(lpx):
    import numpy as np
    c = np.array([3.0, 5.0]); A = np.array([[1.0, 0.0], [0.0, 2.0], [3.0, 2.0]]); b = np.array([4.0, 12.0, 18.0])
    rel = np.zeros(3, dtype=np.int32)
    p = lpx._lib.Problem(0, 2, 3, c.ctypes.data_as(lpx._lib.dp), A.ctypes.data_as(lpx._lib.dp),
                         rel.ctypes.data_as(lpx._lib.ip), b.ctypes.data_as(lpx._lib.dp))
    return p, (c, A, b, rel)


def _solve_ranging(lpx, algorithm):
    p, hold = _problem(lpx)
    r, g = lpx._lib.Result(), lpx._lib.Ranging()
    rc = lpx._lib.lib().lpx_solve_ranging(C.byref(p), algorithm, None, C.byref(r), C.byref(g))
    lpx._lib.lib().lpx_ranging_free(C.byref(g))
    lpx._lib.lib().lpx_result_free(C.byref(r))
    return rc


def test_symbols_exported_and_abi_version_unchanged(lpx):
    L = lpx._lib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
    assert L.lpx_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, hdr), s


def test_csharp_ranging_struct_mirrors_the_header():
    assert _cs_fields("LpxRanging") == _c_fields("lpx_ranging")
    assert _c_fields("lpx_ranging")[:3] == ["n", "m", "valid"]
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    for s in SYMBOLS:
        assert "static extern" in native and (" %s(" % s) in native, s


def test_python_record_mirrors_the_header(lpx):
    assert [f for f, _ in lpx._lib.Ranging._fields_] == _c_fields("lpx_ranging")


def test_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    assert L.lpx_tableau_ranging(None, -1.0, *([None] * 10)) == lpx._lib.EINVAL
    assert L.lpx_tableau_ranging(None, float("nan"), *([None] * 10)) == lpx._lib.EINVAL
    assert L.lpx_tableau_ranging_pairs(None, -1e-9, 0, None, None, None, None, None, None) == lpx._lib.EINVAL
    assert L.lpx_tableau_ranging_pairs(None, 1e-9, 1, None, None, None, None, None, None) == lpx._lib.EINVAL
    for algo in (b"Revised Primal Simplex", b"Branch and Bound", b"Cutting Plane", b"knapsack", b"nonsense", b""):
        assert _solve_ranging(lpx, algo) == lpx._lib.EINVAL, algo
        msg = lpx._lib.last_error()
        assert "Primal Simplex" in msg and "Dual Simplex" in msg
    p, hold = _problem(lpx)
    r, g = lpx._lib.Result(), lpx._lib.Ranging()
    assert L.lpx_solve_ranging(C.byref(p), b"Primal Simplex", None, C.byref(r), None) == lpx._lib.EINVAL
    assert L.lpx_solve_ranging(None, b"Primal Simplex", None, C.byref(r), C.byref(g)) == lpx._lib.EINVAL
    L.lpx_ranging_free(None)
    L.lpx_ranging_free(C.byref(g))          # zeroed record: nothing to free


def test_no_cpu_fallback_without_a_gpu(lpx):
    L = lpx._lib.lib()
    if L.lpx_device_count() > 0:
        pytest.skip("a GPU is visible")
    assert L.lpx_tableau_ranging(None, 1e-9, *([None] * 10)) == lpx._lib.EDEVICE
    assert L.lpx_tableau_ranging_pairs(None, 1e-9, 0, None, None, None, None, None, None) == lpx._lib.EDEVICE
    for algo in (b"Primal Simplex", b"primal", b"Dual Simplex", b"dual algorithm"):
        assert _solve_ranging(lpx, algo) == lpx._lib.EDEVICE, algo
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().SolveRanged(lpx.ParseFromText(open(os.path.join(ROOT, "integration", "Input", "example_input.txt")).read()),
                                   "Primal Simplex")
    assert e.value.code == lpx._lib.EDEVICE
