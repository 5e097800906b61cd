"""CPU checks of the GMI cutting-plane entry points (lpx_default_cut_opts, lpx_tableau_gmi_round, lpx_solve_cuts): exported,
ABI version unchanged, defaults, the C# and Python mirrors of lpx_cut_opts field by field, argument errors before device
errors, and no CPU fallback without a GPU (the "GMI Cutting Plane" key is known, so the solve fails on the device)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_default_cut_opts", "lpx_tableau_gmi_round", "lpx_solve_cuts")


def _names(decls):
    names = []
    for decl in decls.split(";"):
        decl = " ".join(decl.split())
        if not decl:
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
    c = np.array([7.0, 10.0]); A = np.array([[-1.0, 3.0], [7.0, 1.0]]); b = np.array([6.0, 35.0])
    rel = np.zeros(2, dtype=np.int32)
    p = lpx._lib.Problem(0, 2, 2, c.ctypes.data_as(lpx._lib.dp), A.ctypes.data_as(lpx._lib.dp),
                         rel.ctypes.data_as(lpx._lib.ip), b.ctypes.data_as(lpx._lib.dp))
    return p, (c, A, b, rel)


def _round(lpx, o, t=None, is_int=None, n_mask=0, first=1):
    k, p = C.c_int(-7), C.c_int(-7)
    mask = None if is_int is None else (C.c_uint8 * len(is_int))(*is_int)
    return lpx._lib.lib().lpx_tableau_gmi_round(t, mask, n_mask, first, C.byref(o) if o is not None else None,
                                                C.byref(k), None, C.byref(p), None)


def test_symbols_exported_and_abi_version_unchanged(lpx):
    L = lpx._lib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
    assert L.lpx_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, hdr), s


def test_default_cut_opts(lpx):
    o = lpx._lib.cut_opts()
    assert (o.cuts_per_round, o.max_rounds, o.max_active, o.purge) == (8, 50, 64, 1)
    assert (o.away, o.coef_eps, o.max_dynamism, o.purge_tol, o.int_tol) == (1e-3, 1e-9, 1e6, 1e-9, 1e-6)
    py = lpx.CutOpts()
    assert [getattr(py, f) for f, _ in o._fields_] == [getattr(o, f) for f, _ in o._fields_]


def test_csharp_and_python_mirror_the_header(lpx):
    fields = _c_fields("lpx_cut_opts")
    assert fields == ["cuts_per_round", "max_rounds", "max_active", "purge", "away", "coef_eps", "max_dynamism",
                      "purge_tol", "int_tol"]
    assert _cs_fields("LpxCutOpts") == fields
    assert [f for f, _ in lpx._lib.CutOpts._fields_] == fields
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    for s in SYMBOLS:
        assert "static extern" in native and (" %s(" % s) in native, s
    algos = open(os.path.join(ROOT, "integration", "csharp", "LpxAlgorithms.cs")).read()
    assert re.search(r'class GmiCuttingPlaneLpx\b.*base\("GMI Cutting Plane"\)', algos)


@pytest.mark.parametrize("field,value", [("cuts_per_round", 0), ("cuts_per_round", 65), ("max_rounds", -1),
                                         ("max_active", 0), ("away", 0.0), ("away", 0.6), ("away", float("nan")),
                                         ("coef_eps", -1e-9), ("coef_eps", 0.5), ("max_dynamism", 0.5),
                                         ("purge_tol", float("nan")), ("int_tol", float("nan"))])
def test_argument_errors_come_first(lpx, field, value):
    L = lpx._lib.lib()
    o = lpx._lib.cut_opts(**{field: value})
    assert _round(lpx, o) == lpx._lib.EINVAL
    assert field in lpx._lib.last_error()
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    assert L.lpx_solve_cuts(C.byref(p), None, C.byref(o), C.byref(r)) == lpx._lib.EINVAL
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().SolveCuts(lpx.LPProblem.from_arrays(0, [1, 1], [[1, 1]], [0], [1]), **{field: value})
    assert e.value.code == lpx._lib.EINVAL


def test_other_argument_errors(lpx):
    L = lpx._lib.lib()
    o = lpx._lib.cut_opts()
    assert _round(lpx, None) == lpx._lib.EINVAL
    assert _round(lpx, o, n_mask=-1) == lpx._lib.EINVAL
    assert _round(lpx, o, n_mask=3) == lpx._lib.EINVAL          # no mask for 3 columns
    assert _round(lpx, o, is_int=[1, 1], n_mask=2) == lpx._lib.EINVAL   # a null handle is an argument error, with or without a GPU
    assert "null handle" in lpx._lib.last_error()
    r = lpx._lib.Result()
    assert L.lpx_solve_cuts(None, None, None, C.byref(r)) == lpx._lib.EINVAL
    p, hold = _problem(lpx)
    assert L.lpx_solve_cuts(C.byref(p), None, None, None) == lpx._lib.EINVAL


def test_no_cpu_fallback_without_a_gpu(lpx):
    L = lpx._lib.lib()
    if L.lpx_device_count() > 0:
        pytest.skip("a GPU is visible")
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    assert L.lpx_solve_cuts(C.byref(p), None, None, C.byref(r)) == lpx._lib.EDEVICE
    for algo in (b"GMI Cutting Plane", b"gmi", b"  GMI   cutting plane algorithm "):
        r = lpx._lib.Result()
        rc = L.lpx_solve(C.byref(p), algo, None, C.byref(r))
        L.lpx_result_free(C.byref(r))
        assert rc == lpx._lib.EDEVICE, (algo, rc)
    prob = lpx.ParseFromText(open(os.path.join(ROOT, "integration", "Input", "example_gmi.txt")).read())
    for call in (lambda: lpx.LPSolver().Solve(prob, "GMI Cutting Plane"), lambda: lpx.LPSolver().SolveCuts(prob),
                 lambda: lpx.GmiCuttingPlane().Solve(prob)):
        with pytest.raises(lpx.SolverException) as e:
            call()
        assert e.value.code == lpx._lib.EDEVICE


def test_cli_cut_options_take_the_library_key_rule(lpx):
    """--cuts-per-round / --cut-rounds need the GMI algorithm, named as lpx_solve accepts it, and no --ranging."""
    cli = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
    path = os.path.join(ROOT, "integration", "Input", "example_gmi.txt")

    def run(*args):
        return subprocess.run([cli, *args, path], capture_output=True, text=True, timeout=120).returncode
    assert run("--algorithm", "Primal Simplex", "--cut-rounds", "4") == 64
    assert run("--algorithm", "gmi", "--ranging", "--cuts-per-round", "2") == 64
    accepted = 0 if lpx._lib.lib().lpx_device_count() > 0 else 69          # 69: no device, the solve itself was tried
    for name in ("GMI Cutting Plane", "gmi", "  GMI   cutting plane Algorithm ", "gmi algorithm"):
        assert run("--algorithm", name, "--cuts-per-round", "2") == accepted, name
    assert lpx.solver._algorithm_key("  GMI   cutting plane Algorithm ") == "gmi cutting plane"
