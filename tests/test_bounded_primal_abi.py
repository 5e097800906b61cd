"""CPU checks of the entry points of the on-chip bounded primal loop (lpx_bounded_run2, lpx_node_batch_primal, lpx_solve_bounded2,
lpx_solve_bounded_batch, lpx_solve_bnb_bounded8): exported and declared, mirrored in C# and Python, ABI version unchanged, the
record as documented, every LPX_EINVAL that needs no device returned before the device check with its message, the fit rule at
its edges, and no CPU fallback without a GPU.  The argument errors that need a live handle or a live batch (B above W, a repeated
slot) are in tests/test_gpu_bounded_primal.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_integration_files import _c_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_bounded_run2", "lpx_node_batch_primal", "lpx_solve_bounded2", "lpx_solve_bounded_batch", "lpx_solve_bnb_bounded8")
LAUNCHES, ONCHIP, AUTO = 0, 1, 2


def _problem(lpx, n=3, m=2, rel=None, sense=0):
    """Max sum x, rows of ones <= 10: any shape; the arrays are kept alive by the second value."""
    c = np.ones(n); A = np.ones((m, n)); b = np.full(m, 10.0)
    rel = np.zeros(m, dtype=np.int32) if rel is None else np.array(rel, dtype=np.int32)
    p = lpx._lib.Problem(sense, n, m, c.ctypes.data_as(lpx._lib.dp), A.ctypes.data_as(lpx._lib.dp),
                         rel.ctypes.data_as(lpx._lib.ip), b.ctypes.data_as(lpx._lib.dp))
    return p, (c, A, b, rel)


def _vec(lpx, v):
    a = np.array(v, dtype=np.float64)
    return a, a.ctypes.data_as(lpx._lib.dp)


def test_symbols_exported_declared_mirrored_and_abi_version_unchanged(lpx):
    L = lpx._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s          # a ctypes signature in _lib.py
        assert re.search(r"\b%s\(" % s, hdr), s
        assert (" %s(" % s) in native, s
        assert s in guide, s
    assert L.lpx_abi_version() == 1 and re.search(r"#define LPX_ABI_VERSION 1\b", hdr)
    assert lpx._lib.NODE_FORMS == {"launches": LAUNCHES, "onchip": ONCHIP, "auto": AUTO}
    assert hasattr(lpx.LPSolver, "SolveBoundedBatch") and hasattr(lpx.NodeBatch, "solve")
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "--bounded-form" in cli and "--root-form" in cli and "lpx_solve_bounded2(" in cli and "lpx_solve_bnb_bounded8(" in cli


def test_primal_record_layout(lpx):
    assert _c_fields("lpx_primal_record") == ["status", "events", "kind0", "kind1", "flips", "z"] \
        == [f for f, _ in lpx._lib.PrimalRecord._fields_]
    assert C.sizeof(lpx._lib.PrimalRecord) == 40
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    assert "struct LpxPrimalRecord" in native


def test_fit_rule_at_its_edges(lpx):
    fits = lpx._lib.lib().lpx_bounded_node_fits
    assert fits(140, 141) == 1 and fits(16, 1116) == 1 and fits(65, 193) == 1
    assert fits(141, 142) == 0 and fits(257, 769) == 0


def test_handle_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    cb = lpx._lib.NULL_CB
    for bad in (3, -1, 99):
        assert L.lpx_bounded_run2(None, None, bad, cb, None, None) == EINVAL
        assert "lpx_bounded_run2: unknown form" in lpx._lib.last_error()
    for form in (LAUNCHES, ONCHIP, AUTO):                       # the argument errors of lpx_bounded_run with the new name in front
        assert L.lpx_bounded_run2(None, None, form, cb, None, None) == EINVAL
        assert "lpx_bounded_run2: null tableau" in lpx._lib.last_error()
    assert L.lpx_bounded_run(None, None, cb, None, None) == EINVAL       # the old entry point keeps its own name
    assert "lpx_bounded_run: null tableau" in lpx._lib.last_error()


def test_batch_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    slot = np.zeros(2, dtype=np.int32); rc = np.zeros(2, dtype=np.int32)
    recs = (lpx._lib.PrimalRecord * 2)()
    sp, rp = slot.ctypes.data_as(lpx._lib.ip), rc.ctypes.data_as(lpx._lib.ip)
    for args, what in (((None, 1, None, None, recs, rp), "null slot"), ((None, 1, sp, None, None, rp), "null out"),
                       ((None, 1, sp, None, recs, None), "null rc")):
        assert L.lpx_node_batch_primal(*args) == EINVAL
        assert "lpx_node_batch_primal: " + what in lpx._lib.last_error()
    for B in (0, -3):
        assert L.lpx_node_batch_primal(None, B, sp, None, recs, rp) == EINVAL
        assert "lpx_node_batch_primal: B is outside [1, W]" in lpx._lib.last_error()
    assert L.lpx_node_batch_primal(None, 1, sp, None, recs, rp) == EINVAL
    assert "lpx_node_batch_primal: null batch" in lpx._lib.last_error()


def test_model_argument_errors_come_first(lpx):
    """Checked before any device is looked for: the same answers with and without a GPU."""
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r, binfo = lpx._lib.Result(), lpx._lib.BoundedInfo()
    for bad in (3, -1):
        assert L.lpx_solve_bounded2(C.byref(p), None, None, None, bad, C.byref(r), None) == EINVAL
        assert "lpx_solve_bounded2: unknown form" in lpx._lib.last_error()
    assert L.lpx_solve_bounded2(None, None, None, None, ONCHIP, C.byref(r), None) == EINVAL
    assert L.lpx_solve_bounded2(C.byref(p), None, None, None, ONCHIP, None, None) == EINVAL
    assert "lpx_solve_bounded2: null argument" in lpx._lib.last_error()
    # lpx_solve_bounded's own validation comes first, with its messages
    lo, lop = _vec(lpx, [5.0, 0, 0]); up, upp = _vec(lpx, [4.0, 3, 3])
    assert L.lpx_solve_bounded2(C.byref(p), lop, upp, None, ONCHIP, C.byref(r), C.byref(binfo)) == EINVAL
    assert "below its lower bound" in lpx._lib.last_error() and not binfo.flip
    pg, hold_g = _problem(lpx, rel=(0, 1))
    assert L.lpx_solve_bounded2(C.byref(pg), None, None, None, ONCHIP, C.byref(r), None) == lpx._lib.E_GE_PRESENT
    # 256 rows x 512 variables: the 257 x 769 tableau does not fit one compute unit
    big, hold_b = _problem(lpx, n=512, m=256)
    assert L.lpx_solve_bounded2(C.byref(big), None, None, None, ONCHIP, C.byref(r), None) == EINVAL
    assert "257 x 769" in lpx._lib.last_error() and "does not fit" in lpx._lib.last_error()
    # a text callback: the on-chip form reports no event
    seen = []
    o = lpx._lib.SolveOpts()
    L.lpx_default_solve_opts(C.byref(o))
    fn = lpx._lib.TEXT_CB(lambda *a: seen.append(1))
    o.text_cb = fn
    assert L.lpx_solve_bounded2(C.byref(p), None, None, C.byref(o), ONCHIP, C.byref(r), None) == EINVAL
    assert "no per-event callback" in lpx._lib.last_error() and not seen
    prob = lpx.LPProblem.from_arrays(0, np.ones(512), np.ones((256, 512)), [0] * 256, [10.0] * 256)
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().SolveBounded(prob, form="onchip")
    assert e.value.code == EINVAL and "does not fit" in str(e.value)
    with pytest.raises(ValueError):
        lpx.LPSolver().SolveBounded(prob, form="resident")


def test_model_batch_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    big, hold_b = _problem(lpx, n=512, m=256)
    PP = C.POINTER(lpx._lib.Problem)
    rs = (lpx._lib.Result * 3)()
    arr = (PP * 3)(C.pointer(p), C.pointer(p), C.pointer(big))
    for count in (0, -1, 1025):
        assert L.lpx_solve_bounded_batch(count, arr, None, None, None, rs, None) == EINVAL
        assert "lpx_solve_bounded_batch: count is outside [1, 1024]" in lpx._lib.last_error()
    assert L.lpx_solve_bounded_batch(3, None, None, None, None, rs, None) == EINVAL
    assert L.lpx_solve_bounded_batch(3, arr, None, None, None, None, None) == EINVAL
    assert "lpx_solve_bounded_batch: null argument" in lpx._lib.last_error()
    assert L.lpx_solve_bounded_batch(3, arr, None, None, None, rs, None) == EINVAL       # the third model does not fit
    assert "model 2:" in lpx._lib.last_error() and "does not fit" in lpx._lib.last_error()
    assert not rs[0].x and not rs[1].x
    # a model's own validation error names the model too
    lo, lop = _vec(lpx, [5.0, 0, 0]); up, upp = _vec(lpx, [4.0, 3, 3])
    los = (lpx._lib.dp * 3)(None, lop, None); ups = (lpx._lib.dp * 3)(None, upp, None)
    assert L.lpx_solve_bounded_batch(2, arr, los, ups, None, rs, None) == EINVAL
    assert "model 1:" in lpx._lib.last_error() and "below its lower bound" in lpx._lib.last_error()
    with pytest.raises(ValueError):
        lpx.LPSolver().SolveBoundedBatch([])


def test_root_form_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    up, upp = _vec(lpx, [4.0, 3.0, 3.0])
    for bad in (3, -1):
        assert L.lpx_solve_bnb_bounded8(C.byref(p), None, upp, None, None, 0, 0, 1, 0, bad, C.byref(r), None, None, None) == EINVAL
        assert "lpx_solve_bnb_bounded8: unknown root_form" in lpx._lib.last_error()
    assert L.lpx_solve_bnb_bounded8(C.byref(p), None, upp, None, None, 0, 0, 0, 0, ONCHIP, C.byref(r), None, None, None) == EINVAL
    assert "lpx_solve_bnb_bounded8: divers is outside [1, 1024]" in lpx._lib.last_error()
    assert L.lpx_solve_bnb_bounded8(C.byref(p), None, upp, None, None, 0, 0, 1, -1, ONCHIP, C.byref(r), None, None, None) == EINVAL
    assert "stall_events is negative" in lpx._lib.last_error()
    assert L.lpx_solve_bnb_bounded8(None, None, upp, None, None, 0, 0, 1, 0, ONCHIP, C.byref(r), None, None, None) == EINVAL
    assert "lpx_solve_bnb_bounded8: null argument" in lpx._lib.last_error()
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    S = lpx.LPSolver()
    with pytest.raises(ValueError):
        S.SolveBnbBounded(prob, [4, 3, 3], root_form="resident")
    for kw in ({"plunge": 2}, {"branching": "strong"}, {"node_form": "launches"}):
        with pytest.raises(ValueError):
            S.SolveBnbBounded(prob, [4, 3, 3], root_form="onchip", **kw)


def test_no_cpu_fallback_without_a_gpu(lpx):
    L = lpx._lib.lib()
    if L.lpx_device_count() > 0:
        pytest.skip("a GPU is visible")
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    up, upp = _vec(lpx, [4.0, 3.0, 3.0])
    for form in (LAUNCHES, ONCHIP, AUTO):
        assert L.lpx_solve_bounded2(C.byref(p), None, upp, None, form, C.byref(r), None) == lpx._lib.EDEVICE
        assert L.lpx_solve_bnb_bounded8(C.byref(p), None, upp, None, None, 0, 0, 1, 0, form, C.byref(r), None, None, None) == lpx._lib.EDEVICE
    PP = C.POINTER(lpx._lib.Problem)
    rs = (lpx._lib.Result * 1)()
    assert L.lpx_solve_bounded_batch(1, (PP * 1)(C.pointer(p)), None, None, None, rs, None) == lpx._lib.EDEVICE
