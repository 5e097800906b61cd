"""CPU checks of the entry points of GMI cuts on bounded handles and of cut-and-branch (lpx_tableau_gmi_round_bounded,
lpx_bounded_cut_loop, lpx_solve_bnb_bounded9, lpx_bnb_cut_info_free): exported and declared, mirrored in C# and Python field by
field, argument errors before device errors with their messages, and no CPU fallback without a GPU.  The argument errors that
need a live handle are in the one test of this file that is marked gpu: a handle needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_tableau_gmi_round_bounded", "lpx_bounded_cut_loop", "lpx_solve_bnb_bounded9", "lpx_bnb_cut_info_free")


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
        assert getattr(L, s).argtypes is not None, s
        assert re.search(r"\b%s\(" % s, hdr), s
        assert (" %s(" % s) in native, s
    for i, name in enumerate(("INTEGRAL", "STALLED", "ROUNDS", "INFEASIBLE", "ITER_LIMIT", "STATUS")):
        assert re.search(r"#define LPX_CUTLOOP_%s\s+%d\b" % (name, i), hdr)
        assert lpx._lib.CUTLOOP_STOPS[i] == name.lower()
    assert L.lpx_abi_version() == 1 and re.search(r"#define LPX_ABI_VERSION 1\b", hdr)
    assert hasattr(lpx.DeviceTableau, "cut_loop")
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "--root-cuts" in cli and "lpx_solve_bnb_bounded9(" in cli
    # the statement about the plain round stays in the header, and the plain round's name in its place
    assert "they are not bound-aware" in hdr


def test_struct_layouts(lpx):
    loop = _c_fields("lpx_cut_loop_record")
    assert loop == ["rounds", "added", "purged", "stop", "status", "R", "C", "pad", "events", "pick", "z_before", "z_after"]
    assert [f for f, _ in lpx._lib.CutLoopRecord._fields_] == loop and _cs_fields("LpxCutLoopRecord") == loop
    assert C.sizeof(lpx._lib.CutLoopRecord) == 32 + 8 + 24 + 16
    assert lpx._lib.CutLoopRecord.events.offset == 32 and lpx._lib.CutLoopRecord.pick.offset == 40
    assert lpx._lib.CutLoopRecord.z_before.offset == 64
    info = _c_fields("lpx_bnb_cut_info")
    assert info == ["ran", "spare", "rounds", "added", "purged", "stop", "status", "R", "C", "n_z", "events", "z_before", "z_after"]
    assert [f for f, _ in lpx._lib.BnbCutInfo._fields_] == info and _cs_fields("LpxBnbCutInfo") == info
    assert C.sizeof(lpx._lib.BnbCutInfo) == 40 + 8 + 16 and lpx._lib.BnbCutInfo.events.offset == 40


def _round(lpx, o, t=None, is_int=None, n_mask=0, first=1):
    k, p = C.c_int(-7), C.c_int(-7)
    mask = None if is_int is None else (C.c_uint8 * len(is_int))(*is_int)
    return lpx._lib.lib().lpx_tableau_gmi_round_bounded(t, mask, n_mask, first, C.byref(o) if o is not None else None,
                                                        C.byref(k), None, C.byref(p), None)


def _loop(lpx, o, t=None, is_int=None, n_mask=0, first=1, nint=0, flags=0, form=0, rec=True):
    mask = None if is_int is None else (C.c_uint8 * len(is_int))(*is_int)
    r = lpx._lib.CutLoopRecord()
    return lpx._lib.lib().lpx_bounded_cut_loop(t, mask, n_mask, first, nint, None, C.byref(o) if o is not None else None, None,
                                               flags, form, C.byref(r) if rec else None)


@pytest.mark.parametrize("field,value", [("cuts_per_round", -1), ("cuts_per_round", 65), ("max_rounds", -1), ("max_active", 0),
                                         ("away", 0.0), ("away", 0.6), ("coef_eps", 0.5), ("max_dynamism", 0.5),
                                         ("purge_tol", float("nan")), ("int_tol", float("nan"))])
def test_option_errors_come_first(lpx, field, value):
    o = lpx._lib.cut_opts(**{field: value})
    assert _round(lpx, o) == lpx._lib.EINVAL
    assert "lpx_tableau_gmi_round_bounded" in lpx._lib.last_error() and field in lpx._lib.last_error()
    assert _loop(lpx, o) == lpx._lib.EINVAL
    assert "lpx_bounded_cut_loop" in lpx._lib.last_error() and field in lpx._lib.last_error()


def test_other_argument_errors(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    o = lpx._lib.cut_opts()
    zero = lpx._lib.cut_opts(cuts_per_round=0)                      # allowed here: the next error is the handle's
    for call in (_round, _loop):
        assert call(lpx, None) == EINVAL and "null options" in lpx._lib.last_error()
        assert call(lpx, o, n_mask=-1) == EINVAL and "bad integer mask" in lpx._lib.last_error()
        assert call(lpx, o, n_mask=3) == EINVAL and "bad integer mask" in lpx._lib.last_error()
        assert call(lpx, o, is_int=[1, 1], n_mask=2) == EINVAL and "null handle" in lpx._lib.last_error()
        assert call(lpx, zero, is_int=[1, 1], n_mask=2) == EINVAL and "null handle" in lpx._lib.last_error()
    assert _loop(lpx, o, rec=False) == EINVAL and "lpx_bounded_cut_loop: null record" in lpx._lib.last_error()
    # the plain round keeps its range
    k, p = C.c_int(), C.c_int()
    assert L.lpx_tableau_gmi_round(None, None, 0, 1, C.byref(zero), C.byref(k), None, C.byref(p), None) == EINVAL
    assert "cuts_per_round must be in 1..64" in lpx._lib.last_error()


def test_driver_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)
    co = lpx._lib.cut_opts()

    def call(ps=p, divers=1, stall=0, form=0, cuts=co, res=r, max_nodes=0, flags=0):
        return L.lpx_solve_bnb_bounded9(C.byref(ps) if ps is not None else None, None, upp, None, None, max_nodes, flags, divers, stall,
                                        form, C.byref(cuts) if cuts is not None else None, C.byref(res) if res is not None else None,
                                        None, None, None, None)
    assert call(divers=0) == EINVAL and "lpx_solve_bnb_bounded9: divers is outside [1, 1024]" in lpx._lib.last_error()
    assert call(stall=-1) == EINVAL and "stall_events is negative" in lpx._lib.last_error()
    assert call(form=3) == EINVAL and "lpx_solve_bnb_bounded9: unknown root_form" in lpx._lib.last_error()
    assert call(cuts=lpx._lib.cut_opts(cuts_per_round=0)) == EINVAL and "cuts_per_round must be in 1..64" in lpx._lib.last_error()
    assert call(cuts=lpx._lib.cut_opts(away=0.7)) == EINVAL and "away" in lpx._lib.last_error()
    assert call(ps=None) == EINVAL and "lpx_solve_bnb_bounded9: null argument" in lpx._lib.last_error()
    assert call(res=None) == EINVAL
    assert call(max_nodes=-1) == EINVAL and "max_nodes is negative" in lpx._lib.last_error()
    assert call(flags=8) == EINVAL and "search_flags" in lpx._lib.last_error()
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    S = lpx.LPSolver()
    for kw in ({"plunge": 2}, {"branching": "strong"}, {"node_form": "launches"}):
        with pytest.raises(ValueError):
            S.SolveBnbBounded(prob, [4, 3, 3], root_cuts=2, **kw)
    with pytest.raises(lpx.SolverException) as e:
        S.SolveBnbBounded(prob, [4, 3, 3], root_cuts=2, cuts_per_round=0)
    assert e.value.code == EINVAL


def test_no_cpu_fallback_without_a_gpu(lpx):
    L = lpx._lib.lib()
    if L.lpx_device_count() > 0:
        pytest.skip("a GPU is visible")
    p, hold = _problem(lpx)
    r = lpx._lib.Result()
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)
    co = lpx._lib.cut_opts()
    for cuts in (None, C.byref(co)):
        assert L.lpx_solve_bnb_bounded9(C.byref(p), None, upp, None, None, 0, 0, 1, 0, 0, cuts, C.byref(r), None, None, None,
                                        None) == lpx._lib.EDEVICE
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().SolveBnbBounded(prob, [4, 3, 3], divers=2, root_cuts=2)
    assert e.value.code == lpx._lib.EDEVICE


@pytest.mark.gpu
def test_handle_argument_errors_leave_the_handle_alone(gpu):
    """What needs a live handle: first_cut_col, nint, flags, form, a shape or a capacity that does not fit, bounds set for another
    shape, a handle without bounds -- LPX_EINVAL with the entry point's name in front, the tableau and the bounds untouched."""
    import _bounded_ref as B
    T, basis, ub, _ = B.binary_bounded(12, 6, 1)
    R, Cc = T.shape
    flags = np.ones(Cc - 1, dtype=np.uint8)
    with gpu.DeviceTableau.with_capacity(T, basis, R + 8, Cc + 8) as dt:
        with pytest.raises(gpu.LpxError) as e:
            dt.cut_loop(flags, Cc - 1, 12)
        assert e.value.code == gpu._lib.EINVAL and "lpx_bounded_cut_loop: the handle has no bounds" in str(e.value)
        dt.set_bounds(ub)
        assert dt.bounded_run()[0] == 0
        before = dt.download()[0].copy()
        state = [a.copy() for a in dt.bound_state()]
        for kw, what in ((dict(first_cut_col=0), "first_cut_col outside [1, C-1]"), (dict(first_cut_col=Cc), "first_cut_col outside [1, C-1]")):
            for fn, name in ((lambda **k: dt.gmi_round(flags, bounded=True, **k), "lpx_tableau_gmi_round_bounded"),
                             (lambda **k: dt.cut_loop(flags, nint=12, **k), "lpx_bounded_cut_loop")):
                with pytest.raises(gpu.LpxError) as e:
                    fn(**kw)
                assert e.value.code == gpu._lib.EINVAL and name + ": " + what in str(e.value)
        with pytest.raises(gpu.LpxError) as e:
            dt.cut_loop(flags, Cc - 1, 99)
        assert "lpx_bounded_cut_loop: nint is outside [0, C-1]" in str(e.value)
        with pytest.raises(gpu.LpxError) as e:
            dt.cut_loop(flags, Cc - 1, 12, int_tol=0.5)
        assert "lpx_bounded_cut_loop: tol is not in [0, 0.5)" in str(e.value)
        with pytest.raises(ValueError):
            dt.cut_loop(flags, Cc - 1, 12, form="fast")
        rec = gpu._lib.CutLoopRecord()
        o = gpu._lib.cut_opts()
        fp = flags.ctypes.data_as(C.POINTER(C.c_uint8))
        L = gpu._lib.lib()
        assert L.lpx_bounded_cut_loop(dt._h, fp, Cc - 1, Cc - 1, 12, None, C.byref(o), None, 8, 0, C.byref(rec)) == gpu._lib.EINVAL
        assert "lpx_bounded_cut_loop: unknown flag" in gpu._lib.last_error()
        assert L.lpx_bounded_cut_loop(dt._h, fp, Cc - 1, Cc - 1, 12, None, C.byref(o), None, 0, 3, C.byref(rec)) == gpu._lib.EINVAL
        assert "lpx_bounded_cut_loop: unknown form" in gpu._lib.last_error()
        assert np.array_equal(dt.download()[0].view(np.uint64), before.view(np.uint64))
        for a, b in zip(dt.bound_state(), state):
            assert np.array_equal(a, b)
        # bounds that belong to another live shape: the plain round reshapes without carrying them
        dt.gmi_round(flags, Cc - 1)
        assert dt.C > Cc
        for fn in (lambda: dt.gmi_round(flags, Cc - 1, bounded=True), lambda: dt.cut_loop(flags, Cc - 1, 12)):
            with pytest.raises(gpu.LpxError) as e:
                fn()
            assert "the live shape changed since lpx_tableau_set_bounds" in str(e.value)
    # a capacity the on-chip form cannot hold: refused before the first round
    T, basis, ub, _ = B.binary_bounded(128, 64, 1)
    R, Cc = T.shape
    with gpu.DeviceTableau.with_capacity(T, basis, R + 64, Cc + 64) as dt:
        dt.set_bounds(ub)
        assert gpu._lib.lib().lpx_bounded_node_fits(R, Cc) and not gpu._lib.lib().lpx_bounded_node_fits(R + 64, Cc + 64)
        with pytest.raises(gpu.LpxError) as e:
            dt.cut_loop(np.ones(Cc - 1, dtype=np.uint8), Cc - 1, 128, form="onchip")
        assert "spare capacity does not fit the on-chip form" in str(e.value)
