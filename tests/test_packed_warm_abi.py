"""CPU checks of the packed calls from a solved base (lpx_packed_base_open / _solve / _close): exported and declared, mirrored in
C#, Python and the CLI, the struct fields those of the header, ABI version unchanged, every argument error of open and of solve
returned in its order with its message before the device check and with the outputs untouched, close(NULL), and no CPU fallback
without a GPU.  What the kernels compute is in tests/test_gpu_packed_warm.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_integration_files import _c_fields, _cs_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_packed_base_open", "lpx_packed_base_solve", "lpx_packed_base_close")


def test_symbols_exported_declared_mirrored_and_abi_version_unchanged(lpx):
    L = lpx._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    for s in SYMBOLS:
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s            # a ctypes signature in _lib.py
        assert re.search(r"\b%s\(" % s, hdr) and (" %s(" % s) in native and s in guide and (s + "(") in cli, s
    assert "typedef struct lpx_packed_base lpx_packed_base;" in hdr                  # opaque
    assert L.lpx_abi_version() == 1 and re.search(r"#define LPX_ABI_VERSION 1\b", hdr)
    assert hasattr(lpx.LPSolver, "OpenPackedBase") and hasattr(lpx, "PackedBase") and "PackedBase" in lpx.__all__
    for f in ("solve", "close", "__enter__", "__exit__"):
        assert hasattr(lpx.PackedBase, f), f
    assert "--warm-base" in cli
    for old in ("lpx_cli: --rhs-file needs --bounded and combines only with --upper / --lower / --binary",      # the old messages stay
                "lpx_cli: --bounded-dual needs --rhs-file and combines only with --long-step and --upper / --lower / --binary"):
        assert old in cli


def test_struct_fields_are_the_headers(lpx):
    model = ["m", "n", "sense", "c", "A", "b", "lower", "upper", "rel"]
    Lb = lpx._lib
    assert _c_fields("lpx_packed_base_model") == model == [f for f, _ in Lb.PackedBaseModel._fields_] == _cs_fields("LpxPackedBaseModel")
    assert C.sizeof(Lb.PackedBaseModel) == 16 + 6 * 8
    results = ["status", "x", "value", "rec", "basis", "at_upper", "y", "d"]      # the structs of lpx_solve_packed_dual, unchanged
    assert _c_fields("lpx_packed_dual_results") == results and C.sizeof(Lb.PackedDualResults) == 64 and C.sizeof(Lb.PackedDualRecord) == 48


class _Open:
    """One well-formed lpx_packed_base_open of a 2 x 3 model, whose fields the tests spoil one at a time."""

    def __init__(self, lpx):
        self.lpx = lpx
        m, n = 2, 3
        self.arrays = {"c": np.ones(n), "A": np.ones((m, n)), "b": np.full(m, 2.0), "lower": np.zeros(n), "upper": np.full(n, 4.0)}
        self.rel = np.array([0, 1], dtype=np.int32)
        self.status = np.full(1, 77, dtype=np.int32); self.x = np.full(n, 7.5); self.value = np.full(1, 7.5)
        self.y = np.full(m, 7.5); self.d = np.full(n, 7.5)
        dp, ip = lpx._lib.dp, lpx._lib.ip
        self.pm = lpx._lib.PackedBaseModel(m, n, 0, *[self.arrays[k].ctypes.data_as(dp) for k in ("c", "A", "b", "lower", "upper")],
                                           self.rel.ctypes.data_as(ip))
        self.pr = lpx._lib.PackedDualResults(self.status.ctypes.data_as(ip), self.x.ctypes.data_as(dp), self.value.ctypes.data_as(dp),
                                             None, None, None, self.y.ctypes.data_as(dp), self.d.ctypes.data_as(dp))
        self.o = lpx._lib.default_opts(True)
        self.flags = lpx._lib.BDUAL_LONG_STEP
        self.h = C.c_void_p(12345)                      # set to NULL by every refused call that is given it

    def run(self, pm=True, pr=True, h=True):
        L = self.lpx._lib.lib()
        rc = L.lpx_packed_base_open(C.byref(self.pm) if pm else None, self.flags, C.byref(self.o), C.byref(self.pr) if pr else None,
                                    C.byref(self.h) if h else None)
        return rc, self.lpx._lib.last_error()

    def untouched(self):
        return ((self.status == 77).all() and (self.x == 7.5).all() and (self.value == 7.5).all() and (self.y == 7.5).all()
                and (self.d == 7.5).all())


def _open_refused(lpx, spoil, what, **kw):
    call = _Open(lpx)
    spoil(call)
    rc, msg = call.run(**kw)
    assert rc == lpx._lib.EINVAL, (rc, msg)
    assert msg.startswith("lpx_packed_base_open: ") and what in msg, msg
    assert call.untouched()
    if kw.get("h", True):
        assert call.h.value is None                     # *h = NULL


def test_open_argument_errors_come_first(lpx):
    """Those of lpx_solve_packed_dual for one model whose arrays are all shared; the same answers with and without a GPU."""
    _open_refused(lpx, lambda c: None, "null argument", pm=False)
    _open_refused(lpx, lambda c: None, "null argument", h=False)
    for f in ("c", "A", "b"):
        _open_refused(lpx, lambda c, f=f: setattr(c.pm, f, None), "null c, A or b")
    for f in ("status", "x", "value"):
        _open_refused(lpx, lambda c, f=f: setattr(c.pr, f, None), "null status, x or value")
    for f in ("m", "n"):
        for v in (0, -2):
            _open_refused(lpx, lambda c, f=f, v=v: setattr(c.pm, f, v), "m and n must be at least 1")
    for sense in (2, -1):
        _open_refused(lpx, lambda c, v=sense: setattr(c.pm, "sense", v), "sense")

    def big(c):                                         # the shape is checked, not the arrays: nothing is read
        c.pm.m, c.pm.n = 256, 512
        c.pm.rel = None
    _open_refused(lpx, big, "257 x 769")
    _open_refused(lpx, big, "does not fit")
    _open_refused(lpx, lambda c: setattr(c.o, "resident", 1), "resident")
    for v in (2, -1, 7):
        _open_refused(lpx, lambda c, v=v: c.rel.__setitem__(1, v), "rel[1] is neither LPX_LE nor LPX_GE")
    for flags in (lpx._lib.BDUAL_CUTOFF, lpx._lib.BDUAL_LONG_STEP | lpx._lib.BDUAL_CUTOFF, 1, 8, -1):
        _open_refused(lpx, lambda c, v=flags: setattr(c, "flags", v), "unknown flag")


def test_the_order_of_the_open_errors(lpx):
    """Every defect at once, then repaired one by one from the front: each call names the first that is left."""
    call = _Open(lpx)
    pm, pr = call.pm, call.pr
    keep = {"c": call.arrays["c"].ctypes.data_as(lpx._lib.dp), "status": call.status.ctypes.data_as(lpx._lib.ip)}
    pm.c = None; pr.status = None; pm.m = 0; pm.sense = 5
    call.o.resident = 1; call.flags = 64; call.rel[1] = 2
    steps = [("null c, A or b", lambda: setattr(pm, "c", keep["c"])),
             ("null status, x or value", lambda: setattr(pr, "status", keep["status"])),
             ("m and n must be at least 1", lambda: setattr(pm, "m", 2)),
             ("sense", lambda: setattr(pm, "sense", 1)),
             ("resident", lambda: setattr(call.o, "resident", 0)),
             ("rel[1] is neither", lambda: call.rel.__setitem__(1, 1)),
             ("unknown flag", lambda: setattr(call, "flags", 0))]
    for what, repair in steps:
        rc, msg = call.run()
        assert rc == lpx._lib.EINVAL and msg.startswith("lpx_packed_base_open: ") and what in msg, (what, msg)
        assert call.untouched() and call.h.value is None
        call.h = C.c_void_p(12345)
        repair()
    rc, msg = call.run()                                # nothing is left: the device check
    if lpx._lib.lib().lpx_device_count() > 0:
        assert rc == 0 and call.h.value is not None
        assert lpx._lib.lib().lpx_packed_base_close(call.h) == 0
    else:
        assert rc == lpx._lib.EDEVICE and call.h.value is None and call.untouched()


def test_open_without_base_out_and_without_optional_arrays(lpx):
    """base_out = NULL and lower / upper / rel NULL are accepted: the call gets as far as the device check."""
    call = _Open(lpx)
    call.pm.lower = None; call.pm.rel = None; call.pm.sense = 1        # Min 1.x over x >= 0: dual feasible without an upper bound
    call.pm.upper = None
    rc, msg = call.run(pr=False)
    if lpx._lib.lib().lpx_device_count() > 0:
        assert rc == 0 and call.h.value is not None, msg
        assert lpx._lib.lib().lpx_packed_base_close(call.h) == 0
    else:
        assert rc == lpx._lib.EDEVICE and call.h.value is None
    assert call.untouched()


class _Solve:
    """One well-formed lpx_packed_base_solve of 4 right-hand sides.  Its argument checks read nothing through the handle but the
    shape, so without a device (where no handle can be opened) a zeroed stand-in of ample size serves for them."""

    def __init__(self, lpx, handle=None):
        self.lpx = lpx
        B, m, n = 4, 2, 3
        self.standin = (C.c_char * 4096)()
        self.h = handle if handle is not None else C.cast(self.standin, C.c_void_p)
        self.count = B
        self.b = np.full((B, m), 2.0)
        self.status = np.full(B, 77, dtype=np.int32); self.x = np.full((B, n), 7.5); self.value = np.full(B, 7.5)
        self.y = np.full((B, m), 7.5); self.d = np.full((B, n), 7.5)
        dp, ip = lpx._lib.dp, lpx._lib.ip
        self.bp = self.b.ctypes.data_as(dp)
        self.pr = lpx._lib.PackedDualResults(self.status.ctypes.data_as(ip), self.x.ctypes.data_as(dp), self.value.ctypes.data_as(dp),
                                             None, None, None, self.y.ctypes.data_as(dp), self.d.ctypes.data_as(dp))
        self.o = lpx._lib.default_opts(True)
        self.flags = lpx._lib.BDUAL_LONG_STEP

    def run(self, h=True, pr=True):
        L = self.lpx._lib.lib()
        rc = L.lpx_packed_base_solve(self.h if h else None, self.count, self.bp, self.flags, C.byref(self.o),
                                     C.byref(self.pr) if pr else None, None)
        return rc, self.lpx._lib.last_error()

    def untouched(self):
        return ((self.status == 77).all() and (self.x == 7.5).all() and (self.value == 7.5).all() and (self.y == 7.5).all()
                and (self.d == 7.5).all())


def _solve_refused(lpx, spoil, what, **kw):
    call = _Solve(lpx)
    spoil(call)
    rc, msg = call.run(**kw)
    assert rc == lpx._lib.EINVAL, (rc, msg)
    assert msg.startswith("lpx_packed_base_solve: ") and what in msg, msg
    assert call.untouched()


def test_solve_argument_errors_come_first(lpx):
    _solve_refused(lpx, lambda c: None, "null argument", h=False)
    _solve_refused(lpx, lambda c: setattr(c, "bp", None), "null argument")
    _solve_refused(lpx, lambda c: None, "null argument", pr=False)
    for f in ("status", "x", "value"):
        _solve_refused(lpx, lambda c, f=f: setattr(c.pr, f, None), "null status, x or value")
    for count in (0, -1, 65537):
        _solve_refused(lpx, lambda c, v=count: setattr(c, "count", v), "count is outside [1, 65536]")
    for flags in (lpx._lib.BDUAL_CUTOFF, lpx._lib.BDUAL_LONG_STEP | lpx._lib.BDUAL_CUTOFF, 1, 8, -1):
        _solve_refused(lpx, lambda c, v=flags: setattr(c, "flags", v), "unknown flag")
    _solve_refused(lpx, lambda c: setattr(c.o, "resident", 1), "resident")


def test_the_order_of_the_solve_errors(lpx):
    call = _Solve(lpx)
    keep = {"bp": call.bp, "status": call.status.ctypes.data_as(lpx._lib.ip)}
    call.bp = None; call.pr.status = None; call.count = 0; call.flags = 64; call.o.resident = 1
    steps = [("null argument", lambda: setattr(call, "bp", keep["bp"])),
             ("null status, x or value", lambda: setattr(call.pr, "status", keep["status"])),
             ("count is outside", lambda: setattr(call, "count", 4)),
             ("unknown flag", lambda: setattr(call, "flags", 0)),
             ("resident", lambda: setattr(call.o, "resident", 0))]
    for what, repair in steps:
        rc, msg = call.run()
        assert rc == lpx._lib.EINVAL and msg.startswith("lpx_packed_base_solve: ") and what in msg, (what, msg)
        assert call.untouched()
        repair()


def test_solve_refuses_more_than_a_gibibyte(lpx):
    """The rule counts b and every output asked for with the handle's shape; it needs a real handle, so a device."""
    if lpx._lib.lib().lpx_device_count() == 0:
        with pytest.raises(lpx.SolverException) as e:
            lpx.LPSolver().OpenPackedBase(np.ones(3), np.ones((2, 3)), np.full(2, 2.0), rel=[">=", "<="], upper=4.0, sense="min")
        assert e.value.code == lpx._lib.EDEVICE
        return
    g = np.random.default_rng(0)
    with lpx.LPSolver().OpenPackedBase(np.ones(1200), g.integers(1, 9, size=(4, 1200)).astype(np.float64), np.full(4, 50.0),
                                       rel=[">="] * 4, upper=1.0, sense="min") as base:
        call = _Solve(lpx, base._h)
        call.count = 65536                              # 65536 x 1200 doubles of x alone: the arrays are never read
        rc, msg = call.run()
        assert rc == lpx._lib.EINVAL and msg.startswith("lpx_packed_base_solve: ") and "too large" in msg and call.untouched()


def test_close_null_is_allowed(lpx):
    assert lpx._lib.lib().lpx_packed_base_close(None) == 0


def test_no_cpu_fallback_without_a_gpu(lpx):
    """Without a device open is LPX_EDEVICE behind its argument checks, from C and from Python; with one it runs."""
    call = _Open(lpx)
    call.pm.sense = 1
    rc, msg = call.run()
    opened = lambda: lpx.LPSolver().OpenPackedBase(np.ones(3), np.ones((2, 3)), np.full(2, 2.0), rel=["<=", ">="], upper=4.0, sense="min")
    if lpx._lib.lib().lpx_device_count() > 0:
        assert rc == 0 and call.status[0] == 0 and call.h.value is not None
        sv = _Solve(lpx, call.h)
        rc, msg = sv.run()
        assert rc == 0 and (sv.status == 0).all(), msg
        assert lpx._lib.lib().lpx_packed_base_close(call.h) == 0
        with opened() as base:
            assert base.Base.Status.tolist() == [0] and base.solve(np.full((4, 2), 2.0)).Status.shape == (4,)
        return
    assert rc == lpx._lib.EDEVICE and call.untouched() and call.h.value is None
    with pytest.raises(lpx.SolverException) as e:
        opened()
    assert e.value.code == lpx._lib.EDEVICE


def test_open_packed_base_checks_its_shapes(lpx):
    S = lpx.LPSolver()
    c, A, b = np.ones(3), np.ones((2, 3)), np.full(2, 2.0)
    bad = [dict(c=np.ones((4, 3)), A=A, b=b),                                       # a batch axis: the base is one model
           dict(c=c, A=np.ones((4, 2, 3)), b=b),
           dict(c=c, A=A, b=np.full((4, 2), 2.0)),
           dict(c=c, A=A, b=b, upper=np.ones((4, 3))),
           dict(c=c, A=A, b=b, rel=np.zeros((4, 2), dtype=np.int32)),
           dict(c=np.ones(4), A=A, b=b),                                            # n disagrees
           dict(c=c, A=A, b=np.full(3, 2.0)),                                       # m disagrees
           dict(c=c, A=A, b=b, rel=["<=", "="]),                                    # an = row is passed as its pair
           dict(c=c, A=A, b=b, sense="minimise")]
    for kw in bad:
        with pytest.raises(ValueError):
            S.OpenPackedBase(**kw)
