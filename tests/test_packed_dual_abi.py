"""CPU checks of the packed batch call by a dual start (lpx_solve_packed_dual): exported and declared, mirrored in C#, Python and
the CLI, the struct fields those of the header, ABI version unchanged, every argument error returned in its order with its message
before the device check and with the outputs untouched, no CPU fallback without a GPU, and the shape and rel checks of
LPSolver.SolvePackedDual.  What the kernel computes is in tests/test_gpu_packed_dual.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_integration_files import _c_fields, _cs_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "lpx_solve_packed_dual"


def test_symbol_exported_declared_mirrored_and_abi_version_unchanged(lpx):
    L = lpx._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(L, SYMBOL) and getattr(L, SYMBOL).argtypes is not None            # a ctypes signature in _lib.py
    assert re.search(r"\b%s\(" % SYMBOL, hdr) and (" %s(" % SYMBOL) in native and SYMBOL in guide
    assert L.lpx_abi_version() == 1 and re.search(r"#define LPX_ABI_VERSION 1\b", hdr)
    assert hasattr(lpx.LPSolver, "SolvePackedDual") and hasattr(lpx, "PackedDualResult") and "PackedDualResult" in lpx.__all__
    for f in ("Duals", "ReducedCosts", "Passes", "DualizeFlips", "Status", "Solution", "OptimalValue", "Basis", "AtUpper", "Stats"):
        assert f in lpx.PackedDualResult.__dataclass_fields__, f
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "--bounded-dual" in cli and "lpx_solve_packed_dual(" in cli
    assert "lpx_cli: --rhs-file needs --bounded and combines only with --upper / --lower / --binary" in cli      # the old message stays


def test_struct_fields_are_the_headers(lpx):
    models = ["count", "m", "n", "sense", "c", "A", "b", "lower", "upper", "c_stride", "A_stride", "b_stride", "lower_stride", "upper_stride",
              "rel", "rel_stride"]
    record = ["status", "events", "kind0", "kind1", "passes", "dualize_flips", "z"]
    results = ["status", "x", "value", "rec", "basis", "at_upper", "y", "d"]
    Lb = lpx._lib
    assert _c_fields("lpx_packed_dual_models") == models == [f for f, _ in Lb.PackedDualModels._fields_] == _cs_fields("LpxPackedDualModels")
    assert _c_fields("lpx_packed_dual_record") == record == [f for f, _ in Lb.PackedDualRecord._fields_] == _cs_fields("LpxPackedDualRecord")
    assert _c_fields("lpx_packed_dual_results") == results == [f for f, _ in Lb.PackedDualResults._fields_] == _cs_fields("LpxPackedDualResults")
    assert C.sizeof(Lb.PackedDualModels) == 16 + 5 * 8 + 5 * 8 + 8 + 8 and C.sizeof(Lb.PackedDualRecord) == 48
    assert C.sizeof(Lb.PackedDualResults) == 8 * 8
    assert models[:14] == [f for f, _ in Lb.PackedModels._fields_]                   # lpx_packed_models is a prefix, itself unchanged


class _Call:
    """One well-formed call of 4 models of 2 x 3, whose fields the tests spoil one at a time."""

    def __init__(self, lpx):
        self.lpx = lpx
        B, m, n = 4, 2, 3
        self.arrays = {"c": np.ones((B, n)), "A": np.ones((B, m, n)), "b": np.full((B, m), 10.0), "lower": np.zeros((B, n)),
                       "upper": np.full((B, n), 4.0)}
        self.rel = np.tile(np.array([0, 1], dtype=np.int32), (B, 1))
        self.status = np.full(B, 77, dtype=np.int32); self.x = np.full((B, n), 7.5); self.value = np.full(B, 7.5)
        self.y = np.full((B, m), 7.5); self.d = np.full((B, n), 7.5)
        dp, ip = lpx._lib.dp, lpx._lib.ip
        self.pm = lpx._lib.PackedDualModels(B, m, n, 0, *[self.arrays[k].ctypes.data_as(dp) for k in ("c", "A", "b", "lower", "upper")],
                                            n, m * n, m, n, n, self.rel.ctypes.data_as(ip), m)
        self.pr = lpx._lib.PackedDualResults(self.status.ctypes.data_as(ip), self.x.ctypes.data_as(dp), self.value.ctypes.data_as(dp),
                                             None, None, None, self.y.ctypes.data_as(dp), self.d.ctypes.data_as(dp))
        self.o = lpx._lib.default_opts(True)
        self.flags = lpx._lib.BDUAL_LONG_STEP

    def run(self, pm=True, pr=True):
        L = self.lpx._lib.lib()
        rc = L.lpx_solve_packed_dual(C.byref(self.pm) if pm else None, self.flags, C.byref(self.o), C.byref(self.pr) if pr else None, None)
        return rc, self.lpx._lib.last_error()

    def untouched(self):
        return ((self.status == 77).all() and (self.x == 7.5).all() and (self.value == 7.5).all() and (self.y == 7.5).all()
                and (self.d == 7.5).all())


def _refused(lpx, spoil, what, **kw):
    call = _Call(lpx)
    spoil(call)
    rc, msg = call.run(**kw)
    assert rc == lpx._lib.EINVAL, (rc, msg)
    assert msg.startswith("lpx_solve_packed_dual: ") and what in msg, msg
    assert call.untouched()


def test_argument_errors_come_first(lpx):
    """Checked before any device is looked for: the same answers with and without a GPU."""
    _refused(lpx, lambda c: None, "null argument", pm=False)
    _refused(lpx, lambda c: None, "null argument", pr=False)
    for f in ("c", "A", "b"):
        _refused(lpx, lambda c, f=f: setattr(c.pm, f, None), "null c, A or b")
    for f in ("status", "x", "value"):
        _refused(lpx, lambda c, f=f: setattr(c.pr, f, None), "null status, x or value")
    for count in (0, -1, 65537):
        _refused(lpx, lambda c, v=count: setattr(c.pm, "count", v), "count is outside [1, 65536]")
    for f in ("m", "n"):
        for v in (0, -2):
            _refused(lpx, lambda c, f=f, v=v: setattr(c.pm, f, v), "m and n must be at least 1")
    for sense in (2, -1):
        _refused(lpx, lambda c, v=sense: setattr(c.pm, "sense", v), "sense")
    for f, packed in (("c_stride", 3), ("A_stride", 6), ("b_stride", 2), ("lower_stride", 3), ("upper_stride", 3), ("rel_stride", 2)):
        for v in (packed + 1, -packed, 1):
            _refused(lpx, lambda c, f=f, v=v: setattr(c.pm, f, v), f + " is neither 0 nor the packed size %d" % packed)

    def big(c):                                         # the shape is checked, not the arrays: nothing is read
        c.pm.m, c.pm.n = 256, 512
        c.pm.c_stride, c.pm.A_stride, c.pm.b_stride, c.pm.lower_stride, c.pm.upper_stride, c.pm.rel_stride = 512, 256 * 512, 256, 512, 512, 256
    _refused(lpx, big, "257 x 769")
    _refused(lpx, big, "does not fit")
    _refused(lpx, lambda c: setattr(c.o, "resident", 1), "resident")

    def large(c):                                       # 65536 models of 101 x 141: 2 GB of A alone
        c.pm.count, c.pm.m, c.pm.n = 65536, 100, 40
        c.pm.c_stride, c.pm.A_stride, c.pm.b_stride, c.pm.lower_stride, c.pm.upper_stride, c.pm.rel_stride = 40, 4000, 100, 40, 40, 100
    _refused(lpx, large, "too large")

    def shared_rel(c, v):                               # a shared rel is read on the host: m entries
        c.rel[0, 1] = v
        c.pm.rel_stride = 0
    for v in (2, -1, 7):
        _refused(lpx, lambda c, v=v: shared_rel(c, v), "rel[1] is neither LPX_LE nor LPX_GE")
    for flags in (lpx._lib.BDUAL_CUTOFF, lpx._lib.BDUAL_LONG_STEP | lpx._lib.BDUAL_CUTOFF, 1, 8, -1):
        _refused(lpx, lambda c, v=flags: setattr(c, "flags", v), "unknown flag")


def test_the_order_of_the_argument_errors(lpx):
    """Every defect at once, then repaired one by one from the front: each call names the first that is left."""
    call = _Call(lpx)
    pm, pr = call.pm, call.pr
    keep = {"c": call.arrays["c"].ctypes.data_as(lpx._lib.dp), "status": call.status.ctypes.data_as(lpx._lib.ip)}
    pm.c = None; pr.status = None; pm.count = 0; pm.m = 0; pm.sense = 5; pm.c_stride = 7; pm.rel_stride = 9
    call.o.resident = 1; call.flags = 64
    steps = [("null c, A or b", lambda: setattr(pm, "c", keep["c"])),
             ("null status, x or value", lambda: setattr(pr, "status", keep["status"])),
             ("count is outside", lambda: setattr(pm, "count", 4)),
             ("m and n must be at least 1", lambda: setattr(pm, "m", 2)),
             ("sense", lambda: setattr(pm, "sense", 1)),
             ("c_stride is neither", lambda: setattr(pm, "c_stride", 3)),
             ("rel_stride is neither", lambda: setattr(pm, "rel_stride", 0)),
             ("resident", lambda: setattr(call.o, "resident", 0)),
             ("rel[1] is neither", lambda: call.rel.__setitem__((0, 1), 1)),
             ("unknown flag", lambda: setattr(call, "flags", 0))]
    call.rel[0, 1] = 2
    for what, repair in steps:
        rc, msg = call.run()
        assert rc == lpx._lib.EINVAL and msg.startswith("lpx_solve_packed_dual: ") and what in msg, (what, msg)
        assert call.untouched()
        repair()
    rc, msg = call.run()                                # nothing is left: the device check
    assert rc == (0 if lpx._lib.lib().lpx_device_count() > 0 else lpx._lib.EDEVICE)


def test_a_per_model_rel_is_not_looked_at_on_the_host(lpx):
    """rel_stride = m: a bad entry is that model's own LPX_EINVAL, found by its workgroup; the call gets as far as the device."""
    call = _Call(lpx)
    call.rel[2, 0] = 2
    rc, msg = call.run()
    if lpx._lib.lib().lpx_device_count() > 0:
        assert rc == 0 and call.status.tolist()[2] == lpx._lib.EINVAL and (call.status[[0, 1, 3]] >= 0).all()
    else:
        assert rc == lpx._lib.EDEVICE and call.untouched()


def test_null_arrays_and_their_strides(lpx):
    """lower / upper / rel NULL: their strides are not looked at, and the call gets as far as the device check."""
    call = _Call(lpx)
    call.pm.lower = None; call.pm.rel = None
    call.pm.lower_stride = 99; call.pm.rel_stride = -5
    rc, msg = call.run()
    if lpx._lib.lib().lpx_device_count() > 0:
        assert rc == 0
    else:
        assert rc == lpx._lib.EDEVICE and call.untouched()


def test_no_cpu_fallback_without_a_gpu(lpx):
    """Without a device the call is LPX_EDEVICE behind its argument checks, from C and from Python; with one it runs."""
    call = _Call(lpx)
    rc, msg = call.run()
    solve = lambda: lpx.LPSolver().SolvePackedDual(np.ones(3), np.ones((2, 3)), np.full((4, 2), 10.0), rel=[">=", "<="], upper=1.0)
    if lpx._lib.lib().lpx_device_count() > 0:
        assert rc == 0 and (call.status >= 0).all() and solve().Status.shape == (4,)
        return
    assert rc == lpx._lib.EDEVICE and call.untouched()
    with pytest.raises(lpx.SolverException) as e:
        solve()
    assert e.value.code == lpx._lib.EDEVICE


def test_solve_packed_dual_checks_its_shapes_and_rel(lpx):
    S = lpx.LPSolver()
    c, A, b = np.ones(3), np.ones((2, 3)), np.full(2, 10.0)
    bad = [dict(c=np.ones((4, 3)), A=np.ones((5, 2, 3)), b=b),                      # batch axes of 4 and 5
           dict(c=c, A=A, b=np.full((4, 2), 10.0), upper=np.ones((3, 3))),
           dict(c=c, A=A, b=np.full((4, 2), 10.0), rel=np.zeros((3, 2), dtype=np.int32)),
           dict(c=np.ones(4), A=A, b=b),                                            # n disagrees
           dict(c=c, A=A, b=np.full(3, 10.0)),                                      # m disagrees
           dict(c=c, A=A, b=b, rel=[0, 1, 0]),                                      # m entries per row of rel
           dict(c=c, A=A, b=b, rel=np.zeros((2, 2, 2), dtype=np.int32)),
           dict(c=c, A=A, b=b, rel=["<=", "="]),                                    # an = row is passed as its pair
           dict(c=c, A=A, b=b, rel=["<=", "=>"]),
           dict(c=c, A=A, b=b, rel=[0.0, 1.0]),                                     # neither ints nor strings
           dict(c=c, A=A, b=b, sense="minimise"),
           dict(c=c, A=A, b=b, want=("rec", "tableau")),
           dict(c=np.ones((0, 3)), A=A, b=b)]
    for kw in bad:
        with pytest.raises(ValueError):
            S.SolvePackedDual(**kw)
