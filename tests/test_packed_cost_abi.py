"""CPU checks of lpx_packed_base_solve_costs: exported and declared, mirrored in C#, Python and the CLI, the structs those of the
header (a 72-byte record), ABI version unchanged, every argument error returned in its order with its message before the device
check and with the outputs untouched, and no CPU fallback without a GPU.  What the kernel computes is in
tests/test_gpu_packed_cost.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_integration_files import _c_fields, _cs_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "lpx_packed_base_solve_costs"
PREFIX = SYMBOL + ": "


def test_symbol_exported_declared_mirrored_and_abi_version_unchanged(lpx):
    L = lpx._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert hasattr(L, SYMBOL) and getattr(L, SYMBOL).argtypes is not None      # a ctypes signature in _lib.py
    assert re.search(r"\b%s\(" % SYMBOL, hdr) and (" %s(" % SYMBOL) in native and SYMBOL in guide and (SYMBOL + "(") in cli
    assert L.lpx_abi_version() == 1 and re.search(r"#define LPX_ABI_VERSION 1\b", hdr)
    assert hasattr(lpx.PackedBase, "solve_costs") and hasattr(lpx, "PackedCostResult") and "PackedCostResult" in lpx.__all__
    fields = set(lpx.PackedCostResult.__dataclass_fields__)
    assert {"PrimalEvents", "DualEvents", "PrimalCounts", "DualCounts", "Duals", "ReducedCosts", "Z", "Basis", "AtUpper", "Stats"} <= fields
    assert not fields & {"Passes", "DualizeFlips", "BoundCounts"}
    assert "--cost-file" in cli
    assert "Per-scenario bounds or costs are not offered" not in hdr
    for old in ("lpx_cli: --warm-base needs --bounded-dual --rhs-file",            # the old messages stay
                "lpx_cli: --bounded-dual needs --rhs-file and combines only with --long-step and --upper / --lower / --binary"):
        assert old in cli


def test_struct_fields_sizes_and_offsets_are_the_headers(lpx):
    Lb = lpx._lib
    record = ["status", "primal_events", "dual_events", "pad", "primal_kind0", "primal_kind1", "primal_flips", "dual_kind0", "dual_kind1",
              "dual_passes", "z"]
    assert _c_fields("lpx_packed_cost_record") == record == [f for f, _ in Lb.PackedCostRecord._fields_] == _cs_fields("LpxPackedCostRecord")
    assert C.sizeof(Lb.PackedCostRecord) == 72
    assert [getattr(Lb.PackedCostRecord, f).offset for f in record] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64]
    assert lpx.solver.PACKED_COST_DTYPE.itemsize == 72 and list(lpx.solver.PACKED_COST_DTYPE.names) == record
    assert [lpx.solver.PACKED_COST_DTYPE.fields[f][1] for f in record] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64]
    results = ["status", "x", "value", "rec", "basis", "at_upper", "y", "d"]
    assert _c_fields("lpx_packed_cost_results") == results == [f for f, _ in Lb.PackedCostResults._fields_] == _cs_fields("LpxPackedCostResults")
    assert C.sizeof(Lb.PackedCostResults) == 64
    assert [getattr(Lb.PackedCostResults, f).offset for f in results] == [0, 8, 16, 24, 32, 40, 48, 56]
    assert C.sizeof(Lb.PackedDualResults) == 64 and C.sizeof(Lb.PackedDualRecord) == 48        # the existing structs, unchanged


class _Call:
    """One well-formed lpx_packed_base_solve_costs of 4 scenarios.  Its argument checks read nothing through the handle but the
    shape, so without a device (where no handle can be opened) a zeroed stand-in of ample size serves for them."""

    def __init__(self, lpx, handle=None):
        self.lpx = lpx
        B, m, n = 4, 2, 3
        self.standin = (C.c_char * 4096)()
        self.h = handle if handle is not None else C.cast(self.standin, C.c_void_p)
        self.count = B
        self.c = np.ones((B, n)); self.b = np.full((B, m), 2.0)
        self.status = np.full(B, 77, dtype=np.int32); self.x = np.full((B, n), 7.5); self.value = np.full(B, 7.5)
        self.y = np.full((B, m), 7.5); self.d = np.full((B, n), 7.5)
        dp, ip = lpx._lib.dp, lpx._lib.ip
        self.cp = self.c.ctypes.data_as(dp); self.bp = self.b.ctypes.data_as(dp)
        self.pr = lpx._lib.PackedCostResults(self.status.ctypes.data_as(ip), self.x.ctypes.data_as(dp), self.value.ctypes.data_as(dp),
                                             None, None, None, self.y.ctypes.data_as(dp), self.d.ctypes.data_as(dp))
        self.op = lpx._lib.default_opts(False); self.od = lpx._lib.default_opts(True)
        self.flags = lpx._lib.BDUAL_LONG_STEP

    def run(self, h=True, pr=True, op=True, od=True):
        L = self.lpx._lib.lib()
        rc = L.lpx_packed_base_solve_costs(self.h if h else None, self.count, self.cp, self.bp, self.flags,
                                           C.byref(self.op) if op else None, C.byref(self.od) if od else None,
                                           C.byref(self.pr) if pr else None, None)
        return rc, self.lpx._lib.last_error()

    def untouched(self):
        return ((self.status == 77).all() and (self.x == 7.5).all() and (self.value == 7.5).all() and (self.y == 7.5).all()
                and (self.d == 7.5).all())


def _refused(lpx, spoil, what, **kw):
    call = _Call(lpx)
    spoil(call)
    rc, msg = call.run(**kw)
    assert rc == lpx._lib.EINVAL, (rc, msg)
    assert msg.startswith(PREFIX) and what in msg, msg
    assert call.untouched()


def test_argument_errors_come_first(lpx):
    _refused(lpx, lambda c: None, "null argument", h=False)
    _refused(lpx, lambda c: setattr(c, "cp", None), "null argument")
    _refused(lpx, lambda c: None, "null argument", pr=False)
    for f in ("status", "x", "value"):
        _refused(lpx, lambda c, f=f: setattr(c.pr, f, None), "null status, x or value")
    for count in (0, -1, 65537):
        _refused(lpx, lambda c, v=count: setattr(c, "count", v), "count is outside [1, 65536]")
    for flags in (lpx._lib.BDUAL_CUTOFF, lpx._lib.BDUAL_LONG_STEP | lpx._lib.BDUAL_CUTOFF, 1, 8, -1):
        _refused(lpx, lambda c, v=flags: setattr(c, "flags", v), "unknown flag")
    _refused(lpx, lambda c: setattr(c.op, "resident", 1), "resident")
    _refused(lpx, lambda c: setattr(c.od, "resident", 1), "resident")
    _refused(lpx, lambda c: setattr(c.od, "resident", 1), "resident", op=False)    # either structure alone


def test_the_order_of_the_errors(lpx):
    """Every defect at once, then repaired one by one from the front: each call names the first that is left."""
    call = _Call(lpx)
    keep = {"cp": call.cp, "status": call.status.ctypes.data_as(lpx._lib.ip)}
    call.cp = None; call.pr.status = None; call.count = 0; call.flags = 64; call.op.resident = 1; call.od.resident = 1
    steps = [("null argument", lambda: setattr(call, "cp", keep["cp"])),
             ("null status, x or value", lambda: setattr(call.pr, "status", keep["status"])),
             ("count is outside", lambda: setattr(call, "count", 4)),
             ("unknown flag", lambda: setattr(call, "flags", 0)),
             ("resident", lambda: setattr(call.op, "resident", 0)),
             ("resident", lambda: setattr(call.od, "resident", 0))]
    for what, repair in steps:
        rc, msg = call.run()
        assert rc == lpx._lib.EINVAL and msg.startswith(PREFIX) and what in msg, (what, msg)
        assert call.untouched()
        repair()


def _opened(lpx):
    return lpx.LPSolver().OpenPackedBase(np.ones(3), np.ones((2, 3)), np.full(2, 2.0), rel=[">=", "<="], upper=4.0, sense="min")


def test_more_than_a_gibibyte_is_refused(lpx):
    """The rule counts c0, c, b and every output asked for with the handle's shape; it needs a real handle, so a device: without
    one this test only sees LPX_EDEVICE from the open, and the run of the whole suite on a GPU (this file is not marked gpu and runs
    there too) is what covers the size rule and its place behind the other refusals."""
    if lpx._lib.lib().lpx_device_count() == 0:
        with pytest.raises(lpx.SolverException) as e:
            _opened(lpx)
        assert e.value.code == lpx._lib.EDEVICE
        return
    g = np.random.default_rng(0)
    with lpx.LPSolver().OpenPackedBase(np.ones(1200), g.integers(1, 9, size=(4, 1200)).astype(np.float64), np.full(4, 50.0),
                                       rel=[">="] * 4, upper=1.0, sense="min") as base:
        call = _Call(lpx, base._h)
        call.count = 65536                              # 65536 x 1200 doubles of c alone: the arrays are never read
        rc, msg = call.run()
        assert rc == lpx._lib.EINVAL and msg.startswith(PREFIX) and "too large" in msg and call.untouched()


def test_no_cpu_fallback_without_a_gpu(lpx):
    """Without a device no base can be opened, and a call that passes its argument checks is LPX_EDEVICE with the outputs
    untouched; with one it runs, with and without b and with NULL options."""
    if lpx._lib.lib().lpx_device_count() > 0:
        with _opened(lpx) as base:
            call = _Call(lpx, base._h)
            rc, msg = call.run(op=False, od=False)
            assert rc == 0 and (call.status == 0).all(), msg
            res = base.solve_costs(np.ones((4, 3)))
            assert res.Status.tolist() == [0] * 4 and not res.DualEvents.any() and res.Stats["launches"] == 1
            assert base.solve_costs(np.ones(3), np.full((5, 2), 2.0)).Status.shape == (5,)
        return
    call = _Call(lpx)
    rc, msg = call.run()
    assert rc == lpx._lib.EDEVICE and call.untouched()
    with pytest.raises(lpx.SolverException) as e:
        _opened(lpx)
    assert e.value.code == lpx._lib.EDEVICE


def test_solve_costs_checks_its_shapes(lpx):
    """The Python layer refuses shapes before the library is asked; a stand-in object carries the shape without a device."""
    base = lpx.PackedBase.__new__(lpx.PackedBase)
    base._h, base.m, base.n, base._max_iter = C.c_void_p(1), 2, 3, None
    try:
        bad = [dict(c=np.ones(4)), dict(c=np.ones((2, 4))), dict(c=np.ones((2, 2, 3))), dict(c=np.ones((0, 3))),
               dict(c=np.ones(3), b=np.ones(3)), dict(c=np.ones((2, 3)), b=np.ones((3, 2))), dict(c=np.ones(3), b=np.ones((2, 2, 2)))]
        for kw in bad:
            with pytest.raises(ValueError):
                base.solve_costs(**kw)
        base._h = None
        with pytest.raises(lpx.SolverException):
            base.solve_costs(np.ones(3))
    finally:
        base._h = None                                  # nothing to close
