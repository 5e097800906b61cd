"""CPU checks of the packed batch call for integer programs (lpx_solve_packed_bnb): exported and declared, mirrored in C#, Python
and the CLI, the struct fields, sizes and offsets those of the header, ABI version unchanged, every argument error returned in its
order with its message before the device check and with the outputs untouched, no CPU fallback without a GPU, and the argument
checks of LPSolver.SolvePackedBnb.  What the kernel computes is in tests/test_gpu_packed_bnb.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_integration_files import _c_fields, _cs_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "lpx_solve_packed_bnb"


def test_symbol_exported_declared_mirrored_and_abi_version_unchanged(lpx):
    L = lpx._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(L, SYMBOL) and getattr(L, SYMBOL).argtypes is not None            # a ctypes signature in _lib.py
    assert re.search(r"\b%s\(" % SYMBOL, hdr) and (" %s(" % SYMBOL) in native and SYMBOL in guide
    assert L.lpx_abi_version() == 1 and re.search(r"#define LPX_ABI_VERSION 1\b", hdr)
    assert hasattr(lpx.LPSolver, "SolvePackedBnb") and hasattr(lpx, "PackedBnbResult") and "PackedBnbResult" in lpx.__all__
    assert issubclass(lpx.PackedBnbResult, lpx.PackedResult)
    for f in ("Status", "Solution", "OptimalValue", "Stop", "Nodes", "Info", "Log", "Logged", "Stats"):
        assert f in lpx.PackedBnbResult.__dataclass_fields__, f
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "lpx_solve_packed_bnb(" in cli and "--bnb-bounded --rhs-file" in cli
    assert "lpx_cli: --rhs-file needs --bounded and combines only with --upper / --lower / --binary" in cli      # the old message stays
    for k, name in enumerate(("DONE", "ROOT", "NODES", "NODE_ITER", "EVENTS", "DEPTH", "REFUSED")):
        assert re.search(r"#define LPX_PBNB_%s\s+%d\b" % (name, k), hdr) and getattr(lpx._lib, "PBNB_" + name) == k


def test_struct_fields_sizes_and_offsets_are_the_headers(lpx):
    models = ["count", "m", "n", "sense", "c", "A", "b", "lower", "upper", "c_stride", "A_stride", "b_stride", "lower_stride", "upper_stride",
              "is_int"]
    opts = ["search_flags", "max_iter", "max_depth", "log_cap", "max_nodes", "max_events"]
    record = ["status", "stop", "nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K", "deepest",
              "root_events", "logged", "best", "constant"]
    results = ["status", "x", "value", "rec", "log"]
    Lb = lpx._lib
    assert _c_fields("lpx_packed_bnb_models") == models == [f for f, _ in Lb.PackedBnbModels._fields_] == _cs_fields("LpxPackedBnbModels")
    assert _c_fields("lpx_packed_bnb_opts") == opts == [f for f, _ in Lb.PackedBnbOpts._fields_] == _cs_fields("LpxPackedBnbOpts")
    assert _c_fields("lpx_packed_bnb_record") == record == [f for f, _ in Lb.PackedBnbRecord._fields_] == _cs_fields("LpxPackedBnbRecord")
    assert _c_fields("lpx_packed_bnb_results") == results == [f for f, _ in Lb.PackedBnbResults._fields_] == _cs_fields("LpxPackedBnbResults")
    assert models[:14] == [f for f, _ in Lb.PackedModels._fields_]                   # lpx_packed_models is a prefix, itself unchanged
    assert C.sizeof(Lb.PackedBnbModels) == 16 + 5 * 8 + 5 * 8 + 8 and Lb.PackedBnbModels.is_int.offset == 96
    assert C.sizeof(Lb.PackedBnbOpts) == 32 and Lb.PackedBnbOpts.max_nodes.offset == 16 and Lb.PackedBnbOpts.max_events.offset == 24
    assert C.sizeof(Lb.PackedBnbRecord) == 88                                        # the size the header states
    assert "lpx_packed_bnb_record {  /* 88 bytes */" in open(os.path.join(ROOT, "include", "lpx.h")).read()
    offs = {f: getattr(Lb.PackedBnbRecord, f).offset for f in record}
    assert offs == {"status": 0, "stop": 4, "nodes": 8, "events": 16, "flips": 24, "incumbents": 32, "pruned_bound": 40,
                    "pruned_infeasible": 48, "max_K": 56, "deepest": 60, "root_events": 64, "logged": 68, "best": 72, "constant": 80}
    assert C.sizeof(Lb.PackedBnbResults) == 5 * 8 and C.sizeof(Lb.BnbNodeLog) == 32
    from linear_programming_solver_lpr381_amd import solver
    assert solver.PACKED_BNB_DTYPE.itemsize == 88 and list(solver.PACKED_BNB_DTYPE.names) == record
    assert [solver.PACKED_BNB_DTYPE.fields[f][1] for f in record] == [offs[f] for f in record]


class _Call:
    """One well-formed call of 4 models of 2 x 3, whose fields the tests spoil one at a time."""

    def __init__(self, lpx, log_cap=2):
        self.lpx = lpx
        B, m, n = 4, 2, 3
        self.arrays = {"c": np.ones((B, n)), "A": np.ones((B, m, n)), "b": np.full((B, m), 10.0), "lower": np.zeros((B, n)),
                       "upper": np.full((B, n), 4.0)}
        self.status = np.full(B, 77, dtype=np.int32); self.x = np.full((B, n), 7.5); self.value = np.full(B, 7.5)
        self.rec = np.full(B * 11, 7.5); self.log = np.full(B * log_cap * 4 + 1, 7.5)
        dp, ip = lpx._lib.dp, lpx._lib.ip
        self.pm = lpx._lib.PackedBnbModels(B, m, n, 0, *[self.arrays[k].ctypes.data_as(dp) for k in ("c", "A", "b", "lower", "upper")],
                                           n, m * n, m, n, n, None)
        self.pr = lpx._lib.PackedBnbResults(self.status.ctypes.data_as(ip), self.x.ctypes.data_as(dp), self.value.ctypes.data_as(dp),
                                            self.rec.ctypes.data_as(C.POINTER(lpx._lib.PackedBnbRecord)),
                                            self.log.ctypes.data_as(C.POINTER(lpx._lib.BnbNodeLog)) if log_cap else None)
        self.po = lpx._lib.PackedBnbOpts(0, 10000, 0, log_cap, 1000, 100000)

    def run(self, pm=True, po=True, pr=True):
        L = self.lpx._lib.lib()
        rc = L.lpx_solve_packed_bnb(C.byref(self.pm) if pm else None, C.byref(self.po) if po else None, C.byref(self.pr) if pr else None,
                                    None)
        return rc, self.lpx._lib.last_error()

    def untouched(self):
        return ((self.status == 77).all() and (self.x == 7.5).all() and (self.value == 7.5).all() and (self.rec == 7.5).all()
                and (self.log == 7.5).all())


def _refused(lpx, spoil, what, **kw):
    call = _Call(lpx)
    spoil(call)
    rc, msg = call.run(**kw)
    assert rc == lpx._lib.EINVAL, (rc, msg)
    assert msg.startswith("lpx_solve_packed_bnb: ") and what in msg, msg
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
    for f, packed in (("c_stride", 3), ("A_stride", 6), ("b_stride", 2), ("lower_stride", 3), ("upper_stride", 3)):
        for v in (packed + 1, -packed, 1):
            _refused(lpx, lambda c, f=f, v=v: setattr(c.pm, f, v), f + " is neither 0 nor the packed size %d" % packed)

    def big(c):                                         # the shape is checked, not the arrays: nothing is read
        c.pm.m, c.pm.n = 256, 512
        c.pm.c_stride, c.pm.A_stride, c.pm.b_stride, c.pm.lower_stride, c.pm.upper_stride = 512, 256 * 512, 256, 512, 512
    _refused(lpx, big, "257 x 769")
    _refused(lpx, big, "does not fit")
    _refused(lpx, lambda c: None, "null opts", po=False)
    for flags in (1, 8, 2 | 16, -1):
        _refused(lpx, lambda c, v=flags: setattr(c.po, "search_flags", v), "unknown flag")
    _refused(lpx, lambda c: setattr(c.po, "max_iter", -1), "max_iter is negative")
    for v in (0, -5):
        _refused(lpx, lambda c, v=v: setattr(c.po, "max_nodes", v), "max_nodes is below 1")
        _refused(lpx, lambda c, v=v: setattr(c.po, "max_events", v), "max_events is below 1")
    _refused(lpx, lambda c: setattr(c.po, "max_depth", -1), "max_depth is negative")
    _refused(lpx, lambda c: setattr(c.po, "log_cap", -1), "log_cap is negative")
    _refused(lpx, lambda c: setattr(c.po, "log_cap", 0), "log is given but log_cap is 0")
    _refused(lpx, lambda c: setattr(c.pr, "log", None), "log_cap is positive but log is null")

    def large(c):                                       # 65536 models of 101 x 141: 2 GB of A alone
        c.pm.count, c.pm.m, c.pm.n = 65536, 100, 40
        c.pm.c_stride, c.pm.A_stride, c.pm.b_stride, c.pm.lower_stride, c.pm.upper_stride = 40, 4000, 100, 40, 40
    _refused(lpx, large, "too large")
    # the rule counts the log (4 x 9e6 records of 32 bytes) and the work slices (a path and a stack of 2e7 entries per model)
    _refused(lpx, lambda c: (setattr(c.po, "log_cap", 9000000)), "too large")
    _refused(lpx, lambda c: (setattr(c.po, "max_depth", 20000000)), "too large")
    _refused(lpx, lambda c: (setattr(c.po, "max_depth", 2**31 - 1)), "too large")


def test_the_order_of_the_argument_errors(lpx):
    """Every defect at once, then repaired one by one from the front: each call names the first that is left."""
    call = _Call(lpx)
    pm, pr, po = call.pm, call.pr, call.po
    keep = {"c": call.arrays["c"].ctypes.data_as(lpx._lib.dp), "status": call.status.ctypes.data_as(lpx._lib.ip), "log": pr.log}
    pm.c = None; pr.status = None; pm.count = 0; pm.m = 0; pm.sense = 5; pm.c_stride = 7
    po.search_flags = 64; po.max_iter = -1; po.max_nodes = 0; po.max_events = 0; po.max_depth = -1; po.log_cap = -1
    steps = [("null c, A or b", lambda: setattr(pm, "c", keep["c"])),
             ("null status, x or value", lambda: setattr(pr, "status", keep["status"])),
             ("count is outside", lambda: setattr(pm, "count", 4)),
             ("m and n must be at least 1", lambda: setattr(pm, "m", 2)),
             ("sense", lambda: setattr(pm, "sense", 1)),
             ("c_stride is neither", lambda: setattr(pm, "c_stride", 3)),
             ("unknown flag", lambda: setattr(po, "search_flags", 6)),
             ("max_iter is negative", lambda: setattr(po, "max_iter", 0)),
             ("max_nodes is below 1", lambda: setattr(po, "max_nodes", 1)),
             ("max_events is below 1", lambda: setattr(po, "max_events", 1)),
             ("max_depth is negative", lambda: setattr(po, "max_depth", 0)),
             ("log_cap is negative", lambda: setattr(po, "log_cap", 0)),
             ("log is given but log_cap is 0", lambda: setattr(pr, "log", None)),
             ]
    for what, repair in steps:
        rc, msg = call.run()
        assert rc == lpx._lib.EINVAL and msg.startswith("lpx_solve_packed_bnb: ") and what in msg, (what, msg)
        assert call.untouched()
        repair()
    rc, msg = call.run()                                # nothing is left: the device check
    assert rc == (0 if lpx._lib.lib().lpx_device_count() > 0 else lpx._lib.EDEVICE)


def test_null_arrays_and_their_strides(lpx):
    """lower / upper NULL: their strides are not looked at, and the call gets as far as the device check."""
    call = _Call(lpx, log_cap=0)
    call.pm.lower = None
    call.pm.lower_stride = 99
    rc, msg = call.run()
    if lpx._lib.lib().lpx_device_count() > 0:
        assert rc == 0
    else:
        assert rc == lpx._lib.EDEVICE and call.untouched()


def test_no_cpu_fallback_without_a_gpu(lpx):
    """Without a device the call is LPX_EDEVICE behind its argument checks, from C and from Python; with one it runs."""
    call = _Call(lpx)
    rc, msg = call.run()
    solve = lambda: lpx.LPSolver().SolvePackedBnb(np.ones(3), np.ones((2, 3)), np.full((4, 2), 10.0), upper=1.0)
    if lpx._lib.lib().lpx_device_count() > 0:
        assert rc == 0 and (call.status >= 0).all() and solve().Status.shape == (4,)
        return
    assert rc == lpx._lib.EDEVICE and call.untouched()
    with pytest.raises(lpx.SolverException) as e:
        solve()
    assert e.value.code == lpx._lib.EDEVICE


def test_solve_packed_bnb_checks_its_arguments(lpx):
    S = lpx.LPSolver()
    c, A, b = np.ones(3), np.ones((2, 3)), np.full(2, 10.0)
    bad = [dict(c=np.ones((4, 3)), A=np.ones((5, 2, 3)), b=b, upper=1.0),              # batch axes of 4 and 5
           dict(c=c, A=A, b=np.full((4, 2), 10.0), upper=np.ones((3, 3))),
           dict(c=np.ones(4), A=A, b=b, upper=1.0),                                    # n disagrees
           dict(c=c, A=A, b=np.full(3, 10.0), upper=1.0),                              # m disagrees
           dict(c=c, A=A, b=b, upper=1.0, integer=[1, 0]),                             # one flag per variable
           dict(c=c, A=A, b=b, upper=1.0, integer=np.ones((4, 3))),                    # the mask is shared: no batch axis
           dict(c=c, A=A, b=b, upper=1.0, sense="minimise"),
           dict(c=c, A=A, b=b, upper=1.0, want=("rec", "basis")),
           dict(c=c, A=A, b=b, upper=1.0, max_nodes=0),
           dict(c=c, A=A, b=b, upper=1.0, max_events=0),
           dict(c=c, A=A, b=b, upper=1.0, max_iter=-1),
           dict(c=c, A=A, b=b, upper=1.0, max_depth=-1),
           dict(c=c, A=A, b=b, upper=1.0, log_cap=-1),
           dict(c=np.ones((0, 3)), A=A, b=b, upper=1.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            S.SolvePackedBnb(**kw)
