"""CPU checks of the packed batch call (lpx_packed_fits, lpx_solve_packed): exported and declared, mirrored in C#, Python and the
CLI, the struct fields those of the header, ABI version unchanged, the fit rule at its edges, every argument error returned with
its message before the device check and with the outputs untouched, no CPU fallback without a GPU, and the shape checks of
LPSolver.SolvePacked.  What the kernel computes is in tests/test_gpu_packed.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_integration_files import _c_fields, _cs_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_packed_fits", "lpx_solve_packed")


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
    assert hasattr(lpx.LPSolver, "SolvePacked") and hasattr(lpx, "PackedResult")
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "--rhs-file" in cli and "lpx_solve_packed(" in cli


def test_struct_fields_are_the_headers(lpx):
    models = ["count", "m", "n", "sense", "c", "A", "b", "lower", "upper", "c_stride", "A_stride", "b_stride", "lower_stride", "upper_stride"]
    results = ["status", "x", "value", "rec", "basis", "at_upper"]
    assert _c_fields("lpx_packed_models") == models == [f for f, _ in lpx._lib.PackedModels._fields_] == _cs_fields("LpxPackedModels")
    assert _c_fields("lpx_packed_results") == results == [f for f, _ in lpx._lib.PackedResults._fields_] == _cs_fields("LpxPackedResults")
    assert C.sizeof(lpx._lib.PackedModels) == 16 + 5 * 8 + 5 * 8 and C.sizeof(lpx._lib.PackedResults) == 6 * 8


def test_fit_rule_at_its_edges(lpx):
    fits, node = lpx._lib.lib().lpx_packed_fits, lpx._lib.lib().lpx_bounded_node_fits
    assert fits(139, 1) == 1 and fits(140, 1) == 0 and fits(15, 1100) == 1 and fits(256, 512) == 0 and fits(0, 3) == 0
    assert fits(3, 0) == 0 and fits(-1, -1) == 0 and fits(1, 1) == 1 and fits(2 ** 31 - 1, 2 ** 31 - 1) == 0
    for m, n in ((1, 1), (6, 12), (12, 60), (139, 1), (140, 1), (9, 1827), (9, 1828), (100, 20)):
        assert fits(m, n) == node(m + 1, n + m + 1)


class _Call:
    """One well-formed call of 4 models of 2 x 3, whose fields the tests spoil one at a time."""

    def __init__(self, lpx):
        self.lpx = lpx
        B, m, n = 4, 2, 3
        self.arrays = {"c": np.ones((B, n)), "A": np.ones((B, m, n)), "b": np.full((B, m), 10.0), "lower": np.zeros((B, n)),
                       "upper": np.full((B, n), 4.0)}
        self.status = np.full(B, 77, dtype=np.int32); self.x = np.full((B, n), 7.5); self.value = np.full(B, 7.5)
        dp, ip = lpx._lib.dp, lpx._lib.ip
        self.pm = lpx._lib.PackedModels(B, m, n, 0, *[self.arrays[k].ctypes.data_as(dp) for k in ("c", "A", "b", "lower", "upper")],
                                        n, m * n, m, n, n)
        self.pr = lpx._lib.PackedResults(self.status.ctypes.data_as(ip), self.x.ctypes.data_as(dp), self.value.ctypes.data_as(dp),
                                         None, None, None)
        self.o = lpx._lib.default_opts(False)

    def run(self, pm=True, pr=True):
        L = self.lpx._lib.lib()
        rc = L.lpx_solve_packed(C.byref(self.pm) if pm else None, C.byref(self.o), C.byref(self.pr) if pr else None, None)
        return rc, self.lpx._lib.last_error()

    def untouched(self):
        return (self.status == 77).all() and (self.x == 7.5).all() and (self.value == 7.5).all()


def _refused(lpx, spoil, what, **kw):
    call = _Call(lpx)
    spoil(call)
    rc, msg = call.run(**kw)
    assert rc == lpx._lib.EINVAL, (rc, msg)
    assert msg.startswith("lpx_solve_packed: ") and what in msg, msg
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
    _refused(lpx, lambda c: setattr(c.o, "resident", 1), "resident")

    def large(c):                                       # 65536 models of 13 x 73: 1.8 GB of A alone
        c.pm.count, c.pm.m, c.pm.n = 65536, 100, 40
        c.pm.c_stride, c.pm.A_stride, c.pm.b_stride, c.pm.lower_stride, c.pm.upper_stride = 40, 4000, 100, 40, 40
    _refused(lpx, large, "too large")


def test_a_stride_of_a_null_bound_array_is_not_read(lpx):
    """lower / upper NULL: their strides are not looked at, and the call gets as far as the device check."""
    call = _Call(lpx)
    call.pm.lower = None; call.pm.upper = None
    call.pm.lower_stride = 99; call.pm.upper_stride = -5
    rc, msg = call.run()
    if lpx._lib.lib().lpx_device_count() > 0:
        assert rc == 0
    else:
        assert rc == lpx._lib.EDEVICE and call.untouched()


def test_no_cpu_fallback_without_a_gpu(lpx):
    if lpx._lib.lib().lpx_device_count() > 0:
        pytest.skip("a GPU is visible")
    call = _Call(lpx)
    rc, msg = call.run()
    assert rc == lpx._lib.EDEVICE and call.untouched()
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().SolvePacked(np.ones(3), np.ones((2, 3)), np.full((4, 2), 10.0), upper=1.0)
    assert e.value.code == lpx._lib.EDEVICE


def test_solve_packed_checks_its_shapes(lpx):
    S = lpx.LPSolver()
    c, A, b = np.ones(3), np.ones((2, 3)), np.full(2, 10.0)
    bad = [dict(c=np.ones((4, 3)), A=np.ones((5, 2, 3)), b=b),                      # batch axes of 4 and 5
           dict(c=c, A=A, b=np.full((4, 2), 10.0), upper=np.ones((3, 3))),
           dict(c=c, A=A, b=np.full((4, 2), 10.0), lower=np.zeros((2, 3))),
           dict(c=np.ones(4), A=A, b=b),                                            # n disagrees
           dict(c=c, A=A, b=np.full(3, 10.0)),                                      # m disagrees
           dict(c=c, A=A, b=b, upper=np.ones(2)),
           dict(c=c, A=np.ones(3), b=b),
           dict(c=c, A=A, b=b, sense="maximise"),
           dict(c=c, A=A, b=b, want=("rec", "tableau")),
           dict(c=np.ones((0, 3)), A=A, b=b)]
    for kw in bad:
        with pytest.raises(ValueError):
            S.SolvePacked(**kw)
