"""CPU checks of the branch and bound from a dual start (lpx_solve_bnb_bounded_dual, lpx_solve_packed_bnb_dual): exported and
declared, mirrored in C#, Python and the CLI, the struct's fields, size and offsets those a compiled C client sees, ABI version
unchanged, every host-side refusal returned in its order with its message before the device check and with the outputs untouched,
and no CPU fallback without a GPU.  What the kernel computes is in tests/test_gpu_packed_bnb_dual.py."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_integration_files import _c_fields, _cs_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_solve_bnb_bounded_dual", "lpx_solve_packed_bnb_dual")
PREFIX = "lpx_solve_packed_bnb_dual: "
MODELS = ["count", "m", "n", "sense", "c", "A", "b", "lower", "upper", "c_stride", "A_stride", "b_stride", "lower_stride", "upper_stride",
          "rel", "rel_stride", "is_int"]


def test_symbols_exported_declared_mirrored_and_abi_version_unchanged(lpx):
    L = lpx._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lpx.h")).read()
    native = open(os.path.join(ROOT, "integration", "csharp", "LpxNative.cs")).read()
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s          # a ctypes signature in _lib.py
        assert re.search(r"\b%s\(" % s, hdr) and (" %s(" % s) in native and s in guide, s
    assert L.lpx_abi_version() == 1 and re.search(r"#define LPX_ABI_VERSION 1\b", hdr)
    assert len(L.lpx_solve_bnb_bounded_dual.argtypes) == len(L.lpx_solve_bnb_bounded3.argtypes) == 10
    assert len(L.lpx_solve_packed_bnb_dual.argtypes) == 4
    sig = inspect.signature(lpx.LPSolver.SolveBnbBoundedDual).parameters
    assert list(sig)[1:] == ["problem", "upper", "lower", "integer", "max_nodes", "long_step", "cutoff", "node_form"]
    sig = inspect.signature(lpx.LPSolver.SolvePackedBnbDual).parameters
    assert list(sig)[1:] == ["c", "A", "b", "rel", "upper", "lower", "integer", "sense", "long_step", "cutoff", "max_nodes", "max_events",
                             "max_iter", "max_depth", "log_cap", "want"]
    assert (sig["max_nodes"].default, sig["max_events"].default, sig["want"].default) == (100000, 2000000, ("rec",))
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "--dual-root" in cli and "lpx_solve_bnb_bounded_dual(" in cli and "lpx_solve_packed_bnb_dual(" in cli
    bench = open(os.path.join(ROOT, "tools", "bench_bnb_bounded.py")).read()
    assert "--compare-packed-dual" in bench and "SolvePackedBnbDual" in bench


def test_struct_fields_are_the_headers_and_the_neighbours_are_unchanged(lpx):
    Lb = lpx._lib
    assert _c_fields("lpx_packed_bnb_dual_models") == MODELS == [f for f, _ in Lb.PackedBnbDualModels._fields_] == _cs_fields("LpxPackedBnbDualModels")
    assert MODELS[:16] == [f for f, _ in Lb.PackedDualModels._fields_] == _c_fields("lpx_packed_dual_models")      # a prefix, itself unchanged
    assert _c_fields("lpx_packed_bnb_models") == MODELS[:14] + ["is_int"]
    assert C.sizeof(Lb.PackedBnbDualModels) == 16 + 5 * 8 + 5 * 8 + 8 + 8 + 8
    assert (Lb.PackedBnbDualModels.rel.offset, Lb.PackedBnbDualModels.rel_stride.offset, Lb.PackedBnbDualModels.is_int.offset) == (96, 104, 112)
    assert C.sizeof(Lb.PackedBnbModels) == 104 and C.sizeof(Lb.PackedDualModels) == 112 and C.sizeof(Lb.PackedBnbOpts) == 32
    assert C.sizeof(Lb.PackedBnbRecord) == 88 and C.sizeof(Lb.PackedBnbResults) == 40


def test_size_and_offsets_match_a_compiled_c_client(lpx, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler for the client"
    src = tmp_path / "client.c"
    fields = "".join('    printf("%s %%zu\\n", offsetof(lpx_packed_bnb_dual_models, %s));\n' % (f, f) for f in MODELS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lpx.h"\nint main(void)\n{\n'
                   '    printf("sizeof %zu\\n", sizeof(lpx_packed_bnb_dual_models));\n' + fields +
                   '    printf("abi %d\\n", LPX_ABI_VERSION);\n'
                   '    int (*f)(const lpx_packed_bnb_dual_models*, const lpx_packed_bnb_opts*, const lpx_packed_bnb_results*, lpx_stats*) = '
                   'lpx_solve_packed_bnb_dual;\n'
                   '    int (*g)(const lpx_problem*, const double*, const double*, const uint8_t*, const lpx_solve_opts*, int64_t, int, int, '
                   'lpx_result*, lpx_bnb_bounded_info*) = lpx_solve_bnb_bounded_dual;\n'
                   '    return f == 0 || g == 0;\n}\n')
    exe = tmp_path / "client"
    pkg = os.path.dirname(lpx.__file__)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", pkg, "-llpx",
                    "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    T = lpx._lib.PackedBnbDualModels
    assert int(out["sizeof"]) == C.sizeof(T) and int(out["abi"]) == 1
    for f in MODELS:
        assert int(out[f]) == getattr(T, f).offset, f


class _Call:
    """One well-formed call of 4 models of 2 x 3, whose fields the tests spoil one at a time."""

    def __init__(self, lpx, log_cap=2):
        self.lpx = lpx
        B, m, n = 4, 2, 3
        self.arrays = {"c": np.ones((B, n)), "A": np.ones((B, m, n)), "b": np.full((B, m), 2.0), "lower": np.zeros((B, n)),
                       "upper": np.full((B, n), 4.0)}
        self.rel = np.tile(np.array([0, 1], dtype=np.int32), (B, 1))
        self.status = np.full(B, 77, dtype=np.int32); self.x = np.full((B, n), 7.5); self.value = np.full(B, 7.5)
        self.rec = np.full(B * 11, 7.5); self.log = np.full(B * log_cap * 4 + 1, 7.5)
        dp, ip = lpx._lib.dp, lpx._lib.ip
        self.pm = lpx._lib.PackedBnbDualModels(B, m, n, 0, *[self.arrays[k].ctypes.data_as(dp) for k in ("c", "A", "b", "lower", "upper")],
                                               n, m * n, m, n, n, self.rel.ctypes.data_as(ip), m, None)
        self.pr = lpx._lib.PackedBnbResults(self.status.ctypes.data_as(ip), self.x.ctypes.data_as(dp), self.value.ctypes.data_as(dp),
                                            self.rec.ctypes.data_as(C.POINTER(lpx._lib.PackedBnbRecord)),
                                            self.log.ctypes.data_as(C.POINTER(lpx._lib.BnbNodeLog)) if log_cap else None)
        self.po = lpx._lib.PackedBnbOpts(0, 10000, 0, log_cap, 1000, 100000)

    def run(self, pm=True, po=True, pr=True):
        L = self.lpx._lib.lib()
        rc = L.lpx_solve_packed_bnb_dual(C.byref(self.pm) if pm else None, C.byref(self.po) if po else None,
                                         C.byref(self.pr) if pr else None, None)
        return rc, self.lpx._lib.last_error()

    def untouched(self):
        return ((self.status == 77).all() and (self.x == 7.5).all() and (self.value == 7.5).all() and (self.rec == 7.5).all()
                and (self.log == 7.5).all())


def _refused(lpx, spoil, what, **kw):
    call = _Call(lpx)
    spoil(call)
    rc, msg = call.run(**kw)
    assert rc == lpx._lib.EINVAL, (rc, msg)
    assert msg.startswith(PREFIX) and what in msg, msg
    assert call.untouched()


def _share_rel(c, values):
    c.shared = np.array(values, dtype=np.int32)
    c.pm.rel, c.pm.rel_stride = c.shared.ctypes.data_as(c.lpx._lib.ip), 0


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
    for values, i in (([0, 2], 1), ([3, 1], 0), ([-1, 0], 0)):                      # a shared rel is read on the host
        _refused(lpx, lambda c, v=values: _share_rel(c, v), "rel[%d] is neither LPX_LE nor LPX_GE" % i)
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
        c.pm.c_stride, c.pm.A_stride, c.pm.b_stride, c.pm.lower_stride, c.pm.upper_stride, c.pm.rel_stride = 40, 4000, 100, 40, 40, 100
    _refused(lpx, large, "too large")
    _refused(lpx, lambda c: (setattr(c.po, "log_cap", 9000000)), "too large")
    _refused(lpx, lambda c: (setattr(c.po, "max_depth", 20000000)), "too large")


def test_the_one_gib_rule_counts_rel(lpx):
    """Two calls that differ in rel alone, around the limit: c, A, b and the bounds shared, 65536 models of 139 x 1, so rel is
    36 MB of a total the rule reports; without rel the total it reports is 65536 * 4 * 139 bytes smaller."""
    def shape(c, with_rel):
        c.pm.count, c.pm.m, c.pm.n = 65536, 139, 1
        c.pm.c_stride = c.pm.A_stride = c.pm.b_stride = c.pm.lower_stride = c.pm.upper_stride = 0
        c.pm.rel_stride = 139
        if not with_rel:
            c.pm.rel = None
        c.po.log_cap = 500; c.po.max_depth = 1
    totals = []
    for with_rel in (True, False):
        call = _Call(lpx)
        shape(call, with_rel)
        rc, msg = call.run()
        assert rc == lpx._lib.EINVAL and msg.startswith(PREFIX + "too large: ") and call.untouched(), msg
        totals.append(int(msg[len(PREFIX + "too large: "):].split()[0]))
    assert totals[0] - totals[1] == 65536 * 4 * 139


def test_the_order_of_the_argument_errors(lpx):
    """Every defect at once, then repaired one by one from the front: each call names the first that is left."""
    call = _Call(lpx)
    pm, pr, po = call.pm, call.pr, call.po
    keep = {"c": call.arrays["c"].ctypes.data_as(lpx._lib.dp), "status": call.status.ctypes.data_as(lpx._lib.ip)}
    bad_rel = np.array([0, 2], dtype=np.int32)
    good_rel = np.array([0, 1], dtype=np.int32)
    pm.c = None; pr.status = None; pm.count = 0; pm.m = 0; pm.sense = 5; pm.c_stride = 7; pm.rel_stride = 5
    pm.rel = bad_rel.ctypes.data_as(lpx._lib.ip)
    po.search_flags = 64; po.max_iter = -1; po.max_nodes = 0; po.max_events = 0; po.max_depth = -1; po.log_cap = -1
    steps = [("null c, A or b", lambda: setattr(pm, "c", keep["c"])),
             ("null status, x or value", lambda: setattr(pr, "status", keep["status"])),
             ("count is outside", lambda: setattr(pm, "count", 4)),
             ("m and n must be at least 1", lambda: setattr(pm, "m", 2)),
             ("sense", lambda: setattr(pm, "sense", 1)),
             ("c_stride is neither", lambda: setattr(pm, "c_stride", 3)),
             ("rel_stride is neither", lambda: setattr(pm, "rel_stride", 0)),
             ("rel[1] is neither LPX_LE nor LPX_GE", lambda: setattr(pm, "rel", good_rel.ctypes.data_as(lpx._lib.ip))),   # behind the fit rule, before the options
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
        assert rc == lpx._lib.EINVAL and msg.startswith(PREFIX) and what in msg, (what, msg)
        assert call.untouched()
        repair()
    rc, msg = call.run()                                # nothing is left: the device check
    assert rc == (0 if lpx._lib.lib().lpx_device_count() > 0 else lpx._lib.EDEVICE)
    # the fit rule comes in front of the shared rel
    call = _Call(lpx)
    call.pm.m, call.pm.n = 256, 512
    call.pm.c_stride, call.pm.A_stride, call.pm.b_stride, call.pm.lower_stride, call.pm.upper_stride = 512, 256 * 512, 256, 512, 512
    call.pm.rel, call.pm.rel_stride = bad_rel.ctypes.data_as(lpx._lib.ip), 0
    rc, msg = call.run()
    assert rc == lpx._lib.EINVAL and "does not fit" in msg


def test_no_cpu_fallback_without_a_gpu(lpx):
    """Without a device both calls are LPX_EDEVICE behind their argument checks, from C and from Python; with one they run."""
    call = _Call(lpx)
    rc, msg = call.run()
    S = lpx.LPSolver()
    packed = lambda: S.SolvePackedBnbDual(np.ones(3), np.ones((2, 3)), np.full((4, 2), 2.0), ["<=", ">="], upper=1.0)
    p = lpx.LPProblem.from_arrays(1, [1.0, 2.0, 3.0], np.ones((2, 3)), [1, 0], [2.0, 2.5])
    single = lambda: S.SolveBnbBoundedDual(p, np.ones(3), node_form="onchip")
    if lpx._lib.lib().lpx_device_count() > 0:
        assert rc == 0 and (call.status >= 0).all() and packed().Status.shape == (4,) and single().Status == 0
        return
    assert rc == lpx._lib.EDEVICE and call.untouched()
    for f in (packed, single):
        with pytest.raises(lpx.SolverException) as e:
            f()
        assert e.value.code == lpx._lib.EDEVICE


def _driver(lpx, c, A, rel, b, upper, lower=None, is_int=None, sense=0, max_nodes=0, flags=0, node_form=1):
    """lpx_solve_bnb_bounded_dual through ctypes: (rc, message)."""
    from linear_programming_solver_lpr381_amd import solver
    Lb = lpx._lib
    ps, hold = solver._problem_struct(lpx.LPProblem.from_arrays(sense, c, A, rel, b))
    o, keep = solver._solve_opts({})
    vec = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
    lo, up = vec(lower), vec(upper)
    mask = None if is_int is None else np.ascontiguousarray(is_int, dtype=np.uint8)
    r, info = Lb.Result(), Lb.BnbBoundedInfo()
    rc = Lb.lib().lpx_solve_bnb_bounded_dual(C.byref(ps), None if lo is None else lo.ctypes.data_as(Lb.dp), up.ctypes.data_as(Lb.dp),
                                             None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(o), max_nodes, flags,
                                             node_form, C.byref(r), C.byref(info))
    msg = Lb.last_error() if rc else ""
    if rc == 0:
        Lb.lib().lpx_result_free(C.byref(r)); Lb.lib().lpx_bnb_bounded_info_free(C.byref(info))
    return rc, msg


def test_the_host_driver_refuses_in_its_order_without_a_device(lpx):
    """ValidateBnbBounded first (bounds, then the integer variables, max_nodes, search_flags), then node_form, then the preparation:
    every defect at once, repaired from the front."""
    E = lpx._lib.EINVAL
    c, A, rel, b = [1.0, 2.0, 3.0], np.ones((2, 3)), [1, 0], [2.0, 2.5]
    mask = [0, 1, 1]
    # x1 is continuous, improves a Max objective and has no upper bound: the precheck of the preparation, last in the order
    args = dict(upper=[np.inf, 0.5, 1.0], lower=[0.0, 1.0, 0.0], is_int=mask, sense=0, max_nodes=-1, flags=64, node_form=7)
    steps = [("upper bound of x2 is below its lower bound", dict(lower=[0.0, 0.0, 0.0])),
             ("integer variable x2 needs finite, integral lower and upper bounds", dict(upper=[np.inf, 1.0, 1.0])),
             ("max_nodes is negative", dict(max_nodes=0)),
             ("search_flags holds a bit other than", dict(flags=6)),
             ("node_form is none of LPX_NODE_LAUNCHES, LPX_NODE_ONCHIP and LPX_NODE_AUTO", dict(node_form=1)),
             ("x1 improves the objective and has no upper bound", dict(upper=[5.0, 1.0, 1.0]))]
    for what, repair in steps:
        rc, msg = _driver(lpx, c, A, rel, b, **args)
        assert rc == E and msg.startswith("Bounded ") and what in msg, (what, rc, msg)      # the drivers' own messages, as lpx_solve_bnb_bounded3
        args.update(repair)
    assert "Bounded Dual Simplex: x1 improves" in msg   # SolveBoundedDual's own message
    rc, msg = _driver(lpx, c, A, rel, b, **args)        # nothing is left: the device check
    assert rc == (0 if lpx._lib.lib().lpx_device_count() > 0 else lpx._lib.EDEVICE), msg
    rc, msg = _driver(lpx, c, A, rel, b, upper=[np.inf, 1.0, 1.0], is_int=None)       # an integer variable always has an upper bound
    assert rc == E and "integer variable x1 needs finite" in msg
    rc, msg = _driver(lpx, c, A, rel, b, upper=[1.0, 1.0, 1.0], node_form=-1)         # -1 is no form of this call
    assert rc == E and "node_form" in msg
    # null arguments
    assert lpx._lib.lib().lpx_solve_bnb_bounded_dual(None, None, None, None, None, 0, 0, 1, None, None) == E
    assert lpx._lib.last_error() == "lpx_solve_bnb_bounded_dual: null argument"


def test_python_methods_check_their_arguments(lpx):
    S = lpx.LPSolver()
    c, A, b = np.ones(3), np.ones((2, 3)), np.full(2, 2.0)
    bad = [dict(c=c, A=A, b=b, rel=["<=", "="], upper=1.0),                            # an = row is passed as its pair
           dict(c=c, A=A, b=b, rel=[0, 1, 0], upper=1.0),                              # one entry per row
           dict(c=c, A=A, b=b, rel=np.zeros((4, 3), dtype=np.int32), upper=1.0),
           dict(c=c, A=A, b=b, rel=[0.0, 1.0], upper=1.0),
           dict(c=c, A=A, b=b, rel=None, upper=1.0, integer=[1, 0]),
           dict(c=c, A=A, b=b, rel=None, upper=1.0, sense="minimise"),
           dict(c=c, A=A, b=b, rel=None, upper=1.0, want=("rec", "basis")),
           dict(c=c, A=A, b=b, rel=None, upper=1.0, max_nodes=0),
           dict(c=c, A=A, b=b, rel=None, upper=1.0, max_events=0),
           dict(c=c, A=A, b=b, rel=None, upper=1.0, max_iter=-1),
           dict(c=c, A=A, b=b, rel=None, upper=1.0, max_depth=-1),
           dict(c=c, A=A, b=b, rel=None, upper=1.0, log_cap=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            S.SolvePackedBnbDual(**kw)
    p = lpx.LPProblem.from_arrays(1, [1.0, 2.0, 3.0], np.ones((2, 3)), [1, 0], [2.0, 2.5])
    with pytest.raises(ValueError):
        S.SolveBnbBoundedDual(p, np.ones(3), node_form="fast")
    assert inspect.signature(S.SolvePackedBnb) == inspect.signature(lpx.LPSolver().SolvePackedBnb)      # the neighbour keeps its signature
    assert "rel" not in inspect.signature(lpx.LPSolver.SolvePackedBnb).parameters


def test_cli_refuses_what_dual_root_does_not_combine_with(lpx):
    exe = os.path.join(os.path.dirname(lpx.__file__), "lpx_cli")

    def run(*args):
        return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
    assert "--dual-root" in run("--help").stdout
    what = "--dual-root needs --bnb-bounded and combines only with"
    for extra in (("--divers", "2"), ("--plunge", "2"), ("--branching", "strong"), ("--stall-events", "5"), ("--tighten",), ("--iterations",),
                  ("--bounded-dual",), ("--bounded",), ("--rhs-file", "r.txt", "--node-form", "onchip")):
        r = run("--binary", "--bnb-bounded", "--dual-root", *extra, "x.txt")
        assert r.returncode == 64 and what in r.stderr, extra
    r = run("--binary", "--dual-root", "x.txt")
    assert r.returncode == 64 and what in r.stderr
    for extra in ((), ("--long-step", "--cutoff"), ("--node-form", "onchip"), ("--upper", "1=1"), ("--rhs-file", "r.txt")):
        r = run("--binary", "--bnb-bounded", "--dual-root", *extra, "no_such_file.txt")   # accepted: it gets as far as the input file
        assert r.returncode == 66, (extra, r.stderr)
    r = run("--binary", "--bnb-bounded", "--divers", "4", "--rhs-file", "r.txt", "x.txt")  # the neighbour's message stays
    assert r.returncode == 64 and "--bnb-bounded --rhs-file combines only with" in r.stderr
