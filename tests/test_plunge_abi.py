"""CPU checks of the entry points of the plunge (lpx_node_batch_plunge, lpx_solve_bnb_bounded5, lpx_bnb_plunge_info_free):
exported and declared, mirrored in C# and Python, argument errors before device errors with their messages, the Python-level
errors, and no CPU fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_node_batch_plunge", "lpx_solve_bnb_bounded5", "lpx_bnb_plunge_info_free")


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
        assert getattr(L, s).argtypes is not None, s          # a ctypes signature in _lib.py
        assert re.search(r"\b%s\(" % s, hdr), s
        assert (" %s(" % s) in native, s
    assert "struct LpxBnbPlungeInfo" in native and "lpx_bnb_plunge_info" in hdr
    assert L.lpx_abi_version() == 1
    assert hasattr(lpx.NodeBatch, "plunge") and hasattr(lpx._lib, "BnbPlungeInfo")
    assert C.sizeof(lpx._lib.BnbPlungeInfo) == 32 and C.sizeof(lpx._lib.NodeRecord) == 64
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "--plunge" in cli and "lpx_solve_bnb_bounded5(" in cli
    bench = open(os.path.join(ROOT, "tools", "bench_bnb_bounded.py")).read()
    assert "--plunge" in bench and "--compare-plunge" in bench


def test_plunge_argument_errors_come_first(lpx):
    """Checked before any device is looked for: the same answers with and without a GPU."""
    L = lpx._lib.lib()
    EINVAL, ip, dp = lpx._lib.EINVAL, lpx._lib.ip, lpx._lib.dp
    slot = np.zeros(2, dtype=np.int32); K = np.zeros(2, dtype=np.int32); rc = np.zeros(2, dtype=np.int32)
    steps = np.zeros(2, dtype=np.int32)
    recs = (lpx._lib.NodeRecord * 8)()
    cut = np.array([0.0, float("nan")])
    prune = np.array([-np.inf, 1.0]); bad_prune = np.array([0.0, float("nan")])
    depth = np.array([1, 4], dtype=np.int32)
    sp, kp, rp, cp, tp = (slot.ctypes.data_as(ip), K.ctypes.data_as(ip), rc.ctypes.data_as(ip), cut.ctypes.data_as(dp),
                          steps.ctypes.data_as(ip))
    pp, dpp = prune.ctypes.data_as(dp), depth.ctypes.data_as(ip)

    def run(batch=None, B=1, slot=sp, K=kp, flags=1, cutoff=None, prune=pp, depth=dpp, D=4, out=recs, steps=tp, rc=rp):
        return L.lpx_node_batch_plunge(batch, B, slot, K, None, None, None, None, flags, cutoff, prune, depth, D, 0, None, 1e-6,
                                       out, steps, rc)

    def err():
        return lpx._lib.last_error()

    assert run() == EINVAL and "lpx_node_batch_plunge: null batch" in err()
    for name in ("out", "rc", "K", "slot", "depth", "steps", "prune"):
        assert run(**{name: None}) == EINVAL and "lpx_node_batch_plunge: null " + name in err(), name
    for B in (0, -1):
        assert run(B=B) == EINVAL and "lpx_node_batch_plunge: B is outside [1, W]" in err()
    for D in (0, 65, -2):
        assert run(D=D) == EINVAL and "lpx_node_batch_plunge: D is outside [1, 64]" in err()
    for flags in (8, 16, -1):
        assert run(flags=flags) == EINVAL and "lpx_node_batch_plunge: unknown flag" in err()
    assert run(B=2, flags=1 | 4, cutoff=cp) == EINVAL and "lpx_node_batch_plunge: entry 1: cutoff is NaN" in err()
    assert run(B=2, flags=1 | 4) == EINVAL and "null cutoff" in err()
    assert run(B=2, flags=1, cutoff=cp) == EINVAL and "null batch" in err()          # not read without the flag
    assert run(B=2, D=3) == EINVAL and "lpx_node_batch_plunge: entry 1: depth is outside [1, D]" in err()
    zero = np.array([0, 1], dtype=np.int32)
    assert run(B=1, depth=zero.ctypes.data_as(ip)) == EINVAL and "lpx_node_batch_plunge: entry 0: depth is outside [1, D]" in err()
    assert run(B=2, prune=bad_prune.ctypes.data_as(dp)) == EINVAL and "lpx_node_batch_plunge: entry 1: prune is NaN" in err()
    assert run(B=1, prune=bad_prune.ctypes.data_as(dp)) == EINVAL and "null batch" in err()     # entry 1 is not read with B = 1
    L.lpx_bnb_plunge_info_free(None)


def test_python_level_errors(lpx):
    nb = object.__new__(lpx.NodeBatch)          # no handles are needed to reach the checks
    nb._handles, nb._W, nb._h = [], 2, None
    with pytest.raises(ValueError, match=r"B must be in \[1, W\]"):
        nb.plunge([0, 1, 2], [([], [], [])] * 3, 4, 2, 2, -np.inf)
    with pytest.raises(ValueError, match="3 slots but 2 nodes"):
        nb.plunge([0, 1, 2], [([], [], [])] * 2, 4, 2, 2, -np.inf)
    for D in (0, 65):
        with pytest.raises(ValueError, match=r"D must be in \[1, 64\]"):
            nb.plunge([0], [([], [], [])], 4, 1, D, -np.inf)
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    with pytest.raises(ValueError, match="launches"):
        lpx.LPSolver().SolveBnbBounded(prob, [4, 3, 3], plunge=4, node_form="launches")
    with pytest.raises(ValueError, match="launches"):
        lpx.LPSolver().SolveBnbBounded(prob, [4, 3, 3], divers=2, plunge=4, node_form="launches")
    for D in (0, 65):
        with pytest.raises(lpx.SolverException) as e:
            lpx.LPSolver().SolveBnbBounded(prob, [4, 3, 3], plunge=D)               # plunge alone means divers = 1
        assert e.value.code == lpx._lib.EINVAL and "plunge is outside [1, 64]" in str(e.value)
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().SolveBnbBounded(prob, [4, 3, 3], divers=0, plunge=2)
    assert e.value.code == lpx._lib.EINVAL and "divers is outside" in str(e.value)


def test_driver_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r, info, dinfo, pinfo = lpx._lib.Result(), lpx._lib.BnbBoundedInfo(), lpx._lib.BnbDiversInfo(), lpx._lib.BnbPlungeInfo()
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)

    def solve(max_nodes=0, flags=0, divers=4, plunge=4, out=C.byref(r)):
        return L.lpx_solve_bnb_bounded5(C.byref(p), None, upp, None, None, max_nodes, flags, divers, plunge, out, C.byref(info),
                                        C.byref(dinfo), C.byref(pinfo))

    for W in (0, 1025, -3):
        assert solve(divers=W) == EINVAL and "lpx_solve_bnb_bounded5: divers is outside [1, 1024]" in lpx._lib.last_error()
    for D in (0, 65, -3):
        assert solve(plunge=D) == EINVAL and "lpx_solve_bnb_bounded5: plunge is outside [1, 64]" in lpx._lib.last_error()
    for flags in (1, 8, 2 | 16):
        assert solve(flags=flags) == EINVAL and "search_flags" in lpx._lib.last_error()
    assert solve(max_nodes=-1) == EINVAL and "max_nodes is negative" in lpx._lib.last_error()
    assert solve(out=None) == EINVAL and "lpx_solve_bnb_bounded5: null argument" in lpx._lib.last_error()
    frac = np.array([4.0, 2.5, 3.0])
    rc = L.lpx_solve_bnb_bounded5(C.byref(p), None, frac.ctypes.data_as(lpx._lib.dp), None, None, 0, 0, 2, 2, C.byref(r), None, None, None)
    assert rc == EINVAL and "needs finite, integral lower and upper bounds" in lpx._lib.last_error()


def test_no_cpu_fallback(lpx):
    """Without a device the driver is LPX_EDEVICE; with one it solves."""
    L = lpx._lib.lib()
    p, hold = _problem(lpx)
    r, info, dinfo, pinfo = lpx._lib.Result(), lpx._lib.BnbBoundedInfo(), lpx._lib.BnbDiversInfo(), lpx._lib.BnbPlungeInfo()
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)
    rc = L.lpx_solve_bnb_bounded5(C.byref(p), None, upp, None, None, 0, 0, 4, 4, C.byref(r), C.byref(info), C.byref(dinfo),
                                  C.byref(pinfo))
    if L.lpx_device_count() > 0:
        assert rc == 0 and info.nodes >= 1 and dinfo.rounds >= 1 and pinfo.launched >= info.nodes
        L.lpx_bnb_bounded_info_free(C.byref(info)); L.lpx_bnb_divers_info_free(C.byref(dinfo)); L.lpx_bnb_plunge_info_free(C.byref(pinfo))
        L.lpx_result_free(C.byref(r))
    else:
        assert rc == lpx._lib.EDEVICE and "no HIP device" in lpx._lib.last_error()
