"""CPU checks of the entry points of the node batch and of the search by divers (lpx_tableau_clone, lpx_node_batch_create /
_destroy / _run, lpx_solve_bnb_bounded4, lpx_bnb_divers_info_free): exported and declared, mirrored in C# and Python, argument
errors before device errors with their messages, and no CPU fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_tableau_clone", "lpx_node_batch_create", "lpx_node_batch_destroy", "lpx_node_batch_run", "lpx_solve_bnb_bounded4",
           "lpx_bnb_divers_info_free")


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
    assert L.lpx_abi_version() == 1
    assert hasattr(lpx.DeviceTableau, "clone") and hasattr(lpx, "NodeBatch") and hasattr(lpx.NodeBatch, "run")
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "--divers" in cli and "lpx_solve_bnb_bounded4(" in cli
    bench = open(os.path.join(ROOT, "tools", "bench_bnb_bounded.py")).read()
    assert "--divers" in bench and "--compare-divers" in bench


def test_batch_argument_errors_come_first(lpx):
    """Checked before any device is looked for: the same answers with and without a GPU."""
    L = lpx._lib.lib()
    EINVAL, ip, dp = lpx._lib.EINVAL, lpx._lib.ip, lpx._lib.dp
    slot = np.zeros(2, dtype=np.int32); K = np.zeros(2, dtype=np.int32); rc = np.zeros(2, dtype=np.int32)
    recs = (lpx._lib.NodeRecord * 2)()
    cut = np.array([0.0, float("nan")])
    sp, kp, rp, cp = slot.ctypes.data_as(ip), K.ctypes.data_as(ip), rc.ctypes.data_as(ip), cut.ctypes.data_as(dp)

    def run(batch=None, B=1, slot=sp, K=kp, flags=1, cutoff=None, out=recs, rc=rp):
        return L.lpx_node_batch_run(batch, B, slot, K, None, None, None, None, flags, cutoff, 0, None, 1e-6, out, rc)

    assert run() == EINVAL and "lpx_node_batch_run: null batch" in lpx._lib.last_error()
    assert run(out=None) == EINVAL and "lpx_node_batch_run: null out" in lpx._lib.last_error()
    assert run(rc=None) == EINVAL and "lpx_node_batch_run: null rc" in lpx._lib.last_error()
    assert run(K=None) == EINVAL and "lpx_node_batch_run: null K" in lpx._lib.last_error()
    assert run(slot=None) == EINVAL and "lpx_node_batch_run: null slot" in lpx._lib.last_error()
    for B in (0, -1):
        assert run(B=B) == EINVAL and "lpx_node_batch_run: B is outside [1, W]" in lpx._lib.last_error()
    for flags in (8, 16, -1):
        assert run(flags=flags) == EINVAL and "lpx_node_batch_run: unknown flag" in lpx._lib.last_error()
    assert run(B=2, flags=1 | 4, cutoff=cp) == EINVAL and "lpx_node_batch_run: entry 1: cutoff is NaN" in lpx._lib.last_error()
    assert run(B=2, flags=1 | 4) == EINVAL and "null cutoff" in lpx._lib.last_error()
    assert run(B=2, flags=1, cutoff=cp) == EINVAL and "null batch" in lpx._lib.last_error()       # not read without the flag
    # create and clone
    out = C.c_void_p()
    hs = (C.c_void_p * 2)()
    assert L.lpx_node_batch_create(2, hs, None) == EINVAL and "lpx_node_batch_create: null argument" in lpx._lib.last_error()
    assert L.lpx_node_batch_create(2, None, C.byref(out)) == EINVAL and "null argument" in lpx._lib.last_error()
    for W in (0, 1025):
        assert L.lpx_node_batch_create(W, hs, C.byref(out)) == EINVAL and "W is outside [1, 1024]" in lpx._lib.last_error()
    assert L.lpx_node_batch_create(2, hs, C.byref(out)) == EINVAL and "handle 0: null handle" in lpx._lib.last_error()
    assert L.lpx_tableau_clone(None, C.byref(out)) == EINVAL and "lpx_tableau_clone: null argument" in lpx._lib.last_error()
    assert L.lpx_tableau_clone(None, None) == EINVAL
    L.lpx_node_batch_destroy(None)
    L.lpx_bnb_divers_info_free(None)


def test_a_batch_larger_than_its_handles_is_refused_at_the_driver_level(lpx):
    nb = object.__new__(lpx.NodeBatch)          # no handles are needed to reach the check
    nb._handles, nb._W, nb._h = [], 2, None
    with pytest.raises(ValueError, match=r"B must be in \[1, W\]"):
        nb.run([0, 1, 2], [([], [], [])] * 3, 4)
    with pytest.raises(ValueError, match=r"B must be in \[1, W\]"):
        nb.run([], [], 4)
    with pytest.raises(ValueError, match="3 slots but 2 nodes"):
        nb.run([0, 1, 2], [([], [], [])] * 2, 4)


def test_driver_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r, info, dinfo = lpx._lib.Result(), lpx._lib.BnbBoundedInfo(), lpx._lib.BnbDiversInfo()
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)

    def solve(max_nodes=0, flags=0, divers=4, out=C.byref(r), info=C.byref(info), dinfo=C.byref(dinfo)):
        return L.lpx_solve_bnb_bounded4(C.byref(p), None, upp, None, None, max_nodes, flags, divers, out, info, dinfo)

    for W in (0, 1025, -3):
        assert solve(divers=W) == EINVAL and "lpx_solve_bnb_bounded4: divers is outside [1, 1024]" in lpx._lib.last_error()
    for flags in (1, 8, 2 | 16):
        assert solve(flags=flags) == EINVAL and "search_flags" in lpx._lib.last_error()
    assert solve(max_nodes=-1) == EINVAL and "max_nodes is negative" in lpx._lib.last_error()
    assert solve(out=None) == EINVAL and "lpx_solve_bnb_bounded4: null argument" in lpx._lib.last_error()
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    with pytest.raises(ValueError, match="launches"):
        lpx.LPSolver().SolveBnbBounded(prob, [4, 3, 3], divers=4, node_form="launches")
    with pytest.raises(lpx.SolverException) as e:
        lpx.LPSolver().SolveBnbBounded(prob, [4, 3, 3], divers=0)
    assert e.value.code == EINVAL and "divers is outside" in str(e.value)


def test_no_cpu_fallback(lpx):
    """Without a device the driver, the clone's allocation and the batch are LPX_EDEVICE; with one the driver solves."""
    L = lpx._lib.lib()
    p, hold = _problem(lpx)
    r, info, dinfo = lpx._lib.Result(), lpx._lib.BnbBoundedInfo(), lpx._lib.BnbDiversInfo()
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)
    rc = L.lpx_solve_bnb_bounded4(C.byref(p), None, upp, None, None, 0, 0, 4, C.byref(r), C.byref(info), C.byref(dinfo))
    if L.lpx_device_count() > 0:
        assert rc == 0 and info.nodes >= 1 and dinfo.rounds >= 1
        L.lpx_bnb_bounded_info_free(C.byref(info)); L.lpx_bnb_divers_info_free(C.byref(dinfo)); L.lpx_result_free(C.byref(r))
    else:
        assert rc == lpx._lib.EDEVICE and "no HIP device" in lpx._lib.last_error()
