"""CPU checks of the entry points of strong branching by probes (lpx_bounded_probe, lpx_node_batch_run_probe,
lpx_solve_bnb_bounded6, lpx_bnb_strong_info_free): exported and declared, mirrored in C# and Python, struct sizes, argument
errors before device errors with their messages, the Python-level errors, and no CPU fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lpx_bounded_probe", "lpx_node_batch_run_probe", "lpx_solve_bnb_bounded6", "lpx_bnb_strong_info_free")


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
    for cs, c in (("LpxProbeHead", "lpx_probe_head"), ("LpxProbeRecord", "lpx_probe_record"), ("LpxBnbStrongInfo", "lpx_bnb_strong_info")):
        assert "struct " + cs in native and "} %s;" % c in hdr
    assert L.lpx_abi_version() == 1
    assert hasattr(lpx.NodeBatch, "run_probe") and hasattr(lpx.DeviceTableau, "probe")
    assert C.sizeof(lpx._lib.ProbeHead) == 16 and C.sizeof(lpx._lib.ProbeRecord) == 64 and C.sizeof(lpx._lib.BnbStrongInfo) == 48
    assert C.sizeof(lpx._lib.NodeRecord) == 64                 # untouched
    assert re.search(r"#define LPX_PROBE_NONE \(-2\)", hdr) and lpx._lib.PROBE_NONE == -2
    assert "#define LPX_BRANCH_STRONG 1" in hdr and lpx._lib.BRANCHINGS == {"most_fractional": 0, "strong": 1}
    cli = open(os.path.join(ROOT, "tools", "lpx_cli.cpp")).read()
    assert "--branching" in cli and "--candidates" in cli and "--probe-iter" in cli and "lpx_solve_bnb_bounded6(" in cli
    bench = open(os.path.join(ROOT, "tools", "bench_bnb_bounded.py")).read()
    assert "--compare-branching" in bench and "--branching" in bench


def test_cli_help_lists_the_branching_options(lpx):
    import subprocess
    exe = os.path.join(os.path.dirname(lpx.__file__), "lpx_cli")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    for word in ("--branching most_fractional|strong", "--candidates", "--probe-iter"):
        assert word in out.stdout, word
    bad = subprocess.run([exe, "--binary", "--bnb-bounded", "--branching", "weak", "x.txt"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 64 and "--branching takes most_fractional or strong" in bad.stderr
    bad = subprocess.run([exe, "--binary", "--bnb-bounded", "--branching", "strong", "--candidates", "33", "x.txt"], capture_output=True,
                         text=True, timeout=60)
    assert bad.returncode == 64 and "--candidates takes a count in [1, 32]" in bad.stderr
    bad = subprocess.run([exe, "--binary", "--bnb-bounded", "--branching", "strong", "--plunge", "4", "x.txt"], capture_output=True,
                         text=True, timeout=60)
    assert bad.returncode == 64 and "not with --plunge" in bad.stderr


def test_probe_argument_errors_come_first(lpx):
    """Checked before any device is looked for: the same answers with and without a GPU."""
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    head = lpx._lib.ProbeHead()
    recs = (lpx._lib.ProbeRecord * 64)()
    nan = float("nan")

    def err():
        return lpx._lib.last_error()

    # no handle can be made without a device: the checks that need none come in front of the null handle
    assert L.lpx_bounded_probe(None, None, 1 | 2 | 4, -np.inf, -np.inf, 0, None, 1e-6, 32, 0, C.byref(head), recs) == EINVAL
    assert "lpx_bounded_probe: null handle" in err()
    assert L.lpx_bounded_probe(None, None, 1, 0.0, 0.0, 0, None, 1e-6, 4, 10, None, recs) == EINVAL and "lpx_bounded_probe: null head" in err()
    assert L.lpx_bounded_probe(None, None, 1, 0.0, 0.0, 0, None, 1e-6, 4, 10, C.byref(head), None) == EINVAL and "lpx_bounded_probe: null out" in err()
    for cm in (0, 33, -1):
        assert L.lpx_bounded_probe(None, None, 1, 0.0, 0.0, 0, None, 1e-6, cm, 10, C.byref(head), recs) == EINVAL
        assert "lpx_bounded_probe: cand_max is outside [1, 32]" in err()
    assert L.lpx_bounded_probe(None, None, 1, 0.0, 0.0, 0, None, 1e-6, 4, -1, C.byref(head), recs) == EINVAL
    assert "lpx_bounded_probe: probe_iter is negative" in err()
    assert L.lpx_bounded_probe(None, None, 1, 0.0, nan, 0, None, 1e-6, 4, 10, C.byref(head), recs) == EINVAL
    assert "lpx_bounded_probe: prune is NaN" in err()
    for flags in (8, 16, -1):
        assert L.lpx_bounded_probe(None, None, flags, 0.0, 0.0, 0, None, 1e-6, 4, 10, C.byref(head), recs) == EINVAL
        assert "lpx_bounded_probe: unknown flag" in err()
    assert L.lpx_bounded_probe(None, None, 1 | 4, nan, 0.0, 0, None, 1e-6, 4, 10, C.byref(head), recs) == EINVAL
    assert "lpx_bounded_probe: cutoff is NaN" in err()


def test_run_probe_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL, ip, dp = lpx._lib.EINVAL, lpx._lib.ip, lpx._lib.dp
    slot = np.zeros(2, dtype=np.int32); K = np.zeros(2, dtype=np.int32); rc = np.zeros(2, dtype=np.int32)
    recs = (lpx._lib.NodeRecord * 2)()
    heads = (lpx._lib.ProbeHead * 2)()
    probes = (lpx._lib.ProbeRecord * 128)()
    cut = np.array([0.0, float("nan")])
    prune = np.array([-np.inf, 1.0]); bad_prune = np.array([0.0, float("nan")])
    sp, kp, rp, cp, pp = (slot.ctypes.data_as(ip), K.ctypes.data_as(ip), rc.ctypes.data_as(ip), cut.ctypes.data_as(dp),
                          prune.ctypes.data_as(dp))

    def run(batch=None, B=1, slot=sp, K=kp, flags=1, cutoff=None, prune=pp, cand_max=4, probe_iter=8, out=recs, head=heads,
            probes=probes, rc=rp):
        return L.lpx_node_batch_run_probe(batch, B, slot, K, None, None, None, None, flags, cutoff, prune, 0, None, 1e-6, cand_max,
                                          probe_iter, out, head, probes, rc)

    def err():
        return lpx._lib.last_error()

    assert run() == EINVAL and "lpx_node_batch_run_probe: null batch" in err()
    for name in ("out", "rc", "K", "slot", "prune", "head", "probes"):
        assert run(**{name: None}) == EINVAL and "lpx_node_batch_run_probe: null " + name in err(), name
    for cm in (0, 33, -4):
        assert run(cand_max=cm) == EINVAL and "lpx_node_batch_run_probe: cand_max is outside [1, 32]" in err()
    assert run(probe_iter=-1) == EINVAL and "lpx_node_batch_run_probe: probe_iter is negative" in err()
    for B in (0, -1):
        assert run(B=B) == EINVAL and "lpx_node_batch_run_probe: B is outside [1, W]" in err()
    for flags in (8, 16, -1):
        assert run(flags=flags) == EINVAL and "lpx_node_batch_run_probe: unknown flag" in err()
    assert run(B=2, flags=1 | 4, cutoff=cp) == EINVAL and "lpx_node_batch_run_probe: entry 1: cutoff is NaN" in err()
    assert run(B=2, flags=1 | 4) == EINVAL and "null cutoff" in err()
    assert run(B=2, flags=1, cutoff=cp) == EINVAL and "null batch" in err()          # not read without the flag
    assert run(B=2, prune=bad_prune.ctypes.data_as(dp)) == EINVAL and "lpx_node_batch_run_probe: entry 1: prune is NaN" in err()
    assert run(B=1, prune=bad_prune.ctypes.data_as(dp)) == EINVAL and "null batch" in err()     # entry 1 is not read with B = 1
    # the entry it is built on keeps its own name in its messages
    assert L.lpx_node_batch_run(None, 1, sp, kp, None, None, None, None, 1, None, 0, None, 1e-6, recs, rp) == EINVAL
    assert "lpx_node_batch_run: null batch" in err()
    L.lpx_bnb_strong_info_free(None)
    s = lpx._lib.BnbStrongInfo(1, 2, 3, 4, 5, 6)
    L.lpx_bnb_strong_info_free(C.byref(s))
    assert (s.probe_launches, s.probes, s.changed_picks) == (0, 0, 0)


def test_python_level_errors(lpx):
    nb = object.__new__(lpx.NodeBatch)          # no handles are needed to reach the checks
    nb._handles, nb._W, nb._h = [], 2, None
    with pytest.raises(ValueError, match=r"B must be in \[1, W\]"):
        nb.run_probe([0, 1, 2], [([], [], [])] * 3, 4, 4)
    with pytest.raises(ValueError, match="3 slots but 2 nodes"):
        nb.run_probe([0, 1, 2], [([], [], [])] * 2, 4, 4)
    for cm in (0, 33):
        with pytest.raises(ValueError, match=r"cand_max must be in \[1, 32\]"):
            nb.run_probe([0], [([], [], [])], 4, cm)
    dt = object.__new__(lpx.DeviceTableau)
    dt._h = None
    for cm in (0, 33):
        with pytest.raises(ValueError, match=r"cand_max must be in \[1, 32\]"):
            dt.probe(4, cm)
    prob = lpx.LPProblem.from_arrays(0, [3, 5, 2], [[1, 2, 2], [2, 4, 3]], [0, 0], [10, 15])
    S = lpx.LPSolver()
    with pytest.raises(ValueError, match="launches"):
        S.SolveBnbBounded(prob, [4, 3, 3], branching="strong", node_form="launches")
    with pytest.raises(ValueError, match="plunge"):
        S.SolveBnbBounded(prob, [4, 3, 3], branching="strong", plunge=4)
    with pytest.raises(ValueError, match="unknown branching rule"):
        S.SolveBnbBounded(prob, [4, 3, 3], branching="pseudo")
    for cm in (0, 33):
        with pytest.raises(ValueError, match=r"candidates must be in \[1, 32\]"):
            S.SolveBnbBounded(prob, [4, 3, 3], branching="strong", candidates=cm)
    with pytest.raises(lpx.SolverException) as e:
        S.SolveBnbBounded(prob, [4, 3, 3], branching="strong", probe_iter=-2)
    assert e.value.code == lpx._lib.EINVAL and "probe_iter is negative" in str(e.value)
    with pytest.raises(lpx.SolverException) as e:
        S.SolveBnbBounded(prob, [4, 3, 3], branching="strong", divers=0)
    assert e.value.code == lpx._lib.EINVAL and "divers is outside" in str(e.value)


def test_driver_argument_errors_come_first(lpx):
    L = lpx._lib.lib()
    EINVAL = lpx._lib.EINVAL
    p, hold = _problem(lpx)
    r, info, dinfo, sinfo = lpx._lib.Result(), lpx._lib.BnbBoundedInfo(), lpx._lib.BnbDiversInfo(), lpx._lib.BnbStrongInfo()
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)

    def solve(max_nodes=0, flags=0, divers=2, branching=1, cand_max=4, probe_iter=8, out=C.byref(r)):
        return L.lpx_solve_bnb_bounded6(C.byref(p), None, upp, None, None, max_nodes, flags, divers, branching, cand_max, probe_iter,
                                        out, C.byref(info), C.byref(dinfo), C.byref(sinfo))

    for W in (0, 1025, -3):
        assert solve(divers=W) == EINVAL and "lpx_solve_bnb_bounded6: divers is outside [1, 1024]" in lpx._lib.last_error()
    for br in (2, -1, 7):
        assert solve(branching=br) == EINVAL and "lpx_solve_bnb_bounded6: branching is neither" in lpx._lib.last_error()
    for br in (0, 1):                                           # checked whichever rule is asked for
        for cm in (0, 33, -3):
            assert solve(branching=br, cand_max=cm) == EINVAL and "lpx_solve_bnb_bounded6: cand_max is outside [1, 32]" in lpx._lib.last_error()
        assert solve(branching=br, probe_iter=-1) == EINVAL and "lpx_solve_bnb_bounded6: probe_iter is negative" in lpx._lib.last_error()
    for flags in (1, 8, 2 | 16):
        assert solve(flags=flags) == EINVAL and "search_flags" in lpx._lib.last_error()
    assert solve(max_nodes=-1) == EINVAL and "max_nodes is negative" in lpx._lib.last_error()
    assert solve(out=None) == EINVAL and "lpx_solve_bnb_bounded6: null argument" in lpx._lib.last_error()
    frac = np.array([4.0, 2.5, 3.0])
    rc = L.lpx_solve_bnb_bounded6(C.byref(p), None, frac.ctypes.data_as(lpx._lib.dp), None, None, 0, 0, 2, 1, 4, 8, C.byref(r), None, None, None)
    assert rc == EINVAL and "needs finite, integral lower and upper bounds" in lpx._lib.last_error()


@pytest.mark.parametrize("branching", [0, 1])
def test_no_cpu_fallback(lpx, branching):
    """Without a device the driver is LPX_EDEVICE; with one it solves."""
    L = lpx._lib.lib()
    p, hold = _problem(lpx)
    r, info, dinfo, sinfo = lpx._lib.Result(), lpx._lib.BnbBoundedInfo(), lpx._lib.BnbDiversInfo(), lpx._lib.BnbStrongInfo()
    up = np.array([4.0, 3.0, 3.0]); upp = up.ctypes.data_as(lpx._lib.dp)
    rc = L.lpx_solve_bnb_bounded6(C.byref(p), None, upp, None, None, 0, 0, 2, branching, 4, 100, C.byref(r), C.byref(info),
                                  C.byref(dinfo), C.byref(sinfo))
    if L.lpx_device_count() > 0:
        assert rc == 0 and info.nodes >= 1 and dinfo.rounds >= 1
        assert sinfo.probe_launches == (dinfo.rounds if branching else 0)
        L.lpx_bnb_bounded_info_free(C.byref(info)); L.lpx_bnb_divers_info_free(C.byref(dinfo)); L.lpx_bnb_strong_info_free(C.byref(sinfo))
        L.lpx_result_free(C.byref(r))
    else:
        assert rc == lpx._lib.EDEVICE and "no HIP device" in lpx._lib.last_error()
