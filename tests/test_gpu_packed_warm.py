"""GPU tests of the packed calls from a solved base (lpx_packed_base_open / _solve, LPSolver.OpenPackedBase; kernels in
csrc/lpx_packed_warm.hip).  Every comparison with the NumPy restatement of the contract (tests/_packed_warm_ref.py) is bit for bit
(np.uint64 views of the doubles), with and without the long step; the anchors to existing code are base_out against SolvePackedDual
of the base, a b = b0 scenario against the base, and every OPTIMAL scenario within the project's 1e-9 rule of the device's own cold
SolvePackedDual.  The scenario sets and the restatement's answers are shared with tests/test_packed_warm_ref.py, which asserts on
the CPU what they exercise."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _bounded_ref as B
import _packed_dual_ref as P
import _packed_ref as PP
import _packed_warm_ref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
SENSE = {P.MAX: "max", P.MIN: "min"}


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _equal_ref(res, refs, what=""):
    """A PackedDualResult against the restatement's list, every output bit for bit."""
    assert res.Status.tolist() == [r.status for r in refs], what
    for i, r in enumerate(refs):
        assert np.array_equal(_u64(res.Solution[i]), _u64(r.x)), (what, i)
        assert _u64(res.OptimalValue[i]) == _u64(r.value), (what, i)
        assert tuple(res.BoundCounts[i].tolist()) == r.counts and res.Events[i] == r.events, (what, i)
        assert res.Passes[i] == r.counts[2] and res.DualizeFlips[i] == r.dualize_flips, (what, i)
        assert _u64(res.Z[i]) == _u64(r.z), (what, i)
        assert res.Basis[i].tolist() == r.basis.tolist() and res.AtUpper[i].tolist() == r.at_upper.tolist(), (what, i)
        assert np.array_equal(_u64(res.Duals[i]), _u64(r.y)) and np.array_equal(_u64(res.ReducedCosts[i]), _u64(r.d)), (what, i)


def _equal_results(a, b, what="", rows_a=slice(None), rows_b=slice(None), counts=True):
    assert a.Status[rows_a].tolist() == b.Status[rows_b].tolist(), what
    for k in ("Solution", "OptimalValue", "Z", "Duals", "ReducedCosts"):
        assert np.array_equal(_u64(getattr(a, k)[rows_a]), _u64(getattr(b, k)[rows_b])), (what, k)
    for k in ("Basis", "AtUpper") + (("BoundCounts", "Events", "Passes", "DualizeFlips") if counts else ()):
        assert np.array_equal(getattr(a, k)[rows_a], getattr(b, k)[rows_b]), (what, k)


def _open(lpx, name, long_step=True, **kw):
    (c, A, rel, b0, upper, lower, sense), _ = W.scenario_set(name)
    return lpx.LPSolver().OpenPackedBase(c, A, b0, rel, upper, lower, SENSE[sense], long_step=long_step, **kw)


# ---- the sets: the restatement bit for bit, and the anchors to existing code ----------------------------------------------------
@pytest.mark.parametrize("long_step", [True, False])
@pytest.mark.parametrize("name", list(W.SETS))
def test_sets_equal_the_restatement_and_the_anchors(gpu, name, long_step):
    (c, A, rel, b0, upper, lower, sense), bs = W.scenario_set(name)
    refs, ref_base = W.set_refs(name, long_step), W.set_base(name, long_step)
    m, n = A.shape
    assert gpu._lib.lib().lpx_packed_fits(m, n) == 1
    S = gpu.LPSolver()
    cold_base = S.SolvePackedDual(c, A, b0, rel, upper, lower, SENSE[sense], long_step)
    with _open(gpu, name, long_step) as base:
        _equal_ref(base.Base, [ref_base.cold], name + ": base_out")
        _equal_results(base.Base, cold_base, name + ": base_out against SolvePackedDual")
        res = base.solve(bs, long_step=long_step)
        _equal_ref(res, refs, name)
        assert res.Stats["launches"] == 1 and res.Stats["pivots"] == sum(r.counts[0] + r.counts[1] for r in refs)
        # b = b0: the base again, with no event
        assert np.array_equal(bs[0], b0) and res.Events[0] == 0 and not res.BoundCounts[0].any() and res.DualizeFlips[0] == 0
        _equal_results(res, base.Base, name + ": b = b0", rows_a=slice(0, 1), counts=False)
        again = base.solve(bs[::-1], long_step=long_step)                         # the handle is only read; the order does not matter
        _equal_ref(again, refs[::-1], name + ": reversed")
    # the device's own cold solve of every scenario: equal statuses, optima within the 1e-9 rule
    cold = S.SolvePackedDual(c, A, bs, rel, upper, lower, SENSE[sense], long_step)
    assert res.Status.tolist() == cold.Status.tolist()
    for i in range(len(bs)):
        if cold.Status[i] == P.OPTIMAL:
            assert abs(res.OptimalValue[i] - cold.OptimalValue[i]) <= 1e-9 * max(1.0, abs(cold.OptimalValue[i])), (name, i)


# ---- one batch of 300 scenarios with OPTIMAL, INFEASIBLE and EINVAL -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mix():
    """300 right-hand sides of the mixed 12 x 16 model, moved by integers in [-25, 25): more workgroups than compute units.  A NaN
    and an infinity refuse their scenarios alone; the same right-hand side stands at 0, 255 and 299."""
    (c, A, rel, b0, upper, lower, sense), _ = W.scenario_set("mixed 12x16")
    g = np.random.default_rng(77)
    bs = b0 + g.integers(-25, 25, size=(300, 12)).astype(np.float64)
    bs[0] = bs[255] = bs[299] = b0 + np.arange(12.0) - 6.0
    bs[17, 3] = np.nan; bs[200, 11] = INF; bs[201, 0] = -INF
    return bs, W.solve_all(W.set_base("mixed 12x16", True), bs)


def test_batch_of_300_with_every_status(gpu):
    bs, refs = _mix()
    count = {s: sum(1 for r in refs if r.status == s) for s in (P.OPTIMAL, P.INFEASIBLE, P.EINVAL)}
    assert all(v > 0 for v in count.values()) and sum(count.values()) == 300 and count[P.EINVAL] == 3, count
    assert refs[0].events > 0
    with _open(gpu, "mixed 12x16") as base:
        res = base.solve(bs)
        _equal_ref(res, refs, "the batch")
        assert res.Stats["launches"] == 1 and res.Stats["pivots"] == sum(r.counts[0] + r.counts[1] for r in refs)
        bad = res.Status < 0
        assert np.flatnonzero(bad).tolist() == [17, 200, 201]
        for k in ("Solution", "OptimalValue", "Basis", "AtUpper", "Events", "BoundCounts", "DualizeFlips", "Z", "Duals", "ReducedCosts"):
            assert not getattr(res, k)[bad].any(), k
        assert not np.signbit(res.Solution[bad]).any() and not np.signbit(res.Duals[bad]).any()
        for i in (255, 299):                                                        # the position does not matter
            _equal_results(res, res, "position %d" % i, rows_a=slice(0, 1), rows_b=slice(i, i + 1))
        for i in (0, 1, 17, 150, 299):                                              # nor do count and the other scenarios
            _equal_ref(base.solve(bs[i]), [refs[i]], "scenario %d alone" % i)


# ---- the iteration limit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_step", [True, False])
@pytest.mark.parametrize("max_iter", [0, 1, 2])
def test_iteration_limit_is_tested_first(gpu, max_iter, long_step):
    """The limit is tested at the head of a trip: a trip that starts below it may pass it by its passes; with max_iter = 0 even a
    scenario that needs no event ends at the limit."""
    base_ref = W.set_base("covering 12x60", long_step)
    bs = W.scenario_set("covering 12x60")[1][:3]
    refs = W.solve_all(base_ref, bs, long_step=long_step, max_iter=max_iter)
    assert all(r.status == P.ITER_LIMIT and r.events >= max_iter for r in refs[1:]) and (max_iter > 0 or refs[0].status == P.ITER_LIMIT)
    with _open(gpu, "covering 12x60", long_step) as base:
        _equal_ref(base.solve(bs, long_step=long_step, max_iter=max_iter), refs, "max_iter %d" % max_iter)


def test_a_base_that_is_not_optimal_gives_no_handle(gpu):
    (c, A, rel, b0, upper, lower, sense), _ = W.scenario_set("covering 6x12")
    S = gpu.LPSolver()
    for kw, code in ((dict(b=1.5 * A.sum(axis=1)), P.INFEASIBLE), (dict(max_iter=1), P.ITER_LIMIT), (dict(upper=-1.0), gpu._lib.EINVAL)):
        args = dict(c=c, A=A, b=b0, rel=rel, upper=upper, sense="min"); args.update(kw)
        with pytest.raises(gpu.SolverException) as e:
            S.OpenPackedBase(**args)
        assert e.value.code == code and str(e.value).find("lpx_packed_base_open: ") >= 0, (kw, str(e.value))
    # through the C ABI: base_out is filled as lpx_solve_packed_dual fills it, *h is NULL
    Lb = gpu._lib
    bad_b = np.ascontiguousarray(1.5 * A.sum(axis=1)); up = np.ones(12)
    pm = Lb.PackedBaseModel(6, 12, 1, c.ctypes.data_as(Lb.dp), np.ascontiguousarray(A).ctypes.data_as(Lb.dp), bad_b.ctypes.data_as(Lb.dp),
                            None, up.ctypes.data_as(Lb.dp), rel.ctypes.data_as(Lb.ip))
    status = np.full(1, 77, dtype=np.int32); x = np.zeros(12); value = np.zeros(1)
    pr = Lb.PackedDualResults(status.ctypes.data_as(Lb.ip), x.ctypes.data_as(Lb.dp), value.ctypes.data_as(Lb.dp), None, None, None, None, None)
    h = C.c_void_p(12345)
    assert Lb.lib().lpx_packed_base_open(C.byref(pm), Lb.BDUAL_LONG_STEP, None, C.byref(pr), C.byref(h)) == P.INFEASIBLE
    ref = P.solve(c, A, bad_b, rel, None, up, P.MIN)
    assert h.value is None and status[0] == P.INFEASIBLE == ref.status and np.array_equal(_u64(x), _u64(ref.x)) and _u64(value[0]) == _u64(ref.value)


# ---- optional outputs, guard bytes, stats -------------------------------------------------------------------------------------
SIZES = lambda count, m, n: {"status": 4 * count, "x": 8 * count * n, "value": 8 * count, "rec": 48 * count, "basis": 4 * count * m,
                             "at_upper": count * n, "y": 8 * count * m, "d": 8 * count * n}
NAMES = ("status", "x", "value", "rec", "basis", "at_upper", "y", "d")


def _raw_results(Lb, count, m, n, want):
    GUARD = 64
    sizes = SIZES(count, m, n)
    bufs = {k: np.full(v + GUARD, 0xA5, dtype=np.uint8) for k, v in sizes.items()}
    types = {"status": Lb.ip, "x": Lb.dp, "value": Lb.dp, "rec": C.POINTER(Lb.PackedDualRecord), "basis": Lb.ip,
             "at_upper": C.POINTER(C.c_uint8), "y": Lb.dp, "d": Lb.dp}
    ptr = lambda k: C.cast(C.c_void_p(bufs[k].ctypes.data), types[k]) if k in want else None
    return bufs, sizes, Lb.PackedDualResults(*[ptr(k) for k in NAMES])


def _raw_solve(lpx, h, bs, m, n, want):
    """lpx_packed_base_solve through ctypes on arrays with 64 guard bytes behind each; returns the arrays (as bytes) and the stats."""
    Lb = lpx._lib
    bufs, sizes, pr = _raw_results(Lb, len(bs), m, n, want)
    st = Lb.Stats()
    bs = np.ascontiguousarray(bs)
    assert Lb.lib().lpx_packed_base_solve(h, len(bs), bs.ctypes.data_as(Lb.dp), Lb.BDUAL_LONG_STEP, None, C.byref(pr), C.byref(st)) == 0, Lb.last_error()
    for k, v in sizes.items():
        assert (bufs[k][v:] == 0xA5).all(), "guard bytes behind " + k
    return {k: bufs[k][:v].tobytes() for k, v in sizes.items()}, st


def test_optional_outputs_guard_bytes_and_stats(gpu):
    (c, A, rel, b0, upper, lower, sense), bs = W.scenario_set("covering 6x12")
    refs = W.set_refs("covering 6x12", True)
    required = ("status", "x", "value")
    optional = ("rec", "basis", "at_upper", "y", "d")
    with _open(gpu, "covering 6x12") as base:
        full, st = _raw_solve(gpu, base._h, bs, 6, 12, required + optional)
        lean, st2 = _raw_solve(gpu, base._h, bs, 6, 12, required)
        some, st3 = _raw_solve(gpu, base._h, bs, 6, 12, required + ("basis", "y"))
    for k in required:
        assert full[k] == lean[k] == some[k], k
    for k in optional:                                                              # NULL: not written at all
        assert lean[k] == b"\xa5" * len(lean[k]), k
        assert some[k] == (full[k] if k in ("basis", "y") else b"\xa5" * len(some[k])), k
    assert np.frombuffer(full["status"], dtype=np.int32).tolist() == [r.status for r in refs]
    assert np.array_equal(np.frombuffer(full["x"], dtype=np.uint64), np.concatenate([_u64(r.x) for r in refs]))
    assert np.array_equal(np.frombuffer(full["value"], dtype=np.uint64), np.array([_u64(r.value) for r in refs]).ravel())
    assert np.array_equal(np.frombuffer(full["y"], dtype=np.uint64), np.concatenate([_u64(r.y) for r in refs]))
    assert np.array_equal(np.frombuffer(full["d"], dtype=np.uint64), np.concatenate([_u64(r.d) for r in refs]))
    assert np.frombuffer(full["basis"], dtype=np.int32).tolist() == np.concatenate([r.basis for r in refs]).tolist()
    assert np.frombuffer(full["at_upper"], dtype=np.uint8).tolist() == np.concatenate([r.at_upper for r in refs]).tolist()
    pivots = sum(r.counts[0] + r.counts[1] for r in refs)
    for s in (st, st2, st3):
        assert s.launches == 1 and s.pivots == pivots and s.loop_ms > 0.0
    # base_out of open: the optional outputs as NULL, guard bytes behind the others
    Lb = gpu._lib
    bufs, sizes, pr = _raw_results(Lb, 1, 6, 12, required + ("y",))
    up = np.ones(12); cc, AA, bb = (np.ascontiguousarray(v) for v in (c, A, b0))
    pm = Lb.PackedBaseModel(6, 12, 1, cc.ctypes.data_as(Lb.dp), AA.ctypes.data_as(Lb.dp), bb.ctypes.data_as(Lb.dp), None,
                            up.ctypes.data_as(Lb.dp), rel.ctypes.data_as(Lb.ip))
    h = C.c_void_p()
    assert Lb.lib().lpx_packed_base_open(C.byref(pm), Lb.BDUAL_LONG_STEP, None, C.byref(pr), C.byref(h)) == 0, Lb.last_error()
    assert Lb.lib().lpx_packed_base_close(h) == 0
    cold = W.set_base("covering 6x12", True).cold
    for k, v in sizes.items():
        assert (bufs[k][v:] == 0xA5).all(), "guard bytes behind " + k
        if k not in required + ("y",):
            assert (bufs[k] == 0xA5).all(), k
    assert np.array_equal(bufs["x"][:sizes["x"]].view(np.uint64), _u64(cold.x)) and np.array_equal(bufs["y"][:sizes["y"]].view(np.uint64), _u64(cold.y))


# ---- handles and the arena, shared with lpx_solve_packed ------------------------------------------------------------------------
def test_two_handles_interleaved_the_arena_shared_and_a_solve_after_the_other_close(gpu):
    """Two bases open at once, their solves interleaved; a larger solve after a smaller one (the arena grows); a packed primal call
    between two warm solves (the arena is that call's too); a solve after the other handle was closed -- the same bits each time."""
    refs_a, refs_b = W.set_refs("covering 6x12", True), W.set_refs("mixed 12x16", True)
    bs_a, bs_b = W.scenario_set("covering 6x12")[1], W.scenario_set("mixed 12x16")[1]
    S = gpu.LPSolver()
    a, b = _open(gpu, "covering 6x12"), _open(gpu, "mixed 12x16")
    try:
        _equal_ref(a.solve(bs_a), refs_a, "a first")
        _equal_ref(b.solve(bs_b), refs_b, "b first")
        reps = 400                                                                  # 3200 scenarios: well beyond the first arena
        big = a.solve(np.tile(bs_a, (reps, 1)))
        for k in range(len(refs_a)):
            sel = slice(k, None, len(refs_a))
            assert (big.Status[sel] == refs_a[k].status).all() and (_u64(big.Solution[sel]) == _u64(refs_a[k].x)).all()
            assert (_u64(big.OptimalValue[sel]) == _u64(refs_a[k].value)).all() and (big.Basis[sel] == refs_a[k].basis).all()
            assert (big.BoundCounts[sel] == np.array(refs_a[k].counts)).all() and (_u64(big.Duals[sel]) == _u64(refs_a[k].y)).all()
        _equal_ref(b.solve(bs_b), refs_b, "b after the large solve of a")
        pc, pA, pb = (np.stack([B.binary_bounded(12, 6, s)[3][k] for s in (1, 2, 3)]) for k in range(3))
        primal = S.SolvePacked(pc, pA, pb, 1.0)
        for i, r in enumerate(PP.solve_all(pc, pA, pb, None, 1.0)):                 # the bits of the packed primal call
            assert primal.Status[i] == r.status and np.array_equal(_u64(primal.Solution[i]), _u64(r.x))
            assert _u64(primal.OptimalValue[i]) == _u64(r.value) and primal.Basis[i].tolist() == r.basis.tolist()
        _equal_ref(a.solve(bs_a), refs_a, "a after the primal call")
        a.close()
        a.close()                                                                   # closing twice is harmless
        with pytest.raises(gpu.SolverException):
            a.solve(bs_a)
        _equal_ref(b.solve(bs_b), refs_b, "b after a was closed")
    finally:
        a.close(); b.close()


def test_a_solve_with_other_flags_and_limits_than_the_base(gpu):
    """The long-step flag and max_iter are the call's own: a base opened with the long step serves a solve without it."""
    bs = W.scenario_set("covering 12x60")[1]
    base_ref = W.set_base("covering 12x60", True)
    refs = W.solve_all(base_ref, bs, long_step=False)
    with _open(gpu, "covering 12x60", True) as base:
        _equal_ref(base.solve(bs, long_step=False), refs, "long-step base, plain solve")


# ---- the command line: a fresh child process per call ---------------------------------------------------------------------------
def test_cli_warm_base_equals_packed_base_solve(gpu, tmp_path):
    c, A, rel, b, upper = P.hand_model()
    model = tmp_path / "hand.txt"
    model.write_text("Min: 2x1 + 3x2 + 1x3\n1x1 + 1x2 + 1x3 >= 4\n1x1 - 1x2 + 2x3 <= 3\n")
    rhs = ["4 3", "7 3", "4 -1", "2 5", "9 3"]                                      # the last: more than the bounds can cover
    f = tmp_path / "rhs.txt"
    f.write_text("".join(line + "\n" for line in rhs))
    bs = np.array([[float(v) for v in row.split()] for row in rhs])
    exe = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
    bounds = ("--upper", "1=3", "--upper", "2=3", "--upper", "3=2")
    for flags, long_step in ((("--long-step",), True), ((), False)):
        out = subprocess.run([exe, "--bounded-dual", *flags, "--warm-base", "--rhs-file", str(f), *bounds, str(model)],
                             check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
        assert len(out) == len(rhs)
        with gpu.LPSolver().OpenPackedBase(c, A, b, rel, upper, np.zeros(3), "min", long_step=long_step) as base:    # the CLI passes both bound arrays
            res = base.solve(bs, long_step=long_step)
        refs = W.solve_all(W.open_base(c, A, b, rel, np.zeros(3), upper, P.MIN, long_step=long_step), bs, long_step=long_step)
        _equal_ref(res, refs, "hand")
        for i, line in enumerate(out):
            got = line.split()
            assert int(got[0]) == res.Status[i] and float(got[1]) == res.OptimalValue[i], (i, line)
            assert [float(v) for v in got[2:]] == res.Solution[i].tolist(), (i, line)
        assert res.Status[0] == P.OPTIMAL and res.Status[-1] == P.INFEASIBLE
    refused = subprocess.run([exe, "--warm-base", "--rhs-file", str(f), str(model)], capture_output=True, text=True, timeout=120)
    assert refused.returncode == 64 and "--warm-base needs --bounded-dual --rhs-file" in refused.stderr
