"""GPU tests of the packed cost and right-hand-side scenarios from a solved base (lpx_packed_base_solve_costs,
PackedBase.solve_costs; kernel in csrc/lpx_packed_cost.hip).  Every comparison with the NumPy restatement of the contract
(tests/_packed_cost_ref.py) is bit for bit (np.uint64 views of the doubles) and in every output, with and without b, with and
without the long step; the anchors to existing code are c_i = c0 against the base, c_i = c0 with b against PackedBase.solve, and
every OPTIMAL scenario within the project's 1e-9 rule of the device's own cold SolvePackedDual where that call accepts it.  The
scenario sets and the restatement's answers are shared with tests/test_packed_cost_ref.py, which asserts on the CPU what they
exercise."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _packed_cost_ref as K
import _packed_dual_ref as P
import _packed_warm_ref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
SENSE = {P.MAX: "max", P.MIN: "min"}


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _equal_ref(res, refs, what=""):
    """A PackedCostResult against the restatement's list, every output bit for bit."""
    assert res.Status.tolist() == [r.status for r in refs], what
    for i, r in enumerate(refs):
        assert np.array_equal(_u64(res.Solution[i]), _u64(r.x)), (what, i)
        assert _u64(res.OptimalValue[i]) == _u64(r.value), (what, i)
        assert (res.PrimalEvents[i], res.DualEvents[i]) == (r.primal_events, r.dual_events), (what, i)
        assert tuple(res.PrimalCounts[i].tolist()) == r.pcounts and tuple(res.DualCounts[i].tolist()) == r.dcounts, (what, i)
        assert res.Events[i] == r.primal_events + r.dual_events and _u64(res.Z[i]) == _u64(r.z), (what, i)
        assert res.Basis[i].tolist() == r.basis.tolist() and res.AtUpper[i].tolist() == r.at_upper.tolist(), (what, i)
        assert np.array_equal(_u64(res.Duals[i]), _u64(r.y)) and np.array_equal(_u64(res.ReducedCosts[i]), _u64(r.d)), (what, i)
    assert res.Stats["launches"] == 1 and res.Stats["pivots"] == sum(sum(r.pcounts[:2]) + sum(r.dcounts[:2]) for r in refs), what


def _equal_outputs(a, b, what="", rows_a=slice(None), rows_b=slice(None)):
    """The outputs two result classes share, bit for bit."""
    assert a.Status[rows_a].tolist() == b.Status[rows_b].tolist(), what
    for k in ("Solution", "OptimalValue", "Z", "Duals", "ReducedCosts"):
        assert np.array_equal(_u64(getattr(a, k)[rows_a]), _u64(getattr(b, k)[rows_b])), (what, k)
    for k in ("Basis", "AtUpper"):
        assert np.array_equal(getattr(a, k)[rows_a], getattr(b, k)[rows_b]), (what, k)


def _open_model(lpx, model, long_step=True, **kw):
    c, A, rel, b0, upper, lower, sense = model
    return lpx.LPSolver().OpenPackedBase(c, A, b0, rel, upper, lower, SENSE[sense], long_step=long_step, **kw)


def _open(lpx, name, long_step=True, **kw):
    return _open_model(lpx, W.scenario_set(name)[0], long_step, **kw)


# ---- the sets: the restatement bit for bit, and the anchors to existing code ----------------------------------------------------
@pytest.mark.parametrize("long_step", [True, False])
@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("name", list(W.SETS))
def test_sets_equal_the_restatement_and_the_anchors(gpu, name, with_b, long_step):
    (c0, A, rel, b0, upper, lower, sense), cs, rhs = K.cost_set(name)
    refs = K.set_refs(name, long_step, with_b)
    m, n = A.shape
    assert gpu._lib.lib().lpx_packed_fits(m, n) == 1
    bs = rhs if with_b else None
    with _open(gpu, name, long_step) as base:
        res = base.solve_costs(cs, bs, long_step=long_step)
        _equal_ref(res, refs, name)
        # c = c0: the base again with no event; with b the right-hand-side call
        assert np.array_equal(cs[0], c0) and res.PrimalEvents[0] == 0 and not res.PrimalCounts[0].any()
        if with_b:
            warm = base.solve(rhs, long_step=long_step)
            same = base.solve_costs(c0, rhs, long_step=long_step)                  # one cost vector broadcast against the batch of b
            _equal_outputs(same, warm, name + ": c = c0 with b")
            assert np.array_equal(same.DualCounts, warm.BoundCounts) and np.array_equal(same.DualEvents, warm.Events)
            assert not same.PrimalEvents.any()
        else:
            assert res.Events[0] == 0 and not res.DualEvents.any() and not res.DualCounts.any()
            _equal_outputs(res, base.Base, name + ": c = c0", rows_a=slice(0, 1))
        again = base.solve_costs(cs[::-1], None if bs is None else bs[::-1], long_step=long_step)     # the handle is only read
        _equal_ref(again, refs[::-1], name + ": reversed")
        _equal_outputs(base.solve(b0, long_step=long_step), base.Base, name + ": the handle is unchanged")
    # the device's own cold solve of every scenario it accepts: equal statuses, optima within the 1e-9 rule
    cold = gpu.LPSolver().SolvePackedDual(cs, A, rhs if with_b else b0, rel, upper, lower, SENSE[sense], long_step)
    for i in range(len(cs)):
        if cold.Status[i] == P.EINVAL:
            continue                                                                # an improving cost on a column without an upper bound
        assert res.Status[i] == cold.Status[i], (name, i)
        if cold.Status[i] == P.OPTIMAL:
            assert abs(res.OptimalValue[i] - cold.OptimalValue[i]) <= 1e-9 * max(1.0, abs(cold.OptimalValue[i])), (name, i)
    assert (cold.Status[1:K.N_SPREAD + 1] != P.EINVAL).all()


def test_the_unbounded_hand_model(gpu):
    model, cs, rhs = K.unbounded_hand()
    cb = K.open_model(model)
    with _open_model(gpu, model) as base:
        res = base.solve_costs(cs)
        _equal_ref(res, K.solve_all(cb, cs), "hand")
        assert res.Status.tolist() == [K.OPTIMAL, K.UNBOUNDED, K.OPTIMAL] and res.OptimalValue.tolist() == [3.0, -3.0, 6.0]
        resb = base.solve_costs(cs, rhs)
        _equal_ref(resb, K.solve_all(cb, cs, rhs), "hand with b")
        assert resb.Status.tolist() == [K.OPTIMAL, K.UNBOUNDED, K.OPTIMAL] and resb.DualEvents[1] == 0


def test_a_delta_on_basic_columns_only_and_on_nonbasic_columns_only(gpu):
    """mixed 12x16: the sum over the rows runs only for a basic column's g, the subtraction only for a non-basic column's."""
    cb = K.set_base("mixed 12x16")
    (c0, A, rel, b0, upper, lower, sense), _, rhs = K.cost_set("mixed 12x16")
    basic = np.zeros(16, dtype=bool); basic[cb.base.basis[cb.base.basis < 16]] = True
    assert basic.any() and not basic.all()
    step = np.where(np.arange(16) % 2 == 0, 2.5, -1.75)
    cs = np.stack([c0 + np.where(basic, step, 0.0), c0 + np.where(~basic, step, 0.0), c0 + np.where(~basic, 1e-12, 0.0)])
    for bs in (None, rhs[:3]):
        refs = K.solve_all(cb, cs, bs)
        assert sum(r.primal_events for r in refs) > 0
        with _open(gpu, "mixed 12x16") as base:
            _equal_ref(base.solve_costs(cs, bs), refs, "basic / nonbasic")


# ---- one batch of 300 scenarios with every status -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mix():
    """300 scenarios of the 12 x 17 batch model, costs moved by integers in [-3, 3] and right-hand sides by integers in [-25, 25):
    more workgroups than compute units.  A negative right-hand side on the first row is INFEASIBLE; a negative cost on the column
    without an upper bound is UNBOUNDED; a NaN in c and an infinity in b refuse their scenarios alone; the same scenario stands at
    0, 255 and 299."""
    model = K.batch_model()
    c0, b0 = model[0], model[3]
    g = np.random.default_rng(78)
    cs = c0 + g.integers(-3, 4, size=(300, 17)).astype(np.float64)
    bs = b0 + g.integers(-25, 25, size=(300, 12)).astype(np.float64)
    cs[:, 16] = np.where(np.arange(300) % 7 == 3, -1.0, cs[:, 16] + 3.0)
    bs[np.arange(300) % 11 == 5, 0] = -1.0                                          # a <= row of positive coefficients over x >= 0
    cs[0] = cs[255] = cs[299] = c0 + np.arange(17.0) % 5 - 2.0
    bs[0] = bs[255] = bs[299] = b0 + np.arange(12.0) - 6.0
    cs[17, 3] = np.nan; bs[200, 11] = INF; cs[201, 0] = -INF
    return model, cs, bs, K.solve_all(K.open_model(model), cs, bs)


def test_batch_of_300_with_every_status(gpu):
    model, cs, bs, refs = _mix()
    count = {s: sum(1 for r in refs if r.status == s) for s in (K.OPTIMAL, K.UNBOUNDED, K.INFEASIBLE, K.EINVAL)}
    assert all(v > 0 for v in count.values()) and sum(count.values()) == 300 and count[K.EINVAL] == 3, count
    assert refs[0].primal_events > 0 and refs[0].dual_events > 0
    with _open_model(gpu, model) as base:
        res = base.solve_costs(cs, bs)
        _equal_ref(res, refs, "the batch")
        bad = res.Status < 0
        assert np.flatnonzero(bad).tolist() == [17, 200, 201]
        for k in ("Solution", "OptimalValue", "Basis", "AtUpper", "Events", "PrimalEvents", "DualEvents", "PrimalCounts", "DualCounts", "Z",
                  "Duals", "ReducedCosts"):
            assert not getattr(res, k)[bad].any(), k
        assert not np.signbit(res.Solution[bad]).any() and not np.signbit(res.Duals[bad]).any()
        for i in (255, 299):                                                        # the position does not matter
            _equal_outputs(res, res, "position %d" % i, rows_a=slice(0, 1), rows_b=slice(i, i + 1))
            assert np.array_equal(res.PrimalCounts[0], res.PrimalCounts[i]) and np.array_equal(res.DualCounts[0], res.DualCounts[i])
        for i in (0, 3, 17, 150, 299):                                              # nor do count and the other scenarios
            _equal_ref(base.solve_costs(cs[i], bs[i]), [refs[i]], "scenario %d alone" % i)
        nob = base.solve_costs(cs[:40])                                             # the same costs without b
        _equal_ref(nob, K.solve_all(K.open_model(model), cs[:40]), "the batch without b")


# ---- raw calls: the iteration limits of either loop, optional outputs, guard bytes ---------------------------------------------
SIZES = lambda count, m, n: {"status": 4 * count, "x": 8 * count * n, "value": 8 * count, "rec": 72 * count, "basis": 4 * count * m,
                             "at_upper": count * n, "y": 8 * count * m, "d": 8 * count * n}
NAMES = ("status", "x", "value", "rec", "basis", "at_upper", "y", "d")


def _raw_solve(lpx, h, cs, bs, m, n, want, long_step=True, p_max_iter=None, d_max_iter=None):
    """lpx_packed_base_solve_costs through ctypes on arrays with 64 guard bytes behind each; returns the arrays (as bytes) and the
    stats.  A limit of None passes NULL options for that loop."""
    Lb = lpx._lib
    GUARD = 64
    count = len(cs)
    sizes = SIZES(count, m, n)
    bufs = {k: np.full(v + GUARD, 0xA5, dtype=np.uint8) for k, v in sizes.items()}
    types = {"status": Lb.ip, "x": Lb.dp, "value": Lb.dp, "rec": C.POINTER(Lb.PackedCostRecord), "basis": Lb.ip,
             "at_upper": C.POINTER(C.c_uint8), "y": Lb.dp, "d": Lb.dp}
    pr = Lb.PackedCostResults(*[C.cast(C.c_void_p(bufs[k].ctypes.data), types[k]) if k in want else None for k in NAMES])
    st = Lb.Stats()
    cs = np.ascontiguousarray(cs); bs = None if bs is None else np.ascontiguousarray(bs)
    op = None if p_max_iter is None else C.byref(Lb.default_opts(False, max_iter=p_max_iter))
    od = None if d_max_iter is None else C.byref(Lb.default_opts(True, max_iter=d_max_iter))
    rc = Lb.lib().lpx_packed_base_solve_costs(h, count, cs.ctypes.data_as(Lb.dp), None if bs is None else bs.ctypes.data_as(Lb.dp),
                                              Lb.BDUAL_LONG_STEP if long_step else 0, op, od, C.byref(pr), C.byref(st))
    assert rc == 0, Lb.last_error()
    for k, v in sizes.items():
        assert (bufs[k][v:] == 0xA5).all(), "guard bytes behind " + k
    return {k: bufs[k][:v].tobytes() for k, v in sizes.items()}, st


def _raw_equal_ref(lpx, full, refs, what):
    rec = np.frombuffer(full["rec"], dtype=lpx.solver.PACKED_COST_DTYPE)
    assert np.frombuffer(full["status"], dtype=np.int32).tolist() == [r.status for r in refs] == rec["status"].tolist(), what
    assert np.array_equal(np.frombuffer(full["x"], dtype=np.uint64), np.concatenate([_u64(r.x) for r in refs])), what
    assert np.array_equal(np.frombuffer(full["value"], dtype=np.uint64), np.array([_u64(r.value) for r in refs]).ravel()), what
    assert np.array_equal(np.frombuffer(full["y"], dtype=np.uint64), np.concatenate([_u64(r.y) for r in refs])), what
    assert np.array_equal(np.frombuffer(full["d"], dtype=np.uint64), np.concatenate([_u64(r.d) for r in refs])), what
    assert np.frombuffer(full["basis"], dtype=np.int32).tolist() == np.concatenate([r.basis for r in refs]).tolist(), what
    assert np.frombuffer(full["at_upper"], dtype=np.uint8).tolist() == np.concatenate([r.at_upper for r in refs]).tolist(), what
    assert rec["primal_events"].tolist() == [r.primal_events for r in refs] and rec["dual_events"].tolist() == [r.dual_events for r in refs], what
    assert [tuple(v) for v in zip(rec["primal_kind0"], rec["primal_kind1"], rec["primal_flips"])] == [r.pcounts for r in refs], what
    assert [tuple(v) for v in zip(rec["dual_kind0"], rec["dual_kind1"], rec["dual_passes"])] == [r.dcounts for r in refs], what
    assert np.array_equal(_u64(rec["z"]), np.array([_u64(r.z) for r in refs]).ravel()) and not rec["pad"].any(), what


@pytest.mark.parametrize("long_step", [True, False])
@pytest.mark.parametrize("which", ["primal", "dual"])
@pytest.mark.parametrize("max_iter", [0, 1, 2])
def test_iteration_limits_are_tested_first_on_either_loop_alone(gpu, max_iter, which, long_step):
    """The limit is tested at the head of a trip.  The primal limit ends the scenario in front of the dual loop; the dual limit
    leaves the primal loop its default; with max_iter = 0 even a scenario that needs no event ends at the limit."""
    cb = K.set_base("covering 12x60", long_step)
    _, cs, rhs = K.cost_set("covering 12x60")
    cs, rhs = cs[:3], rhs[:3]
    kw = {"p_max_iter": max_iter} if which == "primal" else {"d_max_iter": max_iter}
    refs = K.solve_all(cb, cs, rhs, long_step=long_step, **kw)
    assert all(r.status == K.ITER_LIMIT for r in refs[1:]) and (max_iter > 0 or refs[0].status == K.ITER_LIMIT)
    if which == "primal":
        assert all(r.primal_events == max_iter and r.dual_events == 0 for r in refs[1:])
    else:
        assert all(r.primal_events > 2 and r.dual_events >= max_iter for r in refs[1:])
    with _open(gpu, "covering 12x60", long_step) as base:
        full, _ = _raw_solve(gpu, base._h, cs, rhs, 12, 60, NAMES, long_step, **kw)
        _raw_equal_ref(gpu, full, refs, (which, max_iter))
        if which == "dual":                                                         # without b the dual limit has no reader
            full, _ = _raw_solve(gpu, base._h, cs, None, 12, 60, NAMES, long_step, **kw)
            _raw_equal_ref(gpu, full, K.solve_all(cb, cs, None, long_step=long_step), (which, max_iter, "no b"))


def test_python_limits_of_one_loop_alone_and_of_both(gpu):
    """PackedBase.solve_costs: primal_max_iter and dual_max_iter reach one loop each, max_iter both; a base opened with a limit
    hands it to the dual loop only."""
    cb = K.set_base("covering 12x60")
    _, cs, rhs = K.cost_set("covering 12x60")
    cs, rhs = cs[:3], rhs[:3]
    with _open(gpu, "covering 12x60") as base:
        _equal_ref(base.solve_costs(cs, rhs, primal_max_iter=2), K.solve_all(cb, cs, rhs, p_max_iter=2), "primal alone")
        _equal_ref(base.solve_costs(cs, rhs, dual_max_iter=2), K.solve_all(cb, cs, rhs, d_max_iter=2), "dual alone")
        _equal_ref(base.solve_costs(cs, rhs, max_iter=3), K.solve_all(cb, cs, rhs, p_max_iter=3, d_max_iter=3), "both")
        _equal_ref(base.solve_costs(cs, rhs, max_iter=3, primal_max_iter=50), K.solve_all(cb, cs, rhs, p_max_iter=50, d_max_iter=3), "one in front")
    with _open(gpu, "covering 12x60", max_iter=500) as base:                         # enough for the base; the dual loop's alone
        _equal_ref(base.solve_costs(cs, rhs), K.solve_all(cb, cs, rhs, d_max_iter=500), "the base's limit")
        _equal_ref(base.solve_costs(cs, rhs, dual_max_iter=1), K.solve_all(cb, cs, rhs, d_max_iter=1), "the base's limit overridden")


def test_optional_outputs_guard_bytes_and_stats(gpu):
    _, cs, rhs = K.cost_set("covering 6x12")
    refs = K.set_refs("covering 6x12", True, True)
    required = ("status", "x", "value")
    optional = ("rec", "basis", "at_upper", "y", "d")
    with _open(gpu, "covering 6x12") as base:
        full, st = _raw_solve(gpu, base._h, cs, rhs, 6, 12, required + optional)
        lean, st2 = _raw_solve(gpu, base._h, cs, rhs, 6, 12, required)
        some, st3 = _raw_solve(gpu, base._h, cs, rhs, 6, 12, required + ("rec", "d"))
        nob, st4 = _raw_solve(gpu, base._h, cs, None, 6, 12, required + optional)
    for k in required:
        assert full[k] == lean[k] == some[k], k
    for k in optional:                                                              # NULL: not written at all
        assert lean[k] == b"\xa5" * len(lean[k]), k
        assert some[k] == (full[k] if k in ("rec", "d") else b"\xa5" * len(some[k])), k
    _raw_equal_ref(gpu, full, refs, "with b")
    _raw_equal_ref(gpu, nob, K.set_refs("covering 6x12", True, False), "without b")
    pivots = sum(sum(r.pcounts[:2]) + sum(r.dcounts[:2]) for r in refs)
    for s in (st, st2, st3):
        assert s.launches == 1 and s.pivots == pivots and s.loop_ms > 0.0
    assert st4.launches == 1


# ---- handles and the arena, shared with the other packed calls ----------------------------------------------------------------
def test_two_handles_interleaved_and_both_calls_interleaved_on_one_handle(gpu):
    """Two bases open at once, their cost solves interleaved; a larger solve after a smaller one (the arena grows); a solve and
    a solve_costs interleaved on one handle; the handle unchanged afterwards: solve(b0) still equals Base."""
    refs_a, refs_b = K.set_refs("covering 6x12", True, True), K.set_refs("mixed 12x16", True, False)
    (_, cs_a, rhs_a), (_, cs_b, _) = K.cost_set("covering 6x12"), K.cost_set("mixed 12x16")
    warm_b = W.set_refs("mixed 12x16", True)
    bs_b = W.scenario_set("mixed 12x16")[1]
    a, b = _open(gpu, "covering 6x12"), _open(gpu, "mixed 12x16")
    try:
        _equal_ref(a.solve_costs(cs_a, rhs_a), refs_a, "a first")
        _equal_ref(b.solve_costs(cs_b), refs_b, "b first")
        reps = 400                                                                  # 3200 scenarios: well beyond the first arena
        big = a.solve_costs(np.tile(cs_a, (reps, 1)), np.tile(rhs_a, (reps, 1)))
        for k in range(len(refs_a)):
            sel = slice(k, None, len(refs_a))
            assert (big.Status[sel] == refs_a[k].status).all() and (_u64(big.Solution[sel]) == _u64(refs_a[k].x)).all()
            assert (_u64(big.OptimalValue[sel]) == _u64(refs_a[k].value)).all() and (big.Basis[sel] == refs_a[k].basis).all()
            assert (big.PrimalCounts[sel] == np.array(refs_a[k].pcounts)).all() and (big.DualCounts[sel] == np.array(refs_a[k].dcounts)).all()
            assert (_u64(big.Duals[sel]) == _u64(refs_a[k].y)).all()
        _equal_ref(b.solve_costs(cs_b), refs_b, "b after the large solve of a")
        rhs_only = b.solve(bs_b)                                                    # the right-hand-side call between two cost calls
        assert rhs_only.Status.tolist() == [r.status for r in warm_b]
        for i, r in enumerate(warm_b):
            assert np.array_equal(_u64(rhs_only.Solution[i]), _u64(r.x)) and _u64(rhs_only.OptimalValue[i]) == _u64(r.value)
        _equal_ref(b.solve_costs(cs_b), refs_b, "b after its own solve")
        _equal_outputs(b.solve(bs_b[0]), b.Base, "solve(b0) still equals Base")
        a.close()
        with pytest.raises(gpu.SolverException):
            a.solve_costs(cs_a)
        _equal_ref(b.solve_costs(cs_b), refs_b, "b after a was closed")
    finally:
        a.close(); b.close()


# ---- the command line: a fresh child process per call ---------------------------------------------------------------------------
def test_cli_cost_file_equals_solve_costs(gpu, tmp_path):
    c, A, rel, b, upper = P.hand_model()
    model = tmp_path / "hand.txt"
    model.write_text("Min: 2x1 + 3x2 + 1x3\n1x1 + 1x2 + 1x3 >= 4\n1x1 - 1x2 + 2x3 <= 3\n")
    costs = ["2 3 1", "1 4 -2", "3.5 0.25 1"]
    rhs = ["4 3", "7 3", "9 3"]                                                     # the last: more than the bounds can cover
    f = tmp_path / "costs.txt"; f.write_text("".join(line + "\n" for line in costs))
    g = tmp_path / "rhs.txt"; g.write_text("".join(line + "\n" for line in rhs))
    short = tmp_path / "short.txt"; short.write_text("4 3\n7 3\n")
    cs = np.array([[float(v) for v in row.split()] for row in costs])
    bs = np.array([[float(v) for v in row.split()] for row in rhs])
    exe = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
    bounds = ("--upper", "1=3", "--upper", "2=3", "--upper", "3=2")
    cb = K.open_base(c, A, b, rel, np.zeros(3), upper, P.MIN)
    for extra, bsel in (((), None), (("--rhs-file", str(g)), bs)):
        out = subprocess.run([exe, "--bounded-dual", "--long-step", "--warm-base", "--cost-file", str(f), *extra, *bounds, str(model)],
                             check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
        assert len(out) == len(costs)
        with gpu.LPSolver().OpenPackedBase(c, A, b, rel, upper, np.zeros(3), "min") as base:      # the CLI passes both bound arrays
            res = base.solve_costs(cs, bsel)
        _equal_ref(res, K.solve_all(cb, cs, bsel), "hand")
        for i, line in enumerate(out):
            got = line.split()
            assert int(got[0]) == res.Status[i] and float(got[1]) == res.OptimalValue[i], (i, line)
            assert [float(v) for v in got[2:]] == res.Solution[i].tolist(), (i, line)
        assert res.Status[0] == K.OPTIMAL and (bsel is None or res.Status[-1] == K.INFEASIBLE)
    refused = subprocess.run([exe, "--bounded-dual", "--warm-base", "--cost-file", str(f), "--rhs-file", str(short), *bounds, str(model)],
                             capture_output=True, text=True, timeout=120)
    assert refused.returncode == 65 and "--cost-file holds 3 lines and --rhs-file holds 2" in refused.stderr
    refused = subprocess.run([exe, "--bounded-dual", "--cost-file", str(f), str(model)], capture_output=True, text=True, timeout=120)
    assert refused.returncode == 64 and "--cost-file needs --bounded-dual --warm-base" in refused.stderr
    refused = subprocess.run([exe, "--bounded-dual", "--warm-base", str(model)], capture_output=True, text=True, timeout=120)
    assert refused.returncode == 64 and "--bounded-dual --warm-base needs --rhs-file or --cost-file" in refused.stderr
    empty = tmp_path / "empty.txt"; empty.write_text("\n")
    refused = subprocess.run([exe, "--bounded-dual", "--warm-base", "--cost-file", str(empty), *bounds, str(model)],
                             capture_output=True, text=True, timeout=120)
    assert refused.returncode == 65 and "--cost-file holds no cost vector" in refused.stderr
