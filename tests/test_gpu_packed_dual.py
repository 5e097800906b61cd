"""GPU tests of the packed batch call by a dual start (lpx_solve_packed_dual, LPSolver.SolvePackedDual; kernel in
csrc/lpx_packed_dual.hip).  Every comparison is bit for bit (np.uint64 views of the doubles): against the NumPy restatement of the
contract (tests/_packed_dual_ref.py) and, for the models the model-level call accepts, against SolveBoundedDual of each model.
The instances and the restatement's answers are shared with tests/test_packed_dual_ref.py, which asserts on the CPU that they make
kind-0 pivots, kind-1 pivots, passes and dualize flips and end INFEASIBLE, each at least once."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _bounded_long_ref as L
import _packed_dual_ref as P
import _packed_ref as PP

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


def _equal_results(a, b, what=""):
    assert a.Status.tolist() == b.Status.tolist(), what
    for k in ("Solution", "OptimalValue", "Z", "Duals", "ReducedCosts"):
        assert np.array_equal(_u64(getattr(a, k)), _u64(getattr(b, k))), (what, k)
    for k in ("BoundCounts", "Events", "Passes", "DualizeFlips", "Basis", "AtUpper"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), (what, k)


def _equal_single(lpx, res, i, c, A, rel, b, upper, lower, sense, long_step):
    """Entry i against the model-level dual start of that model (its launches form)."""
    p = lpx.LPProblem.from_arrays(sense, c, A, [int(r) for r in rel], b)
    try:
        one = lpx.LPSolver().SolveBoundedDual(p, INF if upper is None else upper, lower, long_step=long_step)
    except lpx.SolverException as e:
        assert res.Status[i] == e.code < 0
        return
    assert res.Status[i] == one.Status
    assert np.array_equal(_u64(res.Solution[i]), _u64(one.Solution)) and _u64(res.OptimalValue[i]) == _u64(one.OptimalValue)
    assert tuple(res.BoundCounts[i].tolist()) == one.BoundCounts
    assert res.Basis[i].tolist() == one.Basis.tolist() and res.AtUpper[i].tolist() == one.AtUpper.tolist()


# ---- the shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_step", [True, False])
@pytest.mark.parametrize("name", list(P.SHAPES))
def test_shapes_equal_the_restatement_and_the_single_solves(gpu, name, long_step):
    c, A, rel, b, upper, lower, sense = P.shape(name)
    refs = P.shape_refs(name, long_step)
    m, n = A.shape[1:]
    assert gpu._lib.lib().lpx_packed_fits(m, n) == 1
    res = gpu.LPSolver().SolvePackedDual(c, A, b, rel, upper, lower, SENSE[sense], long_step)
    _equal_ref(res, refs, name)
    for i in range(len(refs)):
        _equal_single(gpu, res, i, c[i], A[i], rel[i], b[i], upper, lower, sense, long_step)
    assert res.Stats["launches"] == 1 and res.Stats["pivots"] == sum(r.counts[0] + r.counts[1] for r in refs)


def test_the_last_m_that_fits(gpu):
    fits = gpu._lib.lib().lpx_packed_fits
    assert fits(139, 1) == 1 and fits(140, 1) == 0
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver().SolvePackedDual(np.ones(1), np.ones((140, 1)), np.ones((2, 140)), upper=1.0)
    assert e.value.code == gpu._lib.EINVAL and "141 x 142" in str(e.value) and "does not fit" in str(e.value)


# ---- row negation edges ------------------------------------------------------------------------------------------------------
def test_a_shared_rel_gives_the_bits_of_a_tiled_one(gpu):
    c, A, rel, b, upper, lower, sense = P.shape("mixed 12x16")
    S = gpu.LPSolver()
    shared = S.SolvePackedDual(c[:2], A[0], b[:2], rel[0], upper, lower, SENSE[sense])             # rel[0] == rel[1]
    tiled = S.SolvePackedDual(c[:2], A[:2], b[:2], rel[:2], np.tile(upper, (2, 1)), np.tile(lower, (2, 1)), SENSE[sense])
    _equal_results(shared, tiled, "shared against tiled")
    _equal_ref(shared, P.shape_refs("mixed 12x16", True)[:2], "shared")
    strings = S.SolvePackedDual(c[:2], A[0], b[:2], np.where(rel[0] == P.GE, ">=", "<="), upper, lower, SENSE[sense])
    _equal_results(shared, strings, "rel as strings")
    none = S.SolvePackedDual(c[:2], np.where((rel[0] == P.GE)[:, None], -A[0], A[0]), np.where(rel[0] == P.GE, -b[:2], b[:2]),
                             None, upper, lower, SENSE[sense])                                     # rel = NULL: every row <=
    assert none.Status.tolist() == shared.Status.tolist() and np.array_equal(_u64(none.Solution), _u64(shared.Solution))


def test_a_ge_row_equals_the_negated_le_row_except_for_the_sign_of_its_dual(gpu):
    c, A, rel, b, upper, lower, sense = P.shape("mixed 12x16")
    ge = rel[0] == P.GE
    S = gpu.LPSolver()
    as_given = S.SolvePackedDual(c[0], A[0], b[0], rel[0], upper, lower, SENSE[sense])
    negated = S.SolvePackedDual(c[0], np.where(ge[:, None], -A[0], A[0]), np.where(ge, -b[0], b[0]), np.zeros(12, dtype=np.int32),
                                upper, lower, SENSE[sense])
    for k in ("Solution", "OptimalValue", "Z", "ReducedCosts"):
        assert np.array_equal(_u64(getattr(as_given, k)), _u64(getattr(negated, k))), k
    for k in ("Status", "BoundCounts", "Events", "DualizeFlips", "Basis", "AtUpper"):
        assert np.array_equal(getattr(as_given, k), getattr(negated, k)), k
    assert np.array_equal(_u64(as_given.Duals[0][~ge]), _u64(negated.Duals[0][~ge]))
    assert np.array_equal(_u64(as_given.Duals[0][ge]), _u64(-negated.Duals[0][ge])) and as_given.Duals[0][ge].any()


def test_a_zero_coefficient_in_a_ge_row(gpu):
    """It becomes -0.0 in the tableau; the restatement negates the same way, and the bits agree."""
    c, A, rel, b, upper = P.hand_model()
    A = A.copy(); A[0, 1] = 0.0                         # x1 + 0 x2 + x3 >= 4
    ref = P.solve(c, A, b, rel, None, upper, P.MIN)
    assert ref.status == P.OPTIMAL and ref.events > 0
    res = gpu.LPSolver().SolvePackedDual(c, A, b, rel, upper, sense="min")
    _equal_ref(res, [ref], "zero coefficient")
    _equal_single(gpu, res, 0, c, A, rel, b, upper, None, P.MIN, True)


def test_a_zero_lower_bound_turns_minus_zero_into_plus_zero(gpu):
    """Min x1 + 2 x2, x1 + x2 >= 1, x1 <= -0.0, x2 <= 5.  The long step passes x1 (its ratio is the least, and a flip by its
    upper bound -0.0 leaves the row violated), so x1 ends nonbasic at its upper bound: x1 = ub - 0.0 = -0.0.  Without a lower array
    it comes back as it is; with lower = (0, 0) the host path adds +0.0 and so does the kernel."""
    c, A, rel, b = np.array([1.0, 2.0]), np.array([[1.0, 1.0]]), np.array([P.GE], dtype=np.int32), np.array([1.0])
    upper = np.array([-0.0, 5.0])
    ref = P.solve(c, A, b, rel, None, upper, P.MIN)
    assert ref.status == P.OPTIMAL and ref.counts == (1, 0, 1) and np.signbit(ref.x[0]) and ref.x.tolist() == [0.0, 1.0]
    ref0 = P.solve(c, A, b, rel, np.zeros(2), upper, P.MIN)
    assert not np.signbit(ref0.x).any() and ref0.at_upper.tolist() == [1, 0]
    S = gpu.LPSolver()
    res = S.SolvePackedDual(c, A, b, rel, upper, sense="min")
    _equal_ref(res, [ref], "no lower")
    _equal_single(gpu, res, 0, c, A, rel, b, upper, None, P.MIN, True)
    res0 = S.SolvePackedDual(c, A, b, rel, upper, lower=np.zeros(2), sense="min")
    _equal_ref(res0, [ref0], "zero lower")
    _equal_single(gpu, res0, 0, c, A, rel, b, upper, np.zeros(2), P.MIN, True)
    assert np.signbit(res.Solution[0, 0]) and not np.signbit(res0.Solution).any()


# ---- one batch of 300 models of 12 x 60 with every status -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mix():
    """300 covering models of 12 x 60 from 30 seeds, more workgroups than compute units.  By index: models that nothing can cover
    (INFEASIBLE), an upper bound below its lower bound, a rel entry that is neither <= nor >=, a negative cost on a variable
    without an upper bound (the precheck), and all three defects in one model.  max_iter = 53 lies inside the range of the event
    counts of the seeds, so it stops some models and not others."""
    W, m, n = 300, 12, 60
    base = [L.covering_model(m, n, s) for s in range(1, 31)]
    c, A, rel, b = (np.stack([base[i % 30][k] for i in range(W)]) for k in range(4))
    c, b, rel = c.copy(), b.copy(), rel.copy()
    upper = np.ones((W, n))
    for i in range(W):
        k = i % 10
        if k == 1:
            b[i] = 1.5 * A[i].sum(axis=1)
        if k == 3 or i % 20 == 9:
            upper[i, 2] = -1.0
        if k == 5 or i % 20 == 9:
            rel[i, 4] = 2
        if k == 7 or i % 20 == 9:
            c[i, 0] = -1.0; upper[i, 0] = INF
    max_iter = 53
    return (c, A, rel, b, upper, max_iter), P.solve_all(c, A, b, rel, None, upper, P.MIN, max_iter=max_iter)


def test_batch_of_300_with_every_status(gpu):
    (c, A, rel, b, upper, max_iter), refs = _mix()
    count = {s: sum(1 for r in refs if r.status == s) for s in (P.OPTIMAL, P.INFEASIBLE, P.ITER_LIMIT, P.EINVAL)}
    assert all(v > 0 for v in count.values()) and sum(count.values()) == 300, count
    assert {r.why for r in refs} == {"", "bound", "rel", "precheck"} and refs[9].why == "bound"
    S = gpu.LPSolver()
    res = S.SolvePackedDual(c, A, b, rel, upper, sense="min", max_iter=max_iter)
    _equal_ref(res, refs, "the batch")
    assert res.Stats["launches"] == 1 and res.Stats["pivots"] == sum(r.counts[0] + r.counts[1] for r in refs)
    bad = res.Status < 0                                                            # refused models: zeroed outputs
    assert bad.sum() == count[P.EINVAL]
    for k in ("Solution", "OptimalValue", "Basis", "AtUpper", "Events", "BoundCounts", "DualizeFlips", "Z", "Duals", "ReducedCosts"):
        assert not getattr(res, k)[bad].any(), k
    assert not np.signbit(res.Solution[bad]).any() and not np.signbit(res.Duals[bad]).any()
    for i in range(300):                                                            # every model equals its own count = 1 call
        one = S.SolvePackedDual(c[i], A[i], b[i], rel[i:i + 1], upper[i], sense="min", max_iter=max_iter)
        _equal_ref(one, [refs[i]], "model %d alone" % i)
    for i in (0, 1, 3, 7):                                                          # and the model-level call, where that one answers
        if refs[i].status != P.ITER_LIMIT:
            _equal_single(gpu, res, i, c[i], A[i], rel[i], b[i], upper[i], None, P.MIN, True)


# ---- the iteration limit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_step", [True, False])
@pytest.mark.parametrize("max_iter", [0, 1, 2])
def test_iteration_limit_is_tested_first(gpu, max_iter, long_step):
    """The limit is tested at the head of a trip: a trip that starts below it may pass it by its passes."""
    c, A, rel, b = L.covering_model(6, 12, 1)
    ref = P.solve(c, A, b, rel, None, 1.0, P.MIN, long_step=long_step, max_iter=max_iter)
    assert ref.status == P.ITER_LIMIT and (ref.events >= max_iter) and (max_iter > 0 or ref.events == 0)
    res = gpu.LPSolver().SolvePackedDual(c, A, b, rel, 1.0, sense="min", long_step=long_step, max_iter=max_iter)
    _equal_ref(res, [ref], "max_iter %d" % max_iter)
    if max_iter > 0:                                                                # (the engine option 0 means the default limit)
        with pytest.raises(gpu.SolverException) as e:                               # the model-level call returns an error there
            gpu.LPSolver(max_iter=max_iter).SolveBoundedDual(gpu.LPProblem.from_arrays(1, c, A, [1] * 6, b), 1.0, long_step=long_step)
        assert e.value.code == P.ITER_LIMIT


# ---- optional outputs, guard bytes, stats -------------------------------------------------------------------------------------
SIZES = lambda count, m, n: {"status": 4 * count, "x": 8 * count * n, "value": 8 * count, "rec": 48 * count, "basis": 4 * count * m,
                             "at_upper": count * n, "y": 8 * count * m, "d": 8 * count * n}


def _raw_call(lpx, c, A, rel, b, upper, sense, want):
    """lpx_solve_packed_dual through ctypes on arrays with 64 guard bytes behind each; returns the arrays (as bytes) and the stats."""
    Lb = lpx._lib
    count, m, n = A.shape
    GUARD = 64
    sizes = SIZES(count, m, n)
    bufs = {k: np.full(v + GUARD, 0xA5, dtype=np.uint8) for k, v in sizes.items()}
    up = np.ascontiguousarray(np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,)))
    pm = Lb.PackedDualModels(count, m, n, sense, c.ctypes.data_as(Lb.dp), A.ctypes.data_as(Lb.dp), b.ctypes.data_as(Lb.dp), None,
                             up.ctypes.data_as(Lb.dp), n, m * n, m, 0, 0, rel.ctypes.data_as(Lb.ip), m)
    types = {"status": Lb.ip, "x": Lb.dp, "value": Lb.dp, "rec": C.POINTER(Lb.PackedDualRecord), "basis": Lb.ip,
             "at_upper": C.POINTER(C.c_uint8), "y": Lb.dp, "d": Lb.dp}
    ptr = lambda k: C.cast(C.c_void_p(bufs[k].ctypes.data), types[k]) if k in want else None
    pr = Lb.PackedDualResults(*[ptr(k) for k in ("status", "x", "value", "rec", "basis", "at_upper", "y", "d")])
    st = Lb.Stats()
    assert Lb.lib().lpx_solve_packed_dual(C.byref(pm), Lb.BDUAL_LONG_STEP, None, C.byref(pr), C.byref(st)) == 0, Lb.last_error()
    for k, v in sizes.items():
        assert (bufs[k][v:] == 0xA5).all(), "guard bytes behind " + k
    return {k: bufs[k][:v].tobytes() for k, v in sizes.items()}, st


def test_optional_outputs_guard_bytes_and_stats(gpu):
    c, A, rel, b, upper, lower, sense = P.shape("covering 6x12")
    refs = P.shape_refs("covering 6x12", True)
    c, A, rel, b = (np.ascontiguousarray(v) for v in (c, A, rel, b))
    required = ("status", "x", "value")
    full, st = _raw_call(gpu, c, A, rel, b, upper, sense, required + ("rec", "basis", "at_upper", "y", "d"))
    lean, st2 = _raw_call(gpu, c, A, rel, b, upper, sense, required)
    some, st3 = _raw_call(gpu, c, A, rel, b, upper, sense, required + ("basis", "y"))
    for k in required:
        assert full[k] == lean[k] == some[k], k
    for k in ("rec", "basis", "at_upper", "y", "d"):                                # NULL: not written at all
        assert lean[k] == b"\xa5" * len(lean[k]), k
        assert some[k] == (full[k] if k in ("basis", "y") else b"\xa5" * len(some[k])), k
    assert np.frombuffer(full["status"], dtype=np.int32).tolist() == [r.status for r in refs]
    assert np.array_equal(np.frombuffer(full["x"], dtype=np.uint64), np.concatenate([_u64(r.x) for r in refs]))
    assert np.array_equal(np.frombuffer(full["y"], dtype=np.uint64), np.concatenate([_u64(r.y) for r in refs]))
    assert np.array_equal(np.frombuffer(full["d"], dtype=np.uint64), np.concatenate([_u64(r.d) for r in refs]))
    assert np.frombuffer(full["basis"], dtype=np.int32).tolist() == np.concatenate([r.basis for r in refs]).tolist()
    assert np.frombuffer(full["at_upper"], dtype=np.uint8).tolist() == np.concatenate([r.at_upper for r in refs]).tolist()
    pivots = sum(r.counts[0] + r.counts[1] for r in refs)
    for s in (st, st2, st3):
        assert s.launches == 1 and s.pivots == pivots and s.loop_ms > 0.0
    res = gpu.LPSolver().SolvePackedDual(c, A, b, rel, upper, sense="min", want=())                # the Python face of the lean call
    assert res.Basis is None and res.AtUpper is None and res.Events is None and res.Duals is None and res.ReducedCosts is None
    assert res.Solution.tobytes() == full["x"] and res.OptimalValue.tobytes() == full["value"]


# ---- the arena, shared with lpx_solve_packed --------------------------------------------------------------------------------
def test_a_larger_call_after_a_smaller_one_and_a_primal_call_between_two(gpu):
    """The device buffers are kept between calls, grown when needed, and are those of lpx_solve_packed: small, large, a packed
    primal call, small again -- the same bits each time, and the primal call gives its own."""
    c, A, rel, b, upper, lower, sense = P.shape("covering 6x12")
    refs = P.shape_refs("covering 6x12", True)
    S = gpu.LPSolver()
    first = S.SolvePackedDual(c, A, b, rel, upper, sense="min")
    reps = 600                                                                      # 2400 models: well beyond the first arena
    big = S.SolvePackedDual(np.tile(c, (reps, 1)), np.tile(A, (reps, 1, 1)), np.tile(b, (reps, 1)), rel[0], upper, sense="min")
    import _bounded_ref as B
    pc, pA, pb = (np.stack([B.binary_bounded(12, 6, s)[3][k] for s in (1, 2, 3)]) for k in range(3))
    primal = S.SolvePacked(pc, pA, pb, 1.0)
    again = S.SolvePackedDual(c, A, b, rel, upper, sense="min")
    _equal_ref(first, refs, "first"); _equal_results(first, again, "again")
    for k in range(len(refs)):
        sel = slice(k, None, len(refs))
        assert (big.Status[sel] == refs[k].status).all() and (_u64(big.Solution[sel]) == _u64(refs[k].x)).all()
        assert (_u64(big.OptimalValue[sel]) == _u64(refs[k].value)).all() and (big.Basis[sel] == refs[k].basis).all()
        assert (big.BoundCounts[sel] == np.array(refs[k].counts)).all() and (_u64(big.Duals[sel]) == _u64(refs[k].y)).all()
    for i, r in enumerate(PP.solve_all(pc, pA, pb, None, 1.0)):                     # the bits of the packed primal call
        assert primal.Status[i] == r.status and np.array_equal(_u64(primal.Solution[i]), _u64(r.x))
        assert _u64(primal.OptimalValue[i]) == _u64(r.value) and primal.Basis[i].tolist() == r.basis.tolist()
        assert tuple(primal.BoundCounts[i].tolist()) == r.counts


# ---- the command line: a fresh child process per call ---------------------------------------------------------------------------
def test_cli_bounded_dual_rhs_file_equals_single_solves(gpu, tmp_path):
    c, A, rel, b, upper = P.hand_model()
    model = tmp_path / "hand.txt"
    model.write_text("Min: 2x1 + 3x2 + 1x3\n1x1 + 1x2 + 1x3 >= 4\n1x1 - 1x2 + 2x3 <= 3\n")
    rhs = ["4 3", "5 3", "3 4", "-1 3", "9 3"]                                      # the last: more than the bounds can cover
    f = tmp_path / "rhs.txt"
    f.write_text("".join(line + "\n" for line in rhs))
    exe = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
    bounds = ("--upper", "1=3", "--upper", "2=3", "--upper", "3=2")
    for flags, long_step in ((("--long-step",), True), ((), False)):
        out = subprocess.run([exe, "--bounded-dual", *flags, "--rhs-file", str(f), *bounds, str(model)],
                             check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
        assert len(out) == len(rhs)
        statuses = []
        for line, row in zip(out, rhs):
            bi = np.array([float(v) for v in row.split()])
            ref = P.solve(c, A, bi, rel, np.zeros(3), upper, P.MIN, long_step=long_step)        # the CLI always passes both bound arrays
            got = line.split()
            assert int(got[0]) == ref.status and float(got[1]) == ref.value and [float(v) for v in got[2:]] == ref.x.tolist()
            statuses.append(ref.status)
            one = gpu.LPSolver().SolveBoundedDual(gpu.LPProblem.from_arrays(1, c, A, [1, 0], bi), upper, np.zeros(3), long_step=long_step)
            assert int(got[0]) == one.Status and float(got[1]) == one.OptimalValue and [float(v) for v in got[2:]] == one.Solution.tolist()
        assert statuses[0] == P.OPTIMAL and statuses[-1] == P.INFEASIBLE
    eq = tmp_path / "eq.txt"
    eq.write_text("Max: 1x1 + 1x2\n1x1 + 1x2 = 2\n")
    one_rhs = tmp_path / "one.txt"
    one_rhs.write_text("2\n")
    refused = subprocess.run([exe, "--bounded-dual", "--rhs-file", str(one_rhs), str(eq)], capture_output=True, text=True, timeout=120)
    assert refused.returncode == 65 and "= constraint is not accepted" in refused.stderr
