"""GPU tests of the packed batch call (lpx_solve_packed, LPSolver.SolvePacked; kernel in csrc/lpx_packed.hip).  Every comparison
is bit for bit (np.uint64 views of the doubles): against the NumPy restatement of the contract (tests/_packed_ref.py around
tests/_bounded_ref.py) and against SolveBounded(form="onchip") of each model.  The event kinds of every instance (kind-0 pivots,
kind-1 pivots, flips) are counted by the restatement on the CPU and pinned beside it."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _bounded_ref as B
import _packed_ref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
SEEDS = (1, 2, 3)


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _stack(models):
    return tuple(np.stack([mdl[k] for mdl in models]) for k in range(3))


def _hand_variants():
    """The hand example of _bounded_ref has no seed: its three models differ in their right-hand sides."""
    c, A, b = B.hand_example()[3]
    return [(c, A, b + np.array(d)) for d in ((0.0, 0.0), (1.0, 0.0), (-1.0, -1.0))]


# name -> (the three models (c, A, b), upper, the kinds the restatement counts for each); every row <=, Max
SHAPES = {
    "2x3": (lambda: [B.dense_unit_bounded(1, 1, s)[3] for s in SEEDS], 1.0, [(0, 0, 1), (1, 0, 0), (0, 0, 1)]),
    "hand 3x6": (_hand_variants, np.array([4.0, 3.0, 3.0]), [(1, 1, 1), (1, 1, 1), (1, 1, 1)]),
    "7x19": (lambda: [B.binary_bounded(12, 6, s)[3] for s in SEEDS], 1.0, [(5, 1, 4), (3, 1, 5), (3, 2, 4)]),            # C odd
    "21x61": (lambda: [B.binary_bounded(40, 20, s)[3] for s in SEEDS], 1.0, [(11, 3, 17), (9, 2, 16), (14, 3, 16)]),      # more rows than waves
    "16x1116": (lambda: [B.dense_unit_bounded(15, 1100, s)[3] for s in SEEDS], 1.0,
                [(26, 97, 992), (15, 77, 1004), (27, 86, 1006)]),                      # C even, every column loop wraps past 1024 lanes
    "101x121": (lambda: [B.binary_bounded(20, 100, s)[3] for s in SEEDS], 1.0, [(24, 1, 6), (15, 1, 6), (26, 2, 5)]),     # tall
    "140x141": (lambda: [B.dense_unit_bounded(139, 1, s)[3] for s in SEEDS], 1.0, [(1, 0, 0), (1, 0, 0), (1, 0, 0)]),     # the last shape that fits
}


@functools.lru_cache(maxsize=None)
def _shape(name):
    """The stacked arrays of a shape and the restatement's answers, computed once and shared (nothing writes them)."""
    build, upper, _ = SHAPES[name]
    c, A, b = _stack(build())
    return (c, A, b, upper), P.solve_all(c, A, b, None, upper)


def _equal_ref(res, refs, what=""):
    """A PackedResult against the restatement's list, every output bit for bit."""
    assert res.Status.tolist() == [r.status for r in refs], what
    for i, r in enumerate(refs):
        assert np.array_equal(_u64(res.Solution[i]), _u64(r.x)), (what, i)
        assert _u64(res.OptimalValue[i]) == _u64(r.value), (what, i)
        assert tuple(res.BoundCounts[i].tolist()) == r.counts and res.Events[i] == r.events, (what, i)
        assert _u64(res.Z[i]) == _u64(r.z), (what, i)
        assert res.Basis[i].tolist() == r.basis.tolist() and res.AtUpper[i].tolist() == r.at_upper.tolist(), (what, i)


def _equal_results(a, b, what=""):
    assert a.Status.tolist() == b.Status.tolist(), what
    assert np.array_equal(_u64(a.Solution), _u64(b.Solution)) and np.array_equal(_u64(a.OptimalValue), _u64(b.OptimalValue)), what
    assert np.array_equal(a.BoundCounts, b.BoundCounts) and np.array_equal(a.Events, b.Events) and np.array_equal(_u64(a.Z), _u64(b.Z)), what
    assert np.array_equal(a.Basis, b.Basis) and np.array_equal(a.AtUpper, b.AtUpper), what


def _equal_single(lpx, res, i, c, A, b, upper, lower, sense):
    """Entry i against the model-level on-chip solve of that model."""
    m, n = A.shape
    p = lpx.LPProblem.from_arrays(sense, c, A, [0] * m, b)
    try:
        one = lpx.LPSolver().SolveBounded(p, upper, lower, form="onchip")
    except lpx.SolverException as e:
        assert res.Status[i] == e.code < 0
        return
    assert res.Status[i] == one.Status
    assert np.array_equal(_u64(res.Solution[i]), _u64(one.Solution)) and _u64(res.OptimalValue[i]) == _u64(one.OptimalValue)
    assert tuple(res.BoundCounts[i].tolist()) == one.BoundCounts
    assert res.Basis[i].tolist() == one.Basis.tolist() and res.AtUpper[i].tolist() == one.AtUpper.tolist()


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_equal_the_restatement_and_the_single_solves(gpu, name):
    (c, A, b, upper), refs = _shape(name)
    assert [r.counts for r in refs] == SHAPES[name][2] and all(r.status == B.OPTIMAL for r in refs)
    m, n = A.shape[1:]
    assert gpu._lib.lib().lpx_packed_fits(m, n) == 1
    res = gpu.LPSolver().SolvePacked(c, A, b, upper)
    _equal_ref(res, refs, name)
    for i in range(3):
        _equal_single(gpu, res, i, c[i], A[i], b[i], upper, None, 0)
    assert res.Stats["launches"] == 1 and res.Stats["pivots"] == sum(r.counts[0] + r.counts[1] for r in refs)


def test_all_three_event_kinds_are_exercised():
    for name in ("7x19", "21x61", "16x1116"):
        assert all(min(k) > 0 for k in SHAPES[name][2]), name


def test_the_last_shape_that_fits(gpu):
    fits = gpu._lib.lib().lpx_packed_fits
    assert fits(139, 1) == 1 and fits(140, 1) == 0
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver().SolvePacked(np.ones(1), np.ones((140, 1)), np.ones((2, 140)), 1.0)
    assert e.value.code == gpu._lib.EINVAL and "141 x 142" in str(e.value) and "does not fit" in str(e.value)


# ---- preparation edges on 7 x 19 ------------------------------------------------------------------------------------------
def _edges():
    """name -> (c, lower, upper, sense, the kinds the restatement counts); A and b are those of binary_bounded(12, 6, 1)."""
    c, A, b = B.binary_bounded(12, 6, 1)[3]
    n = 12
    zero_neg = c.copy(); zero_neg[1] = 0.0; zero_neg[4] = -3.0
    mixed = np.zeros(n); mixed[0] = -0.5; mixed[3] = 0.25; mixed[7] = 0.5          # negative, zero and positive lower bounds
    fixed_lo = np.zeros(n); fixed_lo[2] = 1.0; fixed_lo[5] = 0.5
    fixed_up = np.ones(n); fixed_up[5] = 0.5                                        # x3 = 1 and x6 = 0.5 are fixed
    some_inf = np.ones(n); some_inf[::3] = INF
    return (A, b), {
        "min": (-c, None, np.ones(n), 1, (5, 1, 4)),
        "zero and negative cost": (zero_neg, None, np.ones(n), 0, (2, 1, 5)),
        "mixed lower": (c, mixed, mixed + 1.0, 0, (4, 1, 4)),
        "lower all zero": (c, np.zeros(n), np.ones(n), 0, (5, 1, 4)),
        "fixed": (c, fixed_lo, fixed_up, 0, (4, 2, 4)),
        "infinite upper": (c, None, some_inf, 0, (9, 1, 3)),
        "no bounds": (c, None, None, 0, None),
        "lower only": (c, mixed, None, 0, None),
    }


@pytest.mark.parametrize("name", ["min", "zero and negative cost", "mixed lower", "lower all zero", "fixed", "infinite upper", "no bounds",
                                  "lower only"])
def test_preparation_edges(gpu, name):
    (A, b), cases = _edges()
    c, lower, upper, sense, kinds = cases[name]
    ref = P.solve(c, A, b, lower, upper, sense)
    assert ref.status == B.OPTIMAL and (kinds is None or ref.counts == kinds)
    # the edge model between two plain ones, so that it is neither first nor last in the grid
    plain = B.binary_bounded(12, 6, 2)[3][0]
    cs = np.stack([plain, c, plain])
    res = gpu.LPSolver().SolvePacked(cs, A, b, upper, lower, sense="min" if sense else "max")
    _equal_ref(res, [P.solve(plain, A, b, lower, upper, sense), ref, P.solve(plain, A, b, lower, upper, sense)], name)
    _equal_single(gpu, res, 1, c, A, b, upper, lower, sense)


def test_a_zero_lower_bound_turns_minus_zero_into_plus_zero(gpu):
    """No seed of binary_bounded(12, 6, .) in 1..199 leaves a -0.0 component in x (searched with the restatement), so this is
    pinned on a hand model: Max x1, x1 <= -0.0.  x1 enters, the ratio is -0.0 / 1, and x1 = -0.0 is basic.  Without a lower array
    it comes back as it is; with lower = (0) the host path adds +0.0 and so does the kernel."""
    c, A, b = np.array([1.0]), np.array([[1.0]]), np.array([-0.0])
    ref = P.solve(c, A, b)
    assert ref.status == B.OPTIMAL and ref.counts == (1, 0, 0) and np.signbit(ref.x[0]) and ref.x[0] == 0.0
    ref0 = P.solve(c, A, b, np.zeros(1))
    assert not np.signbit(ref0.x[0])
    S = gpu.LPSolver()
    res = S.SolvePacked(c, A, b)
    _equal_ref(res, [ref], "no lower")
    _equal_single(gpu, res, 0, c, A, b, None, None, 0)
    res0 = S.SolvePacked(c, A, b, lower=np.zeros(1))
    _equal_ref(res0, [ref0], "zero lower")
    _equal_single(gpu, res0, 0, c, A, b, None, np.zeros(1), 0)
    assert np.signbit(res.Solution[0, 0]) and not np.signbit(res0.Solution[0, 0])


# ---- sharing -------------------------------------------------------------------------------------------------------------
def test_shared_arrays_give_the_bits_of_tiled_ones(gpu):
    (c, A, b, _), _ = _shape("7x19")
    n = 12
    lower = np.zeros(n); lower[3] = 0.25
    upper = np.ones(n); upper[5] = INF
    S = gpu.LPSolver()
    batched = {"c": 2, "A": 3, "b": 2, "upper": 2, "lower": 2}

    def tiled(kw):
        """The same data with every array given its batch axis."""
        out = {}
        for k, v in kw.items():
            v = np.full(n, float(v)) if np.ndim(v) == 0 else np.asarray(v)
            out[k] = v if v.ndim == batched[k] else np.tile(v, (3,) + (1,) * v.ndim)
        return out
    both = tiled(dict(upper=upper, lower=lower))
    for what, kw in (("A", dict(c=c, A=A[0], b=b, **both)),
                     ("c", dict(c=c[1], A=A, b=b, **both)),
                     ("bounds", dict(c=c, A=A, b=b, upper=upper, lower=lower)),
                     ("all but b", dict(c=c[2], A=A[2], b=b, upper=upper, lower=lower)),
                     ("scalar bounds", dict(c=c, A=A, b=b, upper=1.0, lower=0.0))):
        shared = S.SolvePacked(**kw)
        full = tiled(kw)
        _equal_results(shared, S.SolvePacked(**full), what)
        _equal_ref(shared, P.solve_all(full["c"], full["A"], full["b"], full["lower"], full["upper"]), what)
    one = S.SolvePacked(c[0], A[0], b[0], upper, lower)                  # no batch axis anywhere: B = 1
    assert one.Status.shape == (1,) and one.Solution.shape == (1, n)
    _equal_ref(one, [P.solve(c[0], A[0], b[0], lower, upper)], "B = 1")


# ---- one batch of 300 models of 13 x 73 with every status ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mix():
    """300 models of 13 x 73 from 40 seeds, more workgroups than compute units.  By index: unbounded models (column 0 made
    non-positive and unbounded, as in test_unbounded_after_eight_events), models whose shifted RHS is negative, an upper bound
    below its lower bound, an infinite lower bound, and both defects in one model (the bounds are checked first).  max_iter = 45
    lies inside the range of the event counts (38 .. 57 for the 40 seeds), so it stops some models and not others."""
    W, m, n = 300, 12, 60
    base = [B.binary_bounded(n, m, s)[3] for s in range(1, 41)]
    c, A, b = _stack([base[i % 40] for i in range(W)])
    A = A.copy()
    lower = np.zeros((W, n)); upper = np.ones((W, n))
    for i in range(W):
        k = i % 10
        if k == 1:
            A[i, :, 0] = -np.abs(A[i, :, 0]); upper[i, 0] = INF
        if k == 3 or i % 20 == 9:
            lower[i, 0] = 1000.0; upper[i, 0] = 2000.0                  # b' = b - 1000 A[:, 0] < 0
        if k == 5 or i % 20 == 9:
            upper[i, 2] = -1.0                                          # below its lower bound
        if k == 7:
            lower[i, 1] = -INF
    max_iter = 45
    return (c, A, b, lower, upper, max_iter), P.solve_all(c, A, b, lower, upper, max_iter=max_iter)


def test_batch_of_300_with_every_status(gpu):
    (c, A, b, lower, upper, max_iter), refs = _mix()
    count = {s: sum(1 for r in refs if r.status == s) for s in (B.OPTIMAL, B.UNBOUNDED, B.ITER_LIMIT, P.EINVAL, P.E_NEG_RHS)}
    assert all(v > 0 for v in count.values()) and sum(count.values()) == 300, count
    assert [refs[i].status for i in (9, 29)] == [P.EINVAL, P.EINVAL]               # both defects: the bounds come first
    S = gpu.LPSolver()
    res = S.SolvePacked(c, A, b, upper, lower, max_iter=max_iter)
    _equal_ref(res, refs, "the batch")
    assert res.Stats["launches"] == 1 and res.Stats["pivots"] == sum(r.counts[0] + r.counts[1] for r in refs)
    bad = res.Status < 0                                                            # error models: zeroed outputs
    assert bad.sum() == count[P.EINVAL] + count[P.E_NEG_RHS]
    assert not res.Solution[bad].any() and not res.OptimalValue[bad].any() and not res.Basis[bad].any() and not res.AtUpper[bad].any()
    assert not res.Events[bad].any() and not res.BoundCounts[bad].any() and not res.Z[bad].any()
    assert not np.signbit(res.Solution[bad]).any() and not np.signbit(res.OptimalValue[bad]).any()
    for i in range(300):                                                            # every model equals its own count = 1 call
        one = S.SolvePacked(c[i], A[i], b[i], upper[i], lower[i], max_iter=max_iter)
        _equal_ref(one, [refs[i]], "model %d alone" % i)
    for i in (0, 1, 3, 5, 7, 9):                                                    # and the model-level call, where that one answers
        if refs[i].status != B.ITER_LIMIT:
            _equal_single(gpu, res, i, c[i], A[i], b[i], upper[i], lower[i], 0)


def test_a_model_at_the_limit_fails_the_model_level_call_but_not_the_packed_one(gpu):
    (c, A, b, lower, upper, max_iter), refs = _mix()
    i = next(k for k, r in enumerate(refs) if r.status == B.ITER_LIMIT)
    p = gpu.LPProblem.from_arrays(0, c[i], A[i], [0] * 12, b[i])
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver(max_iter=max_iter).SolveBounded(p, upper[i], lower[i], form="onchip")
    assert e.value.code == B.ITER_LIMIT
    res = gpu.LPSolver(max_iter=max_iter).SolvePacked(c[i], A[i], b[i], upper[i], lower[i])        # the engine option is the default
    _equal_ref(res, [refs[i]], "the limit from the engine options")


# ---- the iteration limit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", range(12))
def test_iteration_limit_is_tested_first(gpu, max_iter):
    c, A, b = B.binary_bounded(12, 6, 1)[3]                                         # 10 events: flips first, then pivots
    ref = P.solve(c, A, b, None, np.ones(12), max_iter=max_iter)
    assert ref.status == (B.ITER_LIMIT if max_iter <= 10 else B.OPTIMAL) and ref.events == min(max_iter, 10)
    res = gpu.LPSolver().SolvePacked(c, A, b, 1.0, max_iter=max_iter)
    _equal_ref(res, [ref], "max_iter %d" % max_iter)


# ---- optional outputs, guard bytes, stats -------------------------------------------------------------------------------------
def _raw_call(lpx, c, A, b, upper, want_optional):
    """lpx_solve_packed through ctypes on arrays with 64 guard bytes behind each; returns the arrays (as bytes) and the stats."""
    L = lpx._lib
    count, m, n = A.shape
    GUARD = 64
    sizes = {"status": 4 * count, "x": 8 * count * n, "value": 8 * count, "rec": 40 * count, "basis": 4 * count * m, "at_upper": count * n}
    bufs = {k: np.full(v + GUARD, 0xA5, dtype=np.uint8) for k, v in sizes.items()}
    up = np.ascontiguousarray(np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,)))
    pm = L.PackedModels(count, m, n, 0, c.ctypes.data_as(L.dp), A.ctypes.data_as(L.dp), b.ctypes.data_as(L.dp), None, up.ctypes.data_as(L.dp),
                        n, m * n, m, 0, 0)
    ptr = lambda k, t: C.cast(C.c_void_p(bufs[k].ctypes.data), t)
    pr = L.PackedResults(ptr("status", L.ip), ptr("x", L.dp), ptr("value", L.dp),
                         ptr("rec", C.POINTER(L.PrimalRecord)) if want_optional else None,
                         ptr("basis", L.ip) if want_optional else None,
                         ptr("at_upper", C.POINTER(C.c_uint8)) if want_optional else None)
    st = L.Stats()
    assert L.lib().lpx_solve_packed(C.byref(pm), None, C.byref(pr), C.byref(st)) == 0, L.last_error()
    for k, v in sizes.items():
        assert (bufs[k][v:] == 0xA5).all(), "guard bytes behind " + k
    return {k: bufs[k][:v].tobytes() for k, v in sizes.items()}, st


def test_optional_outputs_guard_bytes_and_stats(gpu):
    (c, A, b, upper), refs = _shape("21x61")
    c, A, b = (np.ascontiguousarray(v) for v in (c, A, b))
    full, st = _raw_call(gpu, c, A, b, upper, True)
    lean, st2 = _raw_call(gpu, c, A, b, upper, False)
    for k in ("status", "x", "value"):
        assert full[k] == lean[k], k
    for k in ("rec", "basis", "at_upper"):                                          # NULL: not written at all
        assert lean[k] == b"\xa5" * len(lean[k]), k
    assert np.frombuffer(full["status"], dtype=np.int32).tolist() == [r.status for r in refs]
    assert np.array_equal(np.frombuffer(full["x"], dtype=np.uint64), np.concatenate([_u64(r.x) for r in refs]))
    assert np.frombuffer(full["basis"], dtype=np.int32).tolist() == np.concatenate([r.basis for r in refs]).tolist()
    assert np.frombuffer(full["at_upper"], dtype=np.uint8).tolist() == np.concatenate([r.at_upper for r in refs]).tolist()
    pivots = sum(r.counts[0] + r.counts[1] for r in refs)
    for s in (st, st2):
        assert s.launches == 1 and s.pivots == pivots and s.loop_ms > 0.0
    res = gpu.LPSolver().SolvePacked(c, A, b, upper, want=())                       # the Python face of the lean call
    assert res.Basis is None and res.AtUpper is None and res.Events is None and res.BoundCounts is None
    assert res.Solution.tobytes() == full["x"] and res.OptimalValue.tobytes() == full["value"]


def test_a_larger_call_after_a_smaller_one_grows_the_arena(gpu):
    """The device buffers are kept between calls and grown when needed: small, large, small again, the same bits each time."""
    (c, A, b, upper), refs = _shape("7x19")
    S = gpu.LPSolver()
    first = S.SolvePacked(c, A, b, upper)
    reps = 700                                                                      # 2100 models: well beyond the first arena
    big = S.SolvePacked(np.tile(c, (reps, 1)), np.tile(A, (reps, 1, 1)), np.tile(b, (reps, 1)), upper)
    again = S.SolvePacked(c, A, b, upper)
    _equal_ref(first, refs, "first"); _equal_results(first, again, "again")
    for k in range(3):
        sel = slice(k, None, 3)
        assert (big.Status[sel] == refs[k].status).all() and (_u64(big.Solution[sel]) == _u64(refs[k].x)).all()
        assert (_u64(big.OptimalValue[sel]) == _u64(refs[k].value)).all() and (big.Basis[sel] == refs[k].basis).all()
        assert (big.BoundCounts[sel] == np.array(refs[k].counts)).all() and (big.AtUpper[sel] == refs[k].at_upper).all()


# ---- the command line: a fresh child process per call ---------------------------------------------------------------------------
def _cli(tmp_path, name, lines, *extra):
    f = tmp_path / name
    f.write_text("".join(line + "\n" for line in lines))
    exe = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
    out = subprocess.run([exe, "--bounded", "--rhs-file", str(f), *extra, os.path.join(ROOT, "integration", "Input", "example_bounded.txt")],
                         check=True, capture_output=True, text=True, timeout=120).stdout
    return out.splitlines()


def test_cli_rhs_file_equals_single_runs(gpu, tmp_path):
    rhs = ["10 15", "11 15", "9 14"]
    bounds = ("--upper", "1=4", "--upper", "2=3", "--upper", "3=3")
    together = _cli(tmp_path, "three.txt", rhs, *bounds)
    assert len(together) == 3
    singles = [_cli(tmp_path, "one%d.txt" % k, [line], *bounds) for k, line in enumerate(rhs)]
    assert together == [s[0] for s in singles] and all(len(s) == 1 for s in singles)
    c, A, b = B.hand_example()[3]                                                   # the file's model: Taha's example
    for line, row in zip(together, rhs):
        bi = np.array([float(v) for v in row.split()])
        ref = P.solve(c, A, bi, np.zeros(3), np.array([4.0, 3.0, 3.0]))            # the CLI always passes both bound arrays
        got = line.split()
        assert int(got[0]) == ref.status and float(got[1]) == ref.value and [float(v) for v in got[2:]] == ref.x.tolist()
    assert together[0].split()[:2] == ["0", "20.75"]
