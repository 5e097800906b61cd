"""GPU tests of the packed batch call for integer programs (lpx_solve_packed_bnb, LPSolver.SolvePackedBnb; kernel in
csrc/lpx_packed_bnb.hip).  Every comparison is bit for bit (np.uint64 views of the doubles, the bytes of the log): against the NumPy
restatement of the contract (tests/_packed_bnb_ref.py) and against SolveBnbBounded(node_form="onchip") of each model.  The
instances are those tests/test_packed_bnb_ref.py checks on the CPU against solve2 and scipy.optimize.milp: 31-297 nodes, depth
7-19, K up to 12.  A model of <= rows with shifted right-hand sides >= 0 holds its shifted origin, so a whole search never ends
INFEASIBLE here; infeasible NODES are met in the binary models, and the = row model, passed as its pair, is LPX_E_NEG_RHS on
both paths."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _bounded_long_ref as L
import _packed_bnb_ref as R
import _packed_dual_ref as PD
import _packed_ref as PP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
SENSE = {0: "max", 1: "min"}
DEEP = 64
FLAGS = {0: {}, L.LONG_STEP: {"long_step": True}, L.CUTOFF_FLAG: {"cutoff": True},
         L.LONG_STEP | L.CUTOFF_FLAG: {"long_step": True, "cutoff": True}}
MODELS = ["binary %d %d %d" % a for a in R.BINARY] + ["general", "lowers", "min", "mixed", "infeasible"]


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _model(name):
    """(c, A, b, upper, lower, is_int, sense, max_depth)"""
    if name.startswith("binary"):
        n, m, seed = (int(v) for v in name.split()[1:])
        return R.binary(n, m, seed) + (None, None, 0, 0)
    return R.small(name) + (DEEP,)


@functools.lru_cache(maxsize=None)
def _ref(name, flags, **kw):
    c, A, b, upper, lower, is_int, sense, depth = _model(name)
    kw.setdefault("max_depth", depth)
    return R.solve(c, A, b, upper, lower, is_int, sense, search_flags=flags, **kw)


def _equal_ref(res, i, ref, what=""):
    """Entry i of a PackedBnbResult against the restatement, every output bit for bit."""
    info = res.Info[i]
    assert (res.Status[i], res.Stop[i]) == (ref["status"], ref["stop"]) and info["status"] == ref["status"], (what, i, info, ref["stop"])
    assert np.array_equal(_u64(res.Solution[i]), _u64(ref["x"])) and _u64(res.OptimalValue[i]) == _u64(ref["value"]), (what, i)
    for k in R.COUNTERS + ("deepest", "root_events"):
        assert info[k] == ref[k], (what, i, k, info[k], ref[k])
    assert res.Nodes[i] == ref["nodes"] and res.Events[i] == ref["events"]
    assert _u64(info["best"]) == _u64(ref["best"]) and _u64(info["constant"]) == _u64(ref["constant"]), (what, i)
    if res.Log is not None:
        cap = res.Log.shape[1]
        k = min(len(ref["log"]), cap)
        assert res.Logged[i] == info["logged"] == k
        assert res.Log[i, :k].tobytes() == ref["log"][:k].tobytes(), (what, i, "log")
        assert not np.frombuffer(res.Log[i, k:].tobytes(), dtype=np.uint8).any(), (what, i, "the log behind its records")


def _equal_single(lpx, res, i, c, A, b, upper, lower, is_int, sense, flags, max_nodes=0, max_iter=None):
    """Entry i against SolveBnbBounded(node_form="onchip") of that model: statuses, x, value, counters and log."""
    p = lpx.LPProblem.from_arrays(sense, c, A, [0] * len(b), b)
    S = lpx.LPSolver(**({} if max_iter is None else {"max_iter": max_iter}))
    try:
        one = S.SolveBnbBounded(p, upper, lower=lower, integer=is_int, max_nodes=max_nodes, node_form="onchip", **FLAGS[flags])
    except lpx.SolverException as e:
        if e.code != lpx._lib.ITER_LIMIT:
            assert res.Status[i] == e.code < 0, (res.Status[i], e.code)
            return
        assert res.Status[i] == lpx._lib.ITER_LIMIT
        one = e.result                                  # the incumbent so far: OPTIMAL with it, INFEASIBLE (zeros) without
        assert (one.Status == R.OPTIMAL) == (res.Info[i]["incumbents"] > 0)
    else:
        assert res.Status[i] == one.Status
    if one.Solution is None:                            # no incumbent: the single solve has no solution, the packed call zeros
        assert one.Status == R.INFEASIBLE and not res.Solution[i].any() and res.Info[i]["incumbents"] == 0
    else:
        assert np.array_equal(_u64(res.Solution[i]), _u64(one.Solution))
    assert _u64(res.OptimalValue[i]) == _u64(one.OptimalValue)
    if one.Status == R.UNBOUNDED:
        return
    for k in R.COUNTERS:
        assert res.Info[i][k] == one.BnbInfo[k], k
    if res.Log is not None:
        k = min(len(one.BnbLog), res.Log.shape[1])
        assert res.Log[i, :k].tobytes() == one.BnbLog[:k].tobytes()


# ---- the models ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", L.FLAG_SETS)
@pytest.mark.parametrize("name", MODELS)
def test_models_equal_the_restatement_and_the_single_solves(gpu, name, flags):
    c, A, b, upper, lower, is_int, sense, depth = _model(name)
    ref = _ref(name, flags)
    res = gpu.LPSolver().SolvePackedBnb(c, A, b, upper, lower, is_int, SENSE[sense], max_depth=depth, log_cap=ref["nodes"] + 3,
                                        **FLAGS[flags])
    assert res.Status.shape == (1,) and res.Stats["launches"] == 1
    _equal_ref(res, 0, ref, name)
    _equal_single(gpu, res, 0, c, A, b, upper, lower, is_int, sense, flags)
    if name == "infeasible":
        assert res.Status[0] == R.E_NEG_RHS
    else:
        assert res.Status[0] == R.OPTIMAL and res.Stop[0] == R.DONE and res.Nodes[0] > 1


def test_a_batch_of_300_mixing_every_status(gpu):
    """Twelve kinds of model of one shape, 25 of each, interleaved: one model's outcome never reaches another's."""
    n, m, seed = 12, 4, 3
    c, A, b, upper = R.binary(n, m, seed)
    mask = np.ones(n, dtype=np.uint8); mask[0] = 0      # x1 is continuous: it may have any bounds
    kinds = []
    for k in range(12):
        ck, Ak, bk, uk, lk = c.copy(), A.copy(), b.copy(), upper.copy(), np.zeros(n)
        if k == 1: bk = b + 1.0
        if k == 2: bk = np.floor(b * 0.5)
        if k == 3: Ak[:, 0] = 0.0; uk[0] = INF          # an unbounded root
        if k == 4: uk[3] = -1.0                         # a bad bound
        if k == 5: uk[5] = 1.5                          # a fractional bound on an integer variable
        if k == 6: bk[1] = -2.0                         # a negative right-hand side
        if k == 7: uk[0] = 0.5                          # a fractional bound on the continuous variable: fine
        if k == 8: lk[2] = 1.0; uk[2] = 2.0; bk = b + A[:, 2]      # a shifted integer
        if k == 9: ck[4] = 0.0
        if k == 10: uk[7] = INF                         # an integer variable without an upper bound
        if k == 11: lk[6] = np.nan
        kinds.append((ck, Ak, bk, uk, lk))
    order = [k for _ in range(25) for k in range(12)]
    cs, As, bs, us, ls = (np.stack([kinds[k][f] for k in order]) for f in range(5))
    res = gpu.LPSolver().SolvePackedBnb(cs, As, bs, us, ls, mask, max_nodes=60, log_cap=8)
    refs = [R.solve(*kinds[k][:3], kinds[k][3], kinds[k][4], mask, max_nodes=60, log_cap=8) for k in range(12)]
    for i, k in enumerate(order):
        _equal_ref(res, i, refs[k], "kind %d" % k)
    got = {(r["status"], r["stop"]) for r in refs}
    assert {(R.OPTIMAL, R.DONE), (R.ITER_LIMIT, R.NODES), (R.UNBOUNDED, R.ROOT), (R.EINVAL, R.ROOT), (R.E_NEG_RHS, R.ROOT)} <= got, got
    assert [refs[k]["status"] for k in (3, 4, 5, 6, 10, 11)] == [R.UNBOUNDED, R.EINVAL, R.EINVAL, R.E_NEG_RHS, R.EINVAL, R.EINVAL]
    assert sum(r["pruned_infeasible"] for r in refs) > 0                            # infeasible nodes are met
    for k in (0, 3, 4, 6, 8):                           # the single solves: optimal or node limit, unbounded, refused, shifted
        ck, Ak, bk, uk, lk = kinds[k]
        _equal_single(gpu, res, k, ck, Ak, bk, uk, lk, mask, 0, 0, max_nodes=60)


def test_shared_arrays_equal_their_tiled_twin_and_64_right_hand_sides(gpu):
    c, A, b, upper = R.binary(10, 4, 2)
    g = np.random.default_rng(5)
    bs = b + g.integers(-2, 3, size=(64, 4)).astype(np.float64)
    S = gpu.LPSolver()
    shared = S.SolvePackedBnb(c, A, bs, 1.0, cutoff=True, log_cap=40)              # c, A and the bounds at stride 0
    tiled = S.SolvePackedBnb(np.tile(c, (64, 1)), np.tile(A, (64, 1, 1)), bs, np.ones((64, 10)), np.zeros((64, 10)), cutoff=True, log_cap=40)
    assert shared.Status.tolist() == tiled.Status.tolist() and shared.Info.tobytes() == tiled.Info.tobytes()
    assert shared.Log.tobytes() == tiled.Log.tobytes() and shared.OptimalValue.tobytes() == tiled.OptimalValue.tobytes()
    assert np.array_equal(shared.Solution, tiled.Solution)                          # a lower array of zeros turns -0.0 into +0.0
    refs = R.solve_all(c, A, bs, 1.0, search_flags=L.CUTOFF_FLAG, log_cap=40)
    for i, r in enumerate(refs):
        _equal_ref(shared, i, r, "rhs %d" % i)
    assert len({r["nodes"] for r in refs}) > 8 and shared.Stats["launches"] == 1
    assert shared.Stats["pivots"] > 0
    for i in (0, 63):
        one = S.SolvePackedBnb(c, A, bs[i], 1.0, cutoff=True, log_cap=40)           # independent of count and of i
        assert one.Info.tobytes() == shared.Info[i:i + 1].tobytes() and one.Log.tobytes() == shared.Log[i:i + 1].tobytes()


def test_a_backtrack_over_the_first_and_the_last_column(gpu):
    """A node whose edit changes K >= 5 columns, column 0 and column n - 1 among them: the ascending compaction across the first and
    the last wave of the diff (n = 70: a full wave and a tail)."""
    g = np.random.default_rng(3)
    n, m = 70, 3
    A = g.integers(1, 10, size=(m, n)).astype(np.float64)
    c = g.integers(1, 15, size=n).astype(np.float64)
    c[0] = 14.5; c[n - 1] = 14.25                       # the two are worth branching on early
    b = np.floor(0.13 * A.sum(axis=1)) + 0.5
    ref = R.solve(c, A, b, np.ones(n), max_nodes=400, search_flags=L.CUTOFF_FLAG)
    res = gpu.LPSolver().SolvePackedBnb(c, A, b, 1.0, cutoff=True, max_nodes=400, log_cap=400)
    _equal_ref(res, 0, ref, "70 columns")
    # the restatement's own account of the edits: some node changed at least 5 columns with both ends among them
    wide = _edits_with_both_ends(c, A, b, n)
    print("nodes", ref["nodes"], "max_K", ref["max_K"], "edits with both ends and K >= 5:", wide)
    assert ref["max_K"] >= 5 and wide > 0


def _edits_with_both_ends(c, A, b, n):
    """Replays the restatement and counts the edits of K >= 5 columns that hold column 0 and column n - 1."""
    seen = []
    node2 = L.Handle.node2

    def spy(self, cols, *a, **kw):
        seen.append(np.asarray(cols).copy())
        return node2(self, cols, *a, **kw)
    L.Handle.node2 = spy
    try:
        R.solve(c, A, b, np.ones(n), max_nodes=400, search_flags=L.CUTOFF_FLAG)
    finally:
        L.Handle.node2 = node2
    return sum(1 for cols in seen if len(cols) >= 5 and 0 in cols and n - 1 in cols)


def test_one_row_and_one_column(gpu):
    g = np.random.default_rng(11)
    A = g.integers(2, 9, size=(1, 70)).astype(np.float64)       # m = 1, n = 70: a row shorter than two waves
    c = g.integers(1, 20, size=70).astype(np.float64)
    b = np.array([41.5])
    for flags in (0, L.LONG_STEP | L.CUTOFF_FLAG):
        ref = R.solve(c, A, b, np.ones(70), search_flags=flags, max_nodes=500)
        res = gpu.LPSolver().SolvePackedBnb(c, A, b, 1.0, max_nodes=500, log_cap=500, **FLAGS[flags])
        _equal_ref(res, 0, ref, "1 x 70")
        assert ref["nodes"] > 3
    # n = 1: 2 x <= 5, 0 <= x <= 4: the root is 2.5, the ceil child is infeasible, the floor child is the optimum
    c1, A1, b1 = np.array([3.0]), np.array([[2.0]]), np.array([5.0])
    ref = R.solve(c1, A1, b1, np.array([4.0]), max_depth=4)
    res = gpu.LPSolver().SolvePackedBnb(c1, A1, b1, 4.0, max_depth=4, log_cap=4)
    _equal_ref(res, 0, ref, "n = 1")
    assert (ref["nodes"], ref["pruned_infeasible"], ref["value"]) == (3, 1, 6.0)
    _equal_single(gpu, res, 0, c1, A1, b1, np.array([4.0]), None, None, 0, 0)


def test_the_last_m_that_fits(gpu):
    fits = gpu._lib.lib().lpx_packed_fits
    assert fits(139, 1) == 1 and fits(140, 1) == 0
    A = np.arange(1.0, 140.0).reshape(139, 1)
    b = A[:, 0] * 2.5                                   # every row says x <= 2.5
    ref = R.solve(np.ones(1), A, b, np.array([4.0]), max_depth=4)
    res = gpu.LPSolver().SolvePackedBnb(np.ones(1), A, b, 4.0, max_depth=4, log_cap=4)
    _equal_ref(res, 0, ref, "139 x 1")
    assert ref["status"] == R.OPTIMAL and ref["value"] == 2.0
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver().SolvePackedBnb(np.ones(1), np.ones((140, 1)), np.ones((2, 140)), upper=1.0)
    assert e.value.code == gpu._lib.EINVAL and "141 x 142" in str(e.value) and "does not fit" in str(e.value)


def test_a_lower_bound_raised_on_a_branched_integer(gpu):
    """General integers 0..3 without a lower array: the first ceil child stores a non-zero lower shift, which the pick and the
    incumbent use from then on; "lowers" starts with one."""
    for name in ("general", "lowers"):
        ref = _ref(name, 0)
        assert (ref["log"]["var"] >= 0).any() and ref["deepest"] > 8
    c, A, b, upper, lower, is_int, sense, depth = _model("general")
    assert lower is None
    res = gpu.LPSolver().SolvePackedBnb(c, A, np.stack([b, b + 1.0, b - 2.0]), upper, None, is_int, max_depth=depth, log_cap=300)
    for i, bi in enumerate((b, b + 1.0, b - 2.0)):
        _equal_ref(res, i, R.solve(c, A, bi, upper, max_depth=depth, log_cap=300), "general %d" % i)


def test_max_depth_exact_and_one_below(gpu):
    c, A, b, upper = R.binary(12, 4, 3)
    full = _ref("binary 12 4 3", 0)
    S = gpu.LPSolver()
    for depth in (full["deepest"], full["deepest"] - 1):
        ref = R.solve(c, A, b, upper, max_depth=depth)
        res = S.SolvePackedBnb(c, A, b, 1.0, max_depth=depth, log_cap=80)
        _equal_ref(res, 0, ref, "max_depth %d" % depth)
    assert ref["stop"] == R.DEPTH and ref["status"] == R.ITER_LIMIT and ref["nodes"] < full["nodes"]


def test_budgets(gpu):
    c, A, b, upper = R.binary(12, 4, 3)
    full = _ref("binary 12 4 3", 0)
    S = gpu.LPSolver()
    for kw in (dict(max_nodes=1), dict(max_nodes=full["nodes"] - 1), dict(max_events=full["events"] - 1), dict(max_events=91),
               dict(max_events=1), dict(max_iter=0), dict(max_iter=1), dict(max_iter=7)):
        ref = R.solve(c, A, b, upper, **kw)
        res = S.SolvePackedBnb(c, A, b, 1.0, log_cap=80, **kw)
        _equal_ref(res, 0, ref, str(kw))
        if "max_nodes" in kw:                           # the budget the host driver has too (its root has no iteration limit of its own)
            _equal_single(gpu, res, 0, c, A, b, upper, None, None, 0, 0, max_nodes=kw["max_nodes"])
    c2, A2, b2, upper2 = R.binary(16, 6, 4)             # its root makes 12 events, its busiest node 15
    ref = R.solve(c2, A2, b2, upper2, max_iter=14)
    res = S.SolvePackedBnb(c2, A2, b2, 1.0, max_iter=14, log_cap=60)
    _equal_ref(res, 0, ref, "max_iter 14")
    assert ref["stop"] == R.NODE_ITER and ref["incumbents"] > 0
    _equal_single(gpu, res, 0, c2, A2, b2, upper2, None, None, 0, 0, max_iter=14)


# ---- optional outputs, guard bytes, stats -------------------------------------------------------------------------------------
def test_log_cap_below_the_node_count_and_guard_bytes(gpu):
    """Through ctypes on arrays with 64 guard bytes behind each: nothing is written past an output, with and without rec / log."""
    Lb = gpu._lib
    c, A, b, upper = R.binary(10, 4, 2)
    bs = np.ascontiguousarray(np.stack([b, b + 1.0, b - 1.0]))
    count, m, n, cap = 3, 4, 10, 5
    refs = [R.solve(c, A, bi, upper, log_cap=cap) for bi in bs]
    assert all(r["nodes"] > cap for r in refs)
    GUARD = 64
    for want in (("rec", "log"), ("rec",), ()):
        sizes = {"status": 4 * count, "x": 8 * count * n, "value": 8 * count, "rec": 88 * count, "log": 32 * count * cap}
        bufs = {k: np.full(v + GUARD, 0xA5, dtype=np.uint8) for k, v in sizes.items()}
        dp = Lb.dp
        pm = Lb.PackedBnbModels(count, m, n, 0, c.ctypes.data_as(dp), A.ctypes.data_as(dp), bs.ctypes.data_as(dp), None,
                                upper.ctypes.data_as(dp), 0, 0, m, 0, 0, None)
        pr = Lb.PackedBnbResults(bufs["status"].ctypes.data_as(Lb.ip), bufs["x"].ctypes.data_as(dp), bufs["value"].ctypes.data_as(dp),
                                 bufs["rec"].ctypes.data_as(C.POINTER(Lb.PackedBnbRecord)) if "rec" in want else None,
                                 bufs["log"].ctypes.data_as(C.POINTER(Lb.BnbNodeLog)) if "log" in want else None)
        po = Lb.PackedBnbOpts(0, 10000, 0, cap if "log" in want else 0, 100000, 2000000)
        st = Lb.Stats()
        assert Lb.lib().lpx_solve_packed_bnb(C.byref(pm), C.byref(po), C.byref(pr), C.byref(st)) == 0, Lb.last_error()
        for k, v in sizes.items():
            assert (bufs[k][v:] == 0xA5).all(), "guard bytes behind " + k
            if k in ("rec", "log") and k not in want:
                assert (bufs[k] == 0xA5).all(), k + " was not asked for"
        assert bufs["status"][:12].view(np.int32).tolist() == [r["status"] for r in refs]
        assert bufs["x"][:sizes["x"]].tobytes() == np.stack([r["x"] for r in refs]).tobytes()
        if "log" in want:
            assert bufs["log"][:sizes["log"]].tobytes() == b"".join(r["log"].tobytes() for r in refs)
        if "rec" in want:
            rec = bufs["rec"][:sizes["rec"]].view(gpu.solver.PACKED_BNB_DTYPE)
            assert rec["nodes"].tolist() == [r["nodes"] for r in refs]
            assert rec["logged"].tolist() == [cap if "log" in want else 0] * count
        assert st.launches == 1 and st.pivots > 0


def test_a_larger_call_after_a_smaller_one_shares_the_arena(gpu):
    S = gpu.LPSolver()
    c, A, b, upper = R.binary(8, 3, 1)
    small_ref = _ref("binary 8 3 1", 0)
    small = S.SolvePackedBnb(c, A, b, 1.0, log_cap=50)
    _equal_ref(small, 0, small_ref, "small")
    pc, pA, pb = np.ones(4), np.array([[1.0, 2.0, 1.0, 3.0], [2.0, 1.0, 3.0, 1.0]]), np.array([[4.0, 5.0], [6.0, 3.0]])
    primal = S.SolvePacked(pc, pA, pb, 1.0)
    c2, A2, b2, upper2 = R.binary(12, 4, 3)
    g = np.random.default_rng(9)
    bs = b2 + g.integers(-1, 2, size=(96, 4)).astype(np.float64)
    big = S.SolvePackedBnb(c2, A2, bs, 1.0, long_step=True, log_cap=16)             # the arena grows
    dual = S.SolvePackedDual(pc, -pA, -pb, [">=", ">="], 1.0, None, "min")
    again = S.SolvePackedBnb(c, A, b, 1.0, log_cap=50)                              # the smaller one again, in the larger arena
    assert again.Info.tobytes() == small.Info.tobytes() and again.Log.tobytes() == small.Log.tobytes()
    assert np.array_equal(_u64(again.Solution), _u64(small.Solution))
    for i, r in enumerate(R.solve_all(c2, A2, bs, 1.0, search_flags=L.LONG_STEP, log_cap=16)):
        _equal_ref(big, i, r, "big %d" % i)
    for i, r in enumerate(PP.solve_all(pc, pA, pb, None, 1.0)):                     # the bits of the packed primal call
        assert primal.Status[i] == r.status and np.array_equal(_u64(primal.Solution[i]), _u64(r.x))
        assert _u64(primal.OptimalValue[i]) == _u64(r.value)
    for i in range(2):                                                              # ... and of the packed dual call
        r = PD.solve(pc, -pA, -pb[i], np.array([1, 1], dtype=np.int32), None, np.ones(4), PD.MIN)
        assert dual.Status[i] == r.status and np.array_equal(_u64(dual.Solution[i]), _u64(r.x))


# ---- the command line: a fresh child process per call ---------------------------------------------------------------------------
def test_cli_bnb_bounded_rhs_file_equals_single_solves(gpu, tmp_path):
    c = np.array([5.0, 4.0, 3.0, 7.0]); A = np.array([[2.0, 3.0, 1.0, 4.0], [4.0, 1.0, 2.0, 3.0]])
    model = tmp_path / "ip.txt"
    model.write_text("Max: 5x1 + 4x2 + 3x3 + 7x4\n2x1 + 3x2 + 1x3 + 4x4 <= 5\n4x1 + 1x2 + 2x3 + 3x4 <= 11\n")
    rhs = ["5 11", "6.5 4.5", "3 3", "-1 3", "9 9"]
    f = tmp_path / "rhs.txt"
    f.write_text("".join(line + "\n" for line in rhs))
    exe = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
    for args, flags in ((("--long-step", "--cutoff"), L.LONG_STEP | L.CUTOFF_FLAG), ((), 0)):
        out = subprocess.run([exe, "--binary", "--bnb-bounded", *args, "--rhs-file", str(f), str(model)],
                             check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
        assert len(out) == len(rhs)
        statuses = []
        for line, row in zip(out, rhs):
            bi = np.array([float(v) for v in row.split()])
            ref = R.solve(c, A, bi, np.ones(4), np.zeros(4), search_flags=flags)    # the CLI always passes both bound arrays
            got = line.split()
            assert int(got[0]) == ref["status"] and float(got[1]) == ref["value"] and [float(v) for v in got[2:]] == ref["x"].tolist()
            statuses.append(ref["status"])
            try:
                one = gpu.LPSolver().SolveBnbBounded(gpu.LPProblem.from_arrays(0, c, A, [0, 0], bi), np.ones(4), lower=np.zeros(4),
                                                     node_form="onchip", **FLAGS[flags])
                assert int(got[0]) == one.Status and float(got[1]) == one.OptimalValue and [float(v) for v in got[2:]] == one.Solution.tolist()
            except gpu.SolverException as e:
                assert int(got[0]) == e.code
        assert statuses[0] == R.OPTIMAL and statuses[3] == R.E_NEG_RHS
    bad = subprocess.run([exe, "--binary", "--bnb-bounded", "--divers", "4", "--rhs-file", str(f), str(model)], capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode == 64 and "--bnb-bounded --rhs-file combines only with" in bad.stderr
