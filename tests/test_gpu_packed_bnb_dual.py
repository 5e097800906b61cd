"""GPU checks of the branch and bound from a dual start: the packed call (lpx_solve_packed_bnb_dual / LPSolver.SolvePackedBnbDual)
and the host driver (lpx_solve_bnb_bounded_dual / LPSolver.SolveBnbBoundedDual), bit for bit -- uint64 views of the doubles, the
bytes of the log -- against the NumPy restatement of the contract (tests/_packed_bnb_dual_ref.py) and against each other.  The
instances are those tests/test_packed_bnb_dual_ref.py checks on the CPU against scipy.optimize.milp: covering models, rows of both
senses, an = row as its pair (a search that ends INFEASIBLE), a root without a point, a right-hand-side sweep, the edge shapes."""
import os
import subprocess

import numpy as np
import pytest

import _bounded_long_ref as L
import _packed_bnb_dual_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
SENSE = {0: "max", 1: "min"}
FLAGS = {0: {}, L.LONG_STEP: {"long_step": True}, L.CUTOFF_FLAG: {"cutoff": True},
         L.LONG_STEP | L.CUTOFF_FLAG: {"long_step": True, "cutoff": True}}
LAST = "edge 9x130 s1"


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


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


def _single(lpx, inst, flags, node_form="onchip", max_nodes=0, max_iter=None):
    """SolveBnbBoundedDual of one instance: (result, error code or 0)."""
    c, A, rel, b, upper, lower, is_int, sense = inst
    p = lpx.LPProblem.from_arrays(sense, c, A, [int(r) for r in rel], b)
    S = lpx.LPSolver(**({} if max_iter is None else {"max_iter": max_iter}))
    try:
        return S.SolveBnbBoundedDual(p, upper, lower=lower, integer=is_int, max_nodes=max_nodes, node_form=node_form, **FLAGS[flags]), 0
    except lpx.SolverException as e:
        return getattr(e, "result", None), e.code


def _equal_single(lpx, res, i, inst, flags, max_nodes=0, max_iter=None):
    """Entry i against SolveBnbBoundedDual(node_form="onchip") of that model: statuses, x, value, counters and log."""
    one, code = _single(lpx, inst, flags, "onchip", max_nodes, max_iter)
    if code and code != lpx._lib.ITER_LIMIT:
        assert res.Status[i] == code < 0, (res.Status[i], code)
        return
    if code:
        assert res.Status[i] == lpx._lib.ITER_LIMIT and one is not None
        assert (one.Status == R.OPTIMAL) == (res.Info[i]["incumbents"] > 0)
    else:
        assert res.Status[i] == one.Status
    if one.Status == R.INFEASIBLE:                      # no incumbent: zeros on both sides (a root without a point, or the search)
        assert not res.Solution[i].any() and res.Info[i]["incumbents"] == 0 and res.OptimalValue[i] == 0.0
        assert one.Solution is None or not np.asarray(one.Solution).any()
    else:
        assert np.array_equal(_u64(res.Solution[i]), _u64(one.Solution))
    assert _u64(res.OptimalValue[i]) == _u64(one.OptimalValue)
    for k in R.COUNTERS:
        assert res.Info[i][k] == one.BnbInfo[k], k
    if res.Log is not None:
        k = min(len(one.BnbLog), res.Log.shape[1])
        assert res.Log[i, :k].tobytes() == one.BnbLog[:k].tobytes()


def _packed(lpx, inst, flags, **kw):
    c, A, rel, b, upper, lower, is_int, sense = inst
    return lpx.LPSolver().SolvePackedBnbDual(c, A, b, rel, upper, lower, is_int, SENSE[sense], **FLAGS[flags], **kw)


# ---- 1. the models -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", L.FLAG_SETS)
@pytest.mark.parametrize("name", list(R.INSTANCES))
def test_models_equal_the_restatement_and_the_host_driver(gpu, name, flags):
    inst, kw = R.INSTANCES[name]
    ref = R.ref(name, flags)
    res = _packed(gpu, inst, flags, log_cap=ref["nodes"] + 3, **kw)
    assert res.Status.shape == (1,) and res.Stats["launches"] == 1
    _equal_ref(res, 0, ref, name)
    _equal_single(gpu, res, 0, inst, flags)
    assert res.Stop[0] == (R.ROOT if ref["nodes"] == 0 else R.DONE)
    if name == "eq_pair":
        assert (res.Status[0], res.Stop[0]) == (R.INFEASIBLE, R.DONE) and res.Nodes[0] > 1 and res.Info[0]["pruned_infeasible"] > 0
    if name in ("root_infeasible", "sweep f=1.05"):
        assert (res.Status[0], res.Stop[0], res.Nodes[0]) == (R.INFEASIBLE, R.ROOT, 0) and res.Info[0]["root_events"] > 0
    if name.startswith("mixed_rows"):
        assert res.Info[0]["pruned_infeasible"] > 0 and res.Nodes[0] > 1


# ---- 2. the host driver ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", (0, L.LONG_STEP | L.CUTOFF_FLAG))
@pytest.mark.parametrize("name", ["cover 6x12 s1", "mixed_rows s2", "mixed_general s3", "eq_pair", "root_infeasible"])
def test_host_driver_forms_agree_and_equal_the_restatement(gpu, name, flags):
    inst, _ = R.INSTANCES[name]
    ref = R.ref(name, flags)
    a, ca = _single(gpu, inst, flags, "launches")
    b, cb = _single(gpu, inst, flags, "onchip")
    assert ca == cb == 0
    for one in (a, b):
        assert one.Status == ref["status"] and _u64(one.OptimalValue) == _u64(ref["value"])
        assert one.BnbLog.tobytes() == ref["log"].tobytes() and one.Nodes == ref["nodes"]
        for k in R.COUNTERS:
            assert one.BnbInfo[k] == ref[k], k
        assert _u64(one.BnbInfo["constant"]) == _u64(ref["constant"])
        if ref["status"] == R.OPTIMAL:
            assert np.array_equal(_u64(one.Solution), _u64(ref["x"]))
    assert a.BnbLog.tobytes() == b.BnbLog.tobytes()
    if name == "root_infeasible":                       # the result of a search without an incumbent, and without a node
        assert (a.Status, a.Nodes, a.OptimalValue, a.Summary) == (R.INFEASIBLE, 0, 0.0, "INFEASIBLE\n") and len(a.BnbLog) == 0
        assert a.Solution is None or not np.asarray(a.Solution).any()


def test_the_primal_start_still_refuses_a_covering_model(gpu):
    c, A, rel, b, upper, lower, is_int, sense = R.cover(6, 12, 1)
    p = gpu.LPProblem.from_arrays(sense, c, A, [int(r) for r in rel], b)
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver().SolveBnbBounded(p, upper, node_form="onchip")
    assert e.value.code == gpu._lib.E_GE_PRESENT


# ---- 3. a batch of one shape mixing every outcome ------------------------------------------------------------------------------
def test_a_batch_of_300_mixing_every_outcome(gpu):
    """Ten kinds of model of one shape, 30 of each, interleaved: one model's outcome never reaches another's."""
    c, A, rel, b, upper, _, _, sense = R.mixed_rows(2)
    n, m = 10, 6
    mask = np.ones(n, dtype=np.uint8); mask[0] = 0      # x1 is continuous: it may have any bounds
    s = A.sum(axis=1)
    kinds = []
    for k in range(10):
        ck, Ak, bk, rk, uk, lk = c.copy(), A.copy(), b.copy(), rel.copy(), upper.copy(), np.zeros(n)
        if k == 1: bk = b + np.where(rel == R.GE, -1.0, 1.0)
        if k == 2:                                      # 2 x2 + 2 x3 + 2 x4 = 3 as rows 0 and 1: an LP point, no integer point
            Ak[:2] = 0.0; Ak[:2, 1:4] = 2.0; bk[:2] = 3.0
        if k == 3: bk = np.where(rel == R.GE, s + 1.0, b)                              # a root without a point
        if k == 4: uk[3] = -1.0                         # a bad bound
        if k == 5: uk[5] = 1.5                          # a fractional bound on an integer variable
        if k == 6: rk[2] = R.EQ                         # a row sense of its own that is neither <= nor >=
        if k == 7: ck[0] = 5.0; uk[0] = INF             # the continuous variable improves the objective and has no upper bound
        if k == 8: uk[0] = 0.5                          # a fractional bound on the continuous variable: fine
        if k == 9: lk[2] = 1.0; uk[2] = 2.0; bk = b + A[:, 2]      # a shifted integer
        kinds.append((ck, Ak, bk, rk, uk, lk))
    refs = [R.solve(ck, Ak, bk, rk, uk, lk, mask, sense, log_cap=8) for ck, Ak, bk, rk, uk, lk in kinds]
    outcomes = [(r["status"], r["stop"], r["why"]) for r in refs]
    print(outcomes, [r["nodes"] for r in refs])
    assert outcomes[0][:2] == (R.OPTIMAL, R.DONE) and outcomes[2][:2] == (R.INFEASIBLE, R.DONE) and outcomes[3][:2] == (R.INFEASIBLE, R.ROOT)
    assert [o[2] for o in outcomes[4:8]] == ["bound", "integer", "rel", "precheck"] and all(o[0] == R.EINVAL for o in outcomes[4:8])
    assert refs[2]["nodes"] > 1
    order = [k for _ in range(30) for k in range(10)]
    cs, As, bs, rs, us, ls = (np.stack([kinds[k][f] for k in order]) for f in range(6))
    res = gpu.LPSolver().SolvePackedBnbDual(cs, As, bs, rs, us, ls, mask, SENSE[sense], log_cap=8)
    assert res.Stats["launches"] == 1 and res.Status.shape == (300,)
    for i, k in enumerate(order):
        _equal_ref(res, i, refs[k], "kind %d" % k)
    for k, (ck, Ak, bk, rk, uk, lk) in enumerate(kinds):    # each entry equals its own one-model call
        one = gpu.LPSolver().SolvePackedBnbDual(ck, Ak, bk, rk[None], uk, lk, mask, SENSE[sense], log_cap=8)      # rel its own, not shared
        j = 290 + k
        assert one.Info.tobytes() == res.Info[j:j + 1].tobytes() and one.Log.tobytes() == res.Log[j:j + 1].tobytes()
        assert np.array_equal(_u64(one.Solution), _u64(res.Solution[j:j + 1])) and _u64(one.OptimalValue[0]) == _u64(res.OptimalValue[j])
    for k in (0, 2, 3, 7, 9):                           # the host driver: optimal, both infeasible forms, the precheck, shifted
        ck, Ak, bk, rk, uk, lk = kinds[k]
        _equal_single(gpu, res, k, (ck, Ak, rk, bk, uk, lk, mask, sense), 0)


# ---- 4. sharing and position ---------------------------------------------------------------------------------------------------
def test_shared_arrays_equal_their_packed_twin_and_position_does_not_matter(gpu):
    insts = R.sweep()
    c, A, rel, _, upper, _, _, sense = insts[0]
    bs = np.stack([i[3] for i in insts])
    B = len(insts)
    S = gpu.LPSolver()
    shared = S.SolvePackedBnbDual(c, A, bs, rel, 1.0, None, None, "min", cutoff=True, log_cap=40)      # c, A, rel, the bounds at stride 0
    packed = S.SolvePackedBnbDual(np.tile(c, (B, 1)), np.tile(A, (B, 1, 1)), bs, np.tile(rel, (B, 1)), np.ones((B, 9)), None, None, "min",
                                  cutoff=True, log_cap=40)
    assert shared.Status.tolist() == packed.Status.tolist() and shared.Info.tobytes() == packed.Info.tobytes()
    assert shared.Log.tobytes() == packed.Log.tobytes() and shared.OptimalValue.tobytes() == packed.OptimalValue.tobytes()
    assert np.array_equal(_u64(shared.Solution), _u64(packed.Solution))
    for i, f in enumerate(R.SWEEP_F):
        _equal_ref(shared, i, R.ref("sweep f=%g" % f, L.CUTOFF_FLAG), "sweep %g" % f)
    assert shared.Status.tolist() == [R.OPTIMAL] * 5 + [R.INFEASIBLE] and shared.Stats["launches"] == 1 and shared.Stats["pivots"] > 0
    # one model at index 0 of a batch of 1 and at index 70 of a batch of 130
    inst, _ = R.INSTANCES["mixed_rows s3"]
    cm, Am, relm, bm, um, _, _, sm = inst
    one = S.SolvePackedBnbDual(cm, Am, bm, relm, um, sense=SENSE[sm], log_cap=60)
    many_b = np.tile(bm, (130, 1)) + np.where(np.arange(130)[:, None] == 70, 0.0, 1.0) * np.where(relm == R.GE, -1.0, 1.0)
    many = S.SolvePackedBnbDual(cm, Am, many_b, relm, um, sense=SENSE[sm], log_cap=60)
    assert one.Info.tobytes() == many.Info[70:71].tobytes() and one.Log.tobytes() == many.Log[70:71].tobytes()
    assert np.array_equal(_u64(one.Solution), _u64(many.Solution[70:71])) and _u64(one.OptimalValue[0]) == _u64(many.OptimalValue[70])
    _equal_ref(many, 70, R.ref("mixed_rows s3", 0), "index 70")


# ---- 5. the budgets --------------------------------------------------------------------------------------------------------------
def test_budgets(gpu):
    inst, _ = R.INSTANCES["mixed_rows s2"]
    c, A, rel, b, upper, lower, is_int, sense = inst
    full = R.ref("mixed_rows s2", 0)
    busiest = int(full["log"]["events"].max())
    stops = set()
    for kw in (dict(max_nodes=1), dict(max_nodes=full["nodes"] - 1), dict(max_events=full["events"] // 2), dict(max_events=1),
               dict(max_depth=full["deepest"]), dict(max_depth=full["deepest"] - 1), dict(max_iter=busiest - 1), dict(max_iter=1),
               dict(max_iter=0)):
        ref = R.solve(c, A, b, rel, upper, lower, is_int, sense, **kw)
        res = _packed(gpu, inst, 0, log_cap=full["nodes"] + 3, **kw)
        _equal_ref(res, 0, ref, str(kw))
        stops.add(ref["stop"])
        if "max_nodes" in kw:                           # the budget the host driver has too
            _equal_single(gpu, res, 0, inst, 0, max_nodes=kw["max_nodes"])
        if kw == dict(max_nodes=full["nodes"] - 1):
            assert ref["incumbents"] > 0 and res.Solution[0].any()      # the incumbent so far
    assert stops == {R.DONE, R.ROOT, R.NODES, R.NODE_ITER, R.EVENTS, R.DEPTH}
    for cap in (10, full["nodes"] + 40):                # log_cap below and above the node count
        res = _packed(gpu, inst, 0, log_cap=cap)
        _equal_ref(res, 0, full, "log_cap %d" % cap)
        assert res.Logged[0] == min(cap, full["nodes"])


# ---- 6. the edge shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", (0, L.LONG_STEP | L.CUTOFF_FLAG))
@pytest.mark.parametrize("name", list(R.EDGES))
def test_edge_shapes(gpu, name, flags):
    inst, kw = R.EDGES[name]
    ref = R.ref(name, flags)
    res = _packed(gpu, inst, flags, log_cap=ref["nodes"] + 3, **kw)
    _equal_ref(res, 0, ref, name)
    if name == LAST:
        assert (res.Status[0], res.Stop[0], res.Nodes[0]) == (R.ITER_LIMIT, R.NODES, 200)
        _equal_single(gpu, res, 0, inst, flags, max_nodes=200)
    else:
        assert (res.Status[0], res.Stop[0]) == (R.OPTIMAL, R.DONE) and res.Nodes[0] > 1
        _equal_single(gpu, res, 0, inst, flags)         # the host driver has no depth budget; none binds here


def test_the_largest_n_that_fits_eight_rows(gpu):
    fits = gpu._lib.lib().lpx_packed_fits
    n = 1
    while fits(8, 2 * n):
        n *= 2
    step = n
    while step:                                         # the largest n with fits(8, n)
        if fits(8, n + step):
            n += step
        step //= 2
    assert fits(8, n) == 1 and fits(8, n + 1) == 0 and n > 1024
    inst = R.cover(8, n, 1)
    c, A, rel, b, upper, lower, is_int, sense = inst
    ref = R.solve(c, A, b, rel, upper, sense=sense, max_nodes=50)
    res = _packed(gpu, inst, 0, max_nodes=50, log_cap=50)
    _equal_ref(res, 0, ref, "8 x %d" % n)
    assert ref["nodes"] > 1
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver().SolvePackedBnbDual(np.ones(n + 1), np.ones((8, n + 1)), np.ones(8), None, 1.0)
    assert e.value.code == gpu._lib.EINVAL and "does not fit" in str(e.value) and str(e.value).startswith("lpx_solve_packed_bnb_dual: ")


# ---- 7. the command line: a fresh child process per call ----------------------------------------------------------------------
def test_cli_dual_root(gpu, tmp_path):
    c = np.array([5.0, 4.0, 3.0, 7.0]); A = np.array([[2.0, 3.0, 1.0, 4.0], [4.0, 1.0, 2.0, 3.0]])
    rel = np.array([R.GE, R.GE], dtype=np.int32)
    model = tmp_path / "cover.txt"
    model.write_text("Min: 5x1 + 4x2 + 3x3 + 7x4\n2x1 + 3x2 + 1x3 + 4x4 >= 5\n4x1 + 1x2 + 2x3 + 3x4 >= 6\n")
    rhs = ["5 6", "6.5 4.5", "3 3", "-1 3", "11 9"]
    f = tmp_path / "rhs.txt"
    f.write_text("".join(line + "\n" for line in rhs))
    exe = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
    for args, flags in ((("--long-step", "--cutoff"), L.LONG_STEP | L.CUTOFF_FLAG), ((), 0)):
        out = subprocess.run([exe, "--binary", "--bnb-bounded", "--dual-root", *args, "--rhs-file", str(f), str(model)],
                             check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
        assert len(out) == len(rhs)
        bs = np.array([[float(v) for v in row.split()] for row in rhs])
        # the CLI always passes both bound arrays
        res = gpu.LPSolver().SolvePackedBnbDual(c, A, bs, rel, np.ones(4), np.zeros(4), None, "min", **FLAGS[flags])
        for i, line in enumerate(out):
            got = line.split()
            assert int(got[0]) == res.Status[i] and float(got[1]) == res.OptimalValue[i]
            assert [float(v) for v in got[2:]] == res.Solution[i].tolist()
            ref = R.solve(c, A, bs[i], rel, np.ones(4), np.zeros(4), None, R.MIN, search_flags=flags)
            assert int(got[0]) == ref["status"] and float(got[1]) == ref["value"]
            assert res.Status.tolist() == [R.OPTIMAL, R.OPTIMAL, R.OPTIMAL, R.OPTIMAL, R.INFEASIBLE]
    alone = subprocess.run([exe, "--binary", "--bnb-bounded", "--dual-root", str(model)], capture_output=True, text=True, timeout=120)
    ref = R.solve(c, A, np.array([5.0, 6.0]), rel, np.ones(4), np.zeros(4), None, R.MIN)
    assert alone.returncode == 0 and ("%g" % ref["value"]) in alone.stdout and "nodes: %d" % ref["nodes"] in alone.stdout
    primal = subprocess.run([exe, "--binary", "--bnb-bounded", str(model)], capture_output=True, text=True, timeout=120)
    assert primal.returncode == 70 and ">=" in primal.stderr                       # without the flag nothing changes
    bad = subprocess.run([exe, "--binary", "--bnb-bounded", "--dual-root", "--divers", "4", str(model)], capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode == 64 and "--dual-root needs --bnb-bounded and combines only with" in bad.stderr
    eq = tmp_path / "eq.txt"
    eq.write_text("Max: 1x1 + 1x2\n2x1 + 2x2 = 3\n")
    f1 = tmp_path / "one.txt"
    f1.write_text("3\n")
    r = subprocess.run([exe, "--binary", "--bnb-bounded", "--dual-root", "--rhs-file", str(f1), str(eq)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 65 and "an = constraint is not accepted" in r.stderr
