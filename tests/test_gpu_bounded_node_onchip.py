"""GPU tests of the on-chip form of a branch-and-bound node (csrc/lpx_bounded_node.hip: lpx_bounded_node3 with LPX_NODE_ONCHIP,
lpx_solve_bnb_bounded3): one kernel launch per node with the tableau in LDS, bit for bit against the NumPy restatement of
lpx_bounded_node2 (tests/_bounded_long_ref.py) and against a second device handle on the launches form -- record, trace,
tableau, basis, flip, ub, lo and counts; at the lane, wave and row edges of the kernel, with every flag, on the children of
solved roots, along dives, on refusals, at the iteration limit, with the two forms alternating on one handle, and through
the driver and the command line."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bounded_dual_ref as D
import _bounded_long_ref as L
import _bounded_ref as B
from _node_helpers import (bits as _bits, covering_with_fixed as _covering_with_fixed, fresh as _fresh_handle, node3 as _node3,
                           same_record as _same_record, same_state as _same_state, slack_handle as _slack_handle, state as _state,
                           u64 as _u64)

pytestmark = pytest.mark.gpu

INF = np.inf
REL = 1e-9
SKIP, LONG, CUT = L.SKIP_FIXED, L.LONG_STEP, L.CUTOFF_FLAG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
EXAMPLE = os.path.join(ROOT, "integration", "Input", "example_bounded.txt")


def _fresh(lpx, T, basis, ub):
    dt = _fresh_handle(lpx, T, basis, ub)
    dt.snapshot()
    return dt


def _solved_handle(lpx, n, m, seed):
    T, basis, ub, model, Ts, bs, flip = D.root(n, m, seed)
    dt = lpx.DeviceTableau.from_host(T, basis)
    dt.set_bounds(ub)
    status, _ = dt.bounded_run()
    assert status == B.OPTIMAL and np.array_equal(_u64(dt.download()[0]), _u64(Ts))
    dt.snapshot()
    return dt, (Ts, bs, ub, flip)


# ---- 1. lane, wave and row edges with K = 0 on slack-basis covering tableaux ------------------------------------------------
# (m, n): R x C, status, events plain, of them kind 1 (None: not asserted), events long-step, of them passes (None: > 0 only)
EDGES = {
    (1, 3): ((2, 5), L.OPTIMAL, 1, None, 1, None),
    (2, 1): ((3, 4), L.OPTIMAL, 1, None, 1, None),
    (15, 48): ((16, 64), L.OPTIMAL, 32, None, 46, None),
    (16, 47): ((17, 64), L.OPTIMAL, 28, None, 41, None),
    (31, 32): ((32, 64), L.OPTIMAL, 29, None, 49, None),
    (32, 32): ((33, 65), L.OPTIMAL, 29, None, 50, None),
    (63, 190): ((64, 254), L.OPTIMAL, 213, 133, 408, 350),
    (64, 190): ((65, 255), L.OPTIMAL, 197, None, 345, None),
    (65, 190): ((66, 256), L.OPTIMAL, 200, None, 305, None),
    (8, 1015): ((9, 1024), L.OPTIMAL, 462, None, 955, None),
    (8, 1016): ((9, 1025), L.OPTIMAL, 424, None, 775, 765),
    (8, 1017): ((9, 1026), L.OPTIMAL, 458, None, 727, None),
    (129, 4): ((130, 134), L.INFEASIBLE, 7, None, 7, None),      # at the edge of the guaranteed fit; passes made stay applied
}


@pytest.mark.parametrize("flags", [0, LONG])
@pytest.mark.parametrize("m,n", sorted(EDGES))
def test_node_at_lane_wave_and_row_edges(gpu, m, n, flags):
    shape, status, ev_plain, kind1, ev_long, passes = EDGES[(m, n)]
    T, basis, ub = _covering_with_fixed(m, n, 1)
    assert T.shape == shape and gpu._lib.lib().lpx_bounded_node_fits(*shape) == 1
    with _fresh(gpu, T, basis, ub) as dt, _fresh(gpu, T, basis, ub) as other:
        assert dt.bounded_node_fits()
        got, want = _node3(dt, _slack_handle(T, basis, ub), [], [], [], n, flags, other=other)
    assert want["status"] == status and want["events"] == (ev_long if flags else ev_plain)
    if not flags and kind1 is not None:
        assert want["kind1"] == kind1
    if flags and passes is not None:
        assert want["events"] - want["kind0"] - want["kind1"] == passes
    if flags and ev_long != ev_plain:
        assert want["events"] - want["kind0"] - want["kind1"] > 0


# ---- 2. cutoff ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, LONG])
@pytest.mark.parametrize("m,n", [(31, 32), (63, 190)])
def test_node_cutoff(gpu, m, n, flags):
    T, basis, ub = _covering_with_fixed(m, n, 1)
    full = L.dual_run3(T, basis, ub, None, SKIP | flags)
    half = L.dual_run3(T, basis, ub, None, SKIP | flags, max_iter=len(full[4]) // 2)
    cutoff = float(half[1][-1, -1])                    # the objective after about half of the events
    assert full[0] == L.OPTIMAL and cutoff > full[1][-1, -1]
    with _fresh(gpu, T, basis, ub) as dt, _fresh(gpu, T, basis, ub) as other:
        got, want = _node3(dt, _slack_handle(T, basis, ub), [], [], [], n, flags, cutoff=cutoff, other=other)
        assert want["status"] == L.CUTOFF and 0 < want["events"] < len(full[4]) and want["z"] <= cutoff
        assert got["var"] == -1 and got["candidates"] == 0 and got["x_var"] == 0.0
        # a second call on the same handle obeys its own cutoff; -inf never fires
        dt.restore(); other.restore()
        got, want = _node3(dt, _slack_handle(T, basis, ub), [], [], [], n, flags, cutoff=-INF, other=other)
        assert want["status"] == L.OPTIMAL and want["events"] == len(full[4])
        dt.restore()
        later = float(L.dual_run3(T, basis, ub, None, SKIP | flags, max_iter=3 * len(full[4]) // 4)[1][-1, -1])
        got2, want2 = _node3(dt, _slack_handle(T, basis, ub), [], [], [], n, flags, cutoff=later)
        assert want2["status"] == L.CUTOFF and want2["z"] <= later


# ---- 3. children of solved roots ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,seed", [(12, 6, 1), (40, 20, 1), (64, 32, 2), (128, 64, 1)])
def test_node_on_the_children_of_a_root_and_with_no_change(gpu, n, m, seed):
    dt, root = _solved_handle(gpu, n, m, seed)
    other, _ = _solved_handle(gpu, n, m, seed)
    z_root = root[0][-1, -1]
    statuses = set()
    with dt, other:
        assert dt.bounded_node_fits() and ((n, m) != (128, 64) or (dt.R, dt.C) == (65, 193))
        got, want = _node3(dt, L.Handle(*root), [], [], [], n, other=other)          # K = 0: the root itself
        assert want["status"] == L.OPTIMAL and want["events"] == 0 and want["var"] >= 0
        for j, l, u in D.children(n, m, seed):
            plain = N.Handle(*root).node([j], [l], [u], n)
            mid = 0.5 * (z_root + plain["z"])
            for flags, cutoff in ((0, None), (LONG, None), (0, mid), (LONG, mid)):
                dt.restore(); other.restore()
                got, want = _node3(dt, L.Handle(*root), j, l, u, n, flags, cutoff, other=other)
                statuses.add(want["status"])
    assert L.OPTIMAL in statuses


# ---- 4. a dive and its relaxation -----------------------------------------------------------------------------------------
def test_node_relaxing_after_fixing_forces_flips(gpu):
    n = 40
    dt, root = _solved_handle(gpu, n, 20, 1)
    other, _ = _solved_handle(gpu, n, 20, 1)
    with dt, other:
        h = L.Handle(*root)
        fixed = []
        for step in range(6):                                                     # a dive: fix the pick at 0, 1, 0, ...
            p = N.pick(h.T, h.basis, h.flip, h.ub, h.lo, n)
            if p["var"] < 0:
                break
            v = float(step % 2)
            got, want = _node3(dt, h, p["var"], v, v, n, other=other)
            fixed.append(p["var"])
            if want["status"] != L.OPTIMAL:
                break
        assert len(fixed) >= 3
        got, want = _node3(dt, h, sorted(fixed), 0.0, 1.0, n, other=other)       # K > 1, ascending: back to the root bounds
        assert want["status"] == L.OPTIMAL and want["flips"] > 0, "relaxing the fixed columns needed no flip: the test shows nothing"
        assert abs(want["z"] - root[0][-1, -1]) <= REL * abs(root[0][-1, -1])     # the root's optimum again
        assert got["flips"] == want["flips"]


# ---- 5. the cycling node --------------------------------------------------------------------------------------------------
def test_cycling_node_ends_optimal_in_21_events(gpu):
    dt, root = _solved_handle(gpu, 64, 32, 1)
    other, _ = _solved_handle(gpu, 64, 32, 1)
    with dt, other:
        cols = np.array(sorted(N.CYCLING_ONES + N.CYCLING_ZEROS), dtype=np.int32)
        vals = np.array([1.0 if j in N.CYCLING_ONES else 0.0 for j in cols])
        got, want = _node3(dt, L.Handle(*root), cols, vals, vals, 64, other=other)
        assert want["status"] == L.OPTIMAL and want["events"] == 21


# ---- 6. refusals leave the handle alone -----------------------------------------------------------------------------------
def test_node_refuses_an_unrepairable_column_and_leaves_the_handle_alone(gpu):
    T, basis, ub, _ = B.binary_bounded(12, 6, 1)
    ub = ub.copy(); ub[2] = INF                          # T[m,2] = -c_2 < 0 with no upper bound
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        before = _state(dt)
        for cols, low, up in (([], [], []), ([0, 5], [0.0, 1.0], [0.0, 1.0])):
            h = _slack_handle(T, basis, ub)
            want = h.node2(np.array(cols, dtype=np.int32), np.array(low), np.array(up), 12)
            assert want["status"] is None and want["unrepairable"] == 1
            with pytest.raises(gpu.LpxError) as e:
                dt.bounded_node(cols, low, up, 12, form="onchip")
            assert e.value.code == gpu._lib.EINVAL and "lpx_bounded_node3: 1 column(s)" in str(e.value) and "no upper bound" in str(e.value)
            assert _state(dt) == before, "the refused node changed the handle"
        h = _slack_handle(T, basis, ub)                  # a valid node follows: column 2 gets a bound, and is flipped
        got, want = _node3(dt, h, [2], [0.0], [1.0], 12)
        assert want["status"] is not None and want["flips"] > 0


def test_node_refuses_inf_on_a_flipped_column_and_leaves_the_handle_alone(gpu):
    n = 40
    dt, root = _solved_handle(gpu, n, 20, 1)
    flipped = np.flatnonzero(root[3][:n])
    assert len(flipped) > 0
    j = int(flipped[0])
    with dt:
        before = _state(dt)
        for cols, low, up, k in (([j], [0.0], [INF], 0), ([0 if j else 1, j], [0.0, 0.0], [1.0, INF], 1)):
            with pytest.raises(gpu.LpxError) as e:
                dt.bounded_node(cols, low, up, n, form="onchip")
            assert e.value.code == gpu._lib.EINVAL and "lpx_bounded_node3: upper[%d] = +inf on a flipped column" % k in str(e.value)
            assert _state(dt) == before
        _node3(dt, L.Handle(*root), j, 0.0, 0.0, n)


# ---- 7. masks and lower shifts --------------------------------------------------------------------------------------------
def test_node_mask_and_lower_shift(gpu):
    n = 40
    dt, root = _solved_handle(gpu, n, 20, 1)
    other, _ = _solved_handle(gpu, n, 20, 1)
    with dt, other:
        h = L.Handle(*root)
        got, want = _node3(dt, h, [], [], [], n, other=other)
        assert want["var"] >= 0
        mask = np.ones(n, dtype=np.uint8); mask[want["var"]] = 0                  # the mask removes the closest candidate
        again, want2 = _node3(dt, h, [], [], [], n, is_int=mask, other=other)
        assert want2["var"] != want["var"] and want2["candidates"] == want["candidates"] - 1
        again, want3 = _node3(dt, h, [], [], [], n, is_int=mask, other=other)     # the same bytes again: nothing is sent
        assert want3["var"] == want2["var"]
        mask2 = mask.copy(); mask2[want2["var"]] = 0                               # other bytes: sent again
        again, want4 = _node3(dt, h, [], [], [], n, is_int=mask2, other=other)
        assert want4["var"] not in (want["var"], want2["var"])
        # non-zero lower bounds: lo is used by the pick and by bounded_solution
        j = want["var"]
        got, want5 = _node3(dt, h, [j], [1.0], [1.0], n, other=other)
        assert h.lo[j] == 1.0 and want5["status"] == L.OPTIMAL
        x = dt.bounded_solution(n)[0]
        assert np.array_equal(_u64(x), _u64(N.values(h.T, h.basis, h.flip, h.ub, h.lo, n))) and x[j] == 1.0
        got, want6 = _node3(dt, h, [], [], [], n, other=other)                     # the pick of a handle that has stored a lower shift
        assert _bits(got["x_var"]) == _bits(want6["x_var"])


# ---- 8. iteration limit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, LONG])
def test_node_iteration_limit(gpu, flags):
    T, basis, ub = _covering_with_fixed(31, 32, 1)
    with _fresh(gpu, T, basis, ub) as dt, _fresh(gpu, T, basis, ub) as other:
        got, want = _node3(dt, _slack_handle(T, basis, ub), [], [], [], 32, flags, other=other, max_iter=3)
        assert want["status"] == L.ITER_LIMIT and want["events"] >= 3 and got["var"] == -1
        if not flags:
            assert want["events"] == 3
    if flags:       # the limit is tested in step 1 only: a limit inside a run of passes lets the launch finish them
        ref = L.dual_run3(T, basis, ub, None, SKIP | LONG)
        limit = int(np.flatnonzero(ref[4][:, 0] == -1)[0]) + 1
        with _fresh(gpu, T, basis, ub) as dt:
            got, want = _node3(dt, _slack_handle(T, basis, ub), [], [], [], 32, flags, max_iter=limit)
            assert want["status"] == L.ITER_LIMIT and want["events"] >= limit


# ---- 9. the forms alternate on one handle ---------------------------------------------------------------------------------
def test_forms_alternate_on_one_handle(gpu):
    n = 40
    dt, root = _solved_handle(gpu, n, 20, 1)
    with dt:
        h = L.Handle(*root)
        steps = 0
        for step, form in enumerate(("launches", "onchip", "launches", "onchip", "auto", "onchip")):
            p = N.pick(h.T, h.basis, h.flip, h.ub, h.lo, n)
            if p["var"] < 0:
                break
            v = float(step % 2)
            flags = LONG if step >= 2 else 0
            got, want = _node3(dt, h, p["var"], v, v, n, flags, form=form, use_graph=1)
            steps += 1
            if want["status"] != L.OPTIMAL:
                break
        assert steps >= 4
        # snapshot and restore between on-chip nodes
        dt.snapshot()
        keep = L.Handle(h.T, h.basis, h.ub, h.flip, h.lo)
        free = [j for j in range(n) if h.ub[j] > 0.0][:2]
        assert len(free) == 2
        _node3(dt, h, free[0], 1.0, 1.0, n)
        dt.restore()
        h = keep
        _same_state(dt, h, "after the restore")
        got, want = _node3(dt, h, free[1], 0.0, 0.0, n)
        # the loop and the pick directly after an on-chip node: they read the contiguous RHS copy and the state it left
        dt.change_bounds(free[0], 1.0, 1.0)
        h.T, h.ub, h.lo = D.change_bounds(h.T, h.ub, h.lo, h.flip, [free[0]], [1.0], [1.0])
        ref = L.dual_run3(h.T, h.basis, h.ub, h.flip, SKIP)
        status, _ = dt.bounded_dual_run(skip_fixed=True)
        assert status == ref[0] and dt.trace().tolist() == ref[4].tolist()
        assert np.array_equal(_u64(dt.download()[0]), _u64(ref[1]))
        if status == L.OPTIMAL:
            pk = dt.branch_pick(n)
            wp = N.pick(ref[1], ref[2], ref[3], h.ub, h.lo, n)
            assert pk["var"] == wp["var"] and pk["candidates"] == wp["candidates"] and _bits(pk["x_var"]) == _bits(wp["x_var"])


# ---- 10. does not fit -----------------------------------------------------------------------------------------------------
def test_node_that_does_not_fit(gpu):
    T, basis, ub = _covering_with_fixed(256, 512, 1)
    assert T.shape == (257, 769) and gpu._lib.lib().lpx_bounded_node_fits(257, 769) == 0
    with _fresh(gpu, T, basis, ub) as dt, _fresh(gpu, T, basis, ub) as other:
        assert not dt.bounded_node_fits()
        before = _state(dt)
        with pytest.raises(gpu.LpxError) as e:
            dt.bounded_node([], [], [], 512, form="onchip")
        assert e.value.code == gpu._lib.EINVAL and "does not fit" in str(e.value)
        assert _state(dt) == before
        got, want = _node3(dt, _slack_handle(T, basis, ub), [], [], [], 512, form="auto", other=other, max_iter=12)
        assert want["status"] == L.ITER_LIMIT and want["events"] == 12


# ---- 11. the driver -------------------------------------------------------------------------------------------------------
def _problem(lpx, c, A, rel, b, sense=0):
    return lpx.LPProblem.from_arrays(sense, c, A, rel, b)


@functools.lru_cache(maxsize=None)
def _want_binary(n, m, seed, flags, max_nodes=0):
    c, A0, b0 = N.binary_model(n, m, seed)
    return L.solve2(c, A0, b0, np.ones(n), search_flags=flags, max_nodes=max_nodes)


def _same_solve(res, want):
    log = res.BnbLog
    assert len(log) == len(want["log"]) == res.Nodes == want["nodes"]
    for k in ("depth", "K", "status", "events", "flips", "var"):
        assert np.array_equal(log[k], want["log"][k]), k
    assert np.array_equal(_u64(log["z"]), _u64(want["log"]["z"])), "z bits of some node differ"
    for k in ("nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K"):
        assert res.BnbInfo[k] == want[k], k
    assert res.Status == want["status"]
    if want["status"] == L.OPTIMAL:
        assert np.array_equal(_u64(res.Solution), _u64(want["x"])) and _bits(res.OptimalValue) == _bits(want["value"])


# model: (nodes, events) with search flags 0; (nodes, events, cut-off nodes) with long step + cutoff
DRIVER = {(16, 8, 1): ((197, 630), (197, 492, 68)), (32, 16, 2): ((1995, 13454), (1987, 9829, 965)),
          (64, 32, 1): ((5721, 60222), (5729, 39971, 2786))}


@pytest.mark.parametrize("flags", [0, LONG | CUT])
@pytest.mark.parametrize("n,m,seed", sorted(DRIVER))
def test_driver_node_log_bit_for_bit(gpu, n, m, seed, flags):
    c, A0, b0 = N.binary_model(n, m, seed)
    want = _want_binary(n, m, seed, flags)
    p = _problem(gpu, c, A0, np.zeros(m, dtype=np.int32), b0)
    kw = dict(long_step=bool(flags & LONG), cutoff=bool(flags & CUT))
    res = gpu.LPSolver().SolveBnbBounded(p, np.ones(n), node_form="onchip", **kw)
    exp = DRIVER[(n, m, seed)][1 if flags else 0]
    assert want["rc"] == 0 and (want["nodes"], want["events"]) == exp[:2]
    if flags:
        assert int((want["log"]["status"] == L.CUTOFF).sum()) == exp[2]
    _same_solve(res, want)
    ref = gpu.LPSolver().SolveBnbBounded(p, np.ones(n), node_form="launches", **kw)
    assert res.BnbLog.tobytes() == ref.BnbLog.tobytes() and res.BnbInfo == ref.BnbInfo
    assert np.array_equal(_u64(res.Solution), _u64(ref.Solution)) and _bits(res.OptimalValue) == _bits(ref.OptimalValue)
    auto = gpu.LPSolver().SolveBnbBounded(p, np.ones(n), node_form="auto", **kw) if (n, flags) == (16, 0) else res
    assert auto.BnbLog.tobytes() == res.BnbLog.tobytes()


@pytest.mark.parametrize("name", ["general", "lowers", "min", "mixed", "infeasible"])
def test_driver_on_small_models(gpu, name):
    c, A, rel, b, upper, lower, is_int, sense = N.small_models()[name]
    want = L.solve2(c, A, b, upper, lower=lower, is_int=is_int, sense=sense, rel=rel)
    res = gpu.LPSolver().SolveBnbBounded(_problem(gpu, c, A, rel, b, sense), upper, lower=lower, integer=is_int, node_form="onchip")
    assert want["nodes"] > 1 and (want["status"] == L.INFEASIBLE) == (name == "infeasible")
    if name == "infeasible":
        assert want["nodes"] == 11
    _same_solve(res, want)


def test_driver_node_limit_on_the_largest_guaranteed_shape(gpu):
    n, m, seed = 128, 64, 1
    c, A0, b0 = N.binary_model(n, m, seed)
    want = _want_binary(n, m, seed, LONG | CUT, 400)
    assert want["rc"] == L.ITER_LIMIT and want["events"] == 2726
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver().SolveBnbBounded(_problem(gpu, c, A0, np.zeros(m, dtype=np.int32), b0), np.ones(n), max_nodes=400,
                                       long_step=True, cutoff=True, node_form="onchip")
    assert e.value.code == gpu._lib.ITER_LIMIT and "node limit" in str(e.value)
    _same_solve(e.value.result, want)


def test_two_solves_in_a_row_give_identical_logs(gpu):
    c, A0, b0 = N.binary_model(32, 16, 2)
    p = _problem(gpu, c, A0, np.zeros(16, dtype=np.int32), b0)
    a = gpu.LPSolver().SolveBnbBounded(p, 1.0, node_form="onchip")
    b = gpu.LPSolver().SolveBnbBounded(p, 1.0, node_form="onchip")
    assert a.BnbLog.tobytes() == b.BnbLog.tobytes() and a.BnbInfo == b.BnbInfo
    assert np.array_equal(_u64(a.Solution), _u64(b.Solution)) and a.OptimalValue == b.OptimalValue


def test_driver_refuses_a_root_that_does_not_fit(gpu):
    from linear_programming_solver_lpr381_amd import synth
    c, A, b = synth.dense_lp(256, 512, seed=1)
    p = _problem(gpu, np.abs(c), np.abs(A), np.zeros(256, dtype=np.int32), np.abs(A).sum(axis=1) * 0.3)
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver().SolveBnbBounded(p, 1.0, node_form="onchip", max_nodes=1)
    assert e.value.code == gpu._lib.EINVAL and "does not fit" in str(e.value)


# ---- 12. the command line -------------------------------------------------------------------------------------------------
def test_cli_node_form(gpu):
    out = {}
    for form in ("launches", "onchip", "auto"):
        r = subprocess.run([CLI, "--binary", "--bnb-bounded", "--node-form", form, EXAMPLE], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "nodes: " in r.stdout and "dual events: " in r.stdout
        out[form] = r.stdout
    assert out["onchip"] == out["launches"] == out["auto"]
    r = subprocess.run([CLI, "--binary", "--node-form", "onchip", EXAMPLE], capture_output=True, text=True)
    assert r.returncode == 64 and "--node-form needs --bnb-bounded" in r.stderr
    r = subprocess.run([CLI, "--binary", "--bnb-bounded", "--node-form", "fast", EXAMPLE], capture_output=True, text=True)
    assert r.returncode == 64 and "--node-form takes" in r.stderr
