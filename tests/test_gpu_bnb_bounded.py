"""GPU tests of branch and bound by bound changes (csrc/lpx_bnb_bounded.hip, csrc/host/bnb_bounded.cpp): lpx_tableau_branch_pick,
lpx_tableau_dualize, lpx_bounded_dual_run2, lpx_bounded_node and lpx_solve_bnb_bounded, bit for bit against the NumPy restatement
of the contract (tests/_bnb_bounded_ref.py) -- picks at the wave, stride and LDS edges of the pick kernel, flips at the lane
blocks of both dualize launches, the flagged loop at the select kernel's edges and on both scratch paths, the cycling node, the
children of solved roots, and the whole node log of the driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bounded_dual_ref as D
import _bounded_ref as B
from _node_helpers import exact as _exact, pick_tableau as _pick_tableau

pytestmark = pytest.mark.gpu

INF = np.inf
REL = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
EXAMPLE = os.path.join(ROOT, "integration", "Input", "example_bounded.txt")


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _bits(x):
    return np.float64(x).view(np.uint64)


def _same_state(dt, T, basis, ub, lo, flip, what=""):
    Tg, bg = dt.download()
    glo, gub, gflip = dt.bound_state()
    assert np.array_equal(_u64(Tg), _u64(T)), "tableau bits differ from the restatement " + what
    assert bg.tolist() == np.asarray(basis).tolist(), what
    assert gflip.tolist() == np.asarray(flip).tolist(), what
    assert np.array_equal(_u64(gub), _u64(ub)) and np.array_equal(_u64(glo), _u64(lo)), what


# ---- branch pick -------------------------------------------------------------------------------------------------------
def _pick_both(lpx, T, basis, ub, nint, flips=(), lo_cols=(), is_int=None, tol=1e-6):
    """The pick on the device and in the restatement; `flips`: nonbasic or basic columns with a finite bound flipped through
    lpx_tableau_dualize; lo_cols: columns given the lower bound 1 through lpx_tableau_change_bounds."""
    T = T.copy()
    m = T.shape[0] - 1
    T[m, list(flips)] = -1.0
    with lpx.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        Tr, flip, lo, ubr = T, np.zeros(len(ub), dtype=np.uint8), np.zeros(len(ub)), ub.copy()
        if len(flips):
            assert dt.dualize() == (len(flips), 0)
            Tr, flip, k, bad = N.dualize(T, ub, flip)
            assert k == len(flips) and bad == 0 and flip[list(flips)].all()
        if len(lo_cols):
            cols = np.array(sorted(lo_cols), dtype=np.int32)
            low, up = np.ones(len(cols)), 1.0 + np.where(np.isinf(ub[cols]), 5.0, ub[cols])
            dt.change_bounds(cols, low, up)
            Tr, ubr, lo = D.change_bounds(Tr, ubr, lo, flip, cols, low, up)
        got = dt.branch_pick(nint, is_int=is_int, tol=tol)
        x = dt.bounded_solution(nint)[0]
    want = N.pick(Tr, basis, flip, ubr, lo, nint, is_int, tol)
    assert np.array_equal(_u64(x), _u64(N.values(Tr, basis, flip, ubr, lo, nint))), "x differs from lpx_tableau_bounded_solution"
    assert got["var"] == want["var"] and got["candidates"] == want["candidates"], (got, want)
    assert _bits(got["x_var"]) == _bits(want["x_var"]) and _bits(got["z"]) == _bits(want["z"]), (got, want)
    return got


@pytest.mark.parametrize("nint", [1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097])
def test_pick_at_every_edge_of_the_kernel(gpu, nint):
    T, basis, ub = _pick_tableau(nint, max(1, nint // 2), nint)
    m = T.shape[0] - 1
    basic = set(basis.tolist())
    finite = [j for j in range(nint) if np.isfinite(ub[j])]
    flips = [j for j in finite if j not in basic][:5] + [j for j in finite if j in basic][:5]
    got = _pick_both(gpu, T, basis, ub, nint, flips=flips)
    assert nint < 63 or got["candidates"] > 0
    lo_cols = list(range(0, nint, 7))[:40]
    _pick_both(gpu, T, basis, ub, nint, flips=flips, lo_cols=lo_cols)              # a non-zero lo
    g = np.random.default_rng(nint)
    mask = (g.random(nint) < 0.5).astype(np.uint8)
    if got["var"] >= 0:
        mask[got["var"]] = 0                                                          # the mask removes the closest candidate
        again = _pick_both(gpu, T, basis, ub, nint, flips=flips, is_int=mask)
        assert again["var"] != got["var"]
    _pick_both(gpu, T, basis, ub, nint, flips=flips, is_int=np.zeros(nint, dtype=np.uint8))


@pytest.mark.parametrize("entries,winner", [
    ({70: 2.75, 1500: 1.25}, 70),            # equal distance in different waves and different 1024-lane strides
    ({70: 2.25, 1500: 1.75}, 70),
    ({5: 0.75, 1029: 0.25}, 5),              # the same lane, two strides
    ({7: 0.75, 1030: 0.25}, 7),              # the lower index sits in the higher lane
    ({1030: 0.25, 2055: 0.75, 3000: 0.125}, 1030),  # a farther candidate behind the tie
    ({63: 0.25, 64: 0.75}, 63),              # across a wave edge
    ({4099: 0.4}, 4099),                     # a candidate only at the last index
])
def test_pick_ties_go_to_the_lowest_index(gpu, entries, winner):
    nint = 4100
    T, basis, ub = _exact(nint, entries)
    got = _pick_both(gpu, T, basis, ub, nint)
    assert got["var"] == winner and got["candidates"] == len(entries) and got["x_var"] == entries[winner]


def test_pick_without_a_candidate_and_at_the_tolerance(gpu):
    T, basis, ub = _exact(300, {3: 2.0, 299: 1.0})
    got = _pick_both(gpu, T, basis, ub, 300)
    assert got == {"var": -1, "candidates": 0, "x_var": 0.0, "z": -3.5}
    T, basis, ub = _exact(300, {3: 0.25, 10: 0.75, 20: 0.5})
    assert _pick_both(gpu, T, basis, ub, 300, tol=0.25)["var"] == 20          # f == tol and 1 - f == tol are no candidates
    assert _pick_both(gpu, T, basis, ub, 20, tol=0.25)["var"] == -1
    assert _pick_both(gpu, T, basis, ub, 300, tol=0.2499)["candidates"] == 3
    assert _pick_both(gpu, T, basis, ub, 0)["var"] == -1                       # nint = 0


def test_pick_with_more_than_1024_rows(gpu):
    T, basis, ub = _pick_tableau(4097, 1100, 5)
    assert T.shape[0] - 1 == 1100
    got = _pick_both(gpu, T, basis, ub, 4097)
    assert got["var"] >= 0
    T, basis, ub = _exact(64, {9: 0.5}, m_extra=1100)
    assert _pick_both(gpu, T, basis, ub, 64)["var"] == 9


# ---- dualize -----------------------------------------------------------------------------------------------------------
def _dualize_case(lpx, R, Cm, seed, mode="random"):
    g = np.random.default_rng(seed)
    T = g.uniform(-1.0, 1.0, size=(R, Cm + 1))
    m = R - 1
    ub = g.uniform(0.5, 3.0, size=Cm)
    if mode == "random":
        kind = g.integers(0, 4, size=Cm)
        ub[kind == 0] = 0.0
        ub[kind == 1] = INF
    elif mode == "empty":
        T[m, :Cm] = np.abs(T[m, :Cm])
    elif mode == "all":
        T[m, :Cm] = -np.abs(T[m, :Cm]) - 1e-3
    basis = g.permutation(Cm + m)[:m].astype(np.int32) % Cm if m else np.zeros(0, dtype=np.int32)
    Tr, flip, k, bad = N.dualize(T, ub, np.zeros(Cm, dtype=np.uint8))
    with lpx.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        assert dt.dualize() == (k, bad)
        _same_state(dt, Tr, basis, ub, np.zeros(Cm), flip, "after dualize")
        if m >= 1:
            # the loop right after reads the contiguous RHS copy the second launch kept current
            ref = N.dual_run2(Tr, basis, ub, flip, N.SKIP_FIXED, max_iter=2)
            status, _ = dt.bounded_dual_run(skip_fixed=True, max_iter=2)
            assert status == ref[0] and dt.trace().tolist() == ref[4].tolist()
            _same_state(dt, ref[1], ref[2], ub, np.zeros(Cm), ref[3], "after the loop")
    return k, bad


@pytest.mark.parametrize("R,Cm", [(2, 1), (255, 1023), (256, 1024), (257, 1025), (1026, 4100), (2, 4100), (1026, 1)])
def test_dualize_at_the_lane_blocks_of_both_launches(gpu, R, Cm):
    k, bad = _dualize_case(gpu, R, Cm, R + Cm)
    assert Cm < 64 or (k > 0 and bad > 0)


@pytest.mark.parametrize("mode", ["empty", "all"])
def test_dualize_with_an_empty_list_and_with_every_column(gpu, mode):
    k, bad = _dualize_case(gpu, 257, 1025, 3, mode)
    assert (k, bad) == ((0, 0) if mode == "empty" else (1025, 0))


def test_dualize_leaves_fixed_and_unbounded_columns_alone(gpu):
    T = np.array([[1.0, 2.0, 3.0, 4.0, 10.0], [-1.0, -1.0, -1.0, 1.0, 5.0]])
    ub = np.array([0.0, INF, 2.0, 1.0])
    basis = np.array([3], dtype=np.int32)
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        assert dt.dualize() == (1, 1)                   # column 2 flipped, column 1 counted, column 0 neither
        Tg, _ = dt.download()
        assert Tg.tolist() == [[1.0, 2.0, -3.0, 4.0, 4.0], [-1.0, -1.0, 1.0, 1.0, 7.0]]
        assert dt.bound_flags().tolist() == [0, 0, 1, 0]
        assert dt.dualize() == (0, 1)


# ---- the flagged dual loop ---------------------------------------------------------------------------------------------
def _flagged(lpx, T, basis, ub, flip=None, dt=None, **opts):
    ref_opts = {k: v for k, v in opts.items() if k in ("eps", "max_iter")}
    ref = N.dual_run2(T, basis, ub, flip, N.SKIP_FIXED, **ref_opts)
    own = dt is None
    if own:
        dt = lpx.DeviceTableau.from_host(T, basis)
        dt.set_bounds(ub)
    try:
        status, st = dt.bounded_dual_run(skip_fixed=True, **opts)
        assert status == ref[0] and dt.trace().tolist() == ref[4].tolist()
        assert dt.bounded_counts() == ref[5] and st["pivots"] == len(ref[4])
        Tg, bg = dt.download()
        assert np.array_equal(_u64(Tg), _u64(ref[1])), "tableau bits differ from the restatement"
        assert bg.tolist() == ref[2].tolist() and dt.bound_flags().tolist() == ref[3].tolist()
    finally:
        if own:
            dt.close()
    return ref


def _covering_with_fixed(m, n, seed):
    T, basis, ub, _ = D.covering(m, n, seed)
    g = np.random.default_rng(seed)
    ub[:n][g.random(n) < 0.2] = 0.0                     # fixed columns: they do not enter
    return T, basis, ub


@pytest.mark.parametrize("m,n,seed", [(1, 3, 1), (2, 1, 1), (63, 960, 1), (64, 960, 1), (65, 960, 1), (1025, 40, 1)])
def test_flagged_loop_at_lane_and_wave_edges(gpu, m, n, seed):
    T, basis, ub = _covering_with_fixed(m, n, seed)
    ref = _flagged(gpu, T, basis, ub)
    fixed = np.flatnonzero(ub == 0.0)
    assert not np.isin(ref[4][:, 1], fixed).any()
    if m >= 63:
        assert len(fixed) > 0 and len(ref[4]) > 0
        plain = D.dual_run(T, basis, ub)
        assert plain[4].tolist() != ref[4].tolist(), "the flag changes nothing on this instance"


def test_flagged_loop_on_both_scratch_paths(gpu):
    T, basis, ub = _covering_with_fixed(8, 4100, 2)
    assert T.shape[1] - 1 == 4108
    assert len(_flagged(gpu, T, basis, ub)[4]) > 0
    T, basis, ub = _covering_with_fixed(4100, 24, 3)
    assert T.shape == (4101, 4125)
    assert len(_flagged(gpu, T, basis, ub)[4]) > 0


def _solved_handle(lpx, n, m, seed):
    T, basis, ub, model, Ts, bs, flip = D.root(n, m, seed)
    dt = lpx.DeviceTableau.from_host(T, basis)
    dt.set_bounds(ub)
    status, _ = dt.bounded_run()
    Tg, bg = dt.download()
    assert status == B.OPTIMAL and np.array_equal(_u64(Tg), _u64(Ts)) and dt.bound_flags().tolist() == flip.tolist()
    dt.snapshot()
    return dt, (Ts, bs, ub, flip)


def test_cycling_node_ends_optimal_with_the_restatement_trace(gpu):
    Tc, bs, ubc, flip = N.cycling_node()
    dt, root = _solved_handle(gpu, 64, 32, 1)
    with dt:
        cols = np.array(sorted(N.CYCLING_ONES + N.CYCLING_ZEROS), dtype=np.int32)
        vals = np.array([1.0 if j in N.CYCLING_ONES else 0.0 for j in cols])
        dt.change_bounds(cols, vals, vals)
        assert np.array_equal(_u64(dt.download()[0]), _u64(Tc))
        assert dt.dualize() == (0, 0)
        ref = _flagged(gpu, Tc, bs, ubc, flip, dt=dt)
        assert ref[0] == N.OPTIMAL and len(ref[4]) == 21


def test_the_two_forms_keep_their_graphs_apart_and_flags_zero_is_the_old_loop(gpu):
    L = gpu._lib.lib()
    dt, root = _solved_handle(gpu, 40, 20, 2)
    Ts, bs, ub, flip = root
    kids = D.children(40, 20, 2)
    with dt:
        for rnd in range(2):
            for j, l, u in kids[:2]:
                Tc, ubc, _ = D.change_bounds(Ts, ub, np.zeros(len(ub)), flip, [j], [l], [u])
                dt.restore(); dt.change_bounds(j, l, u)
                _flagged(gpu, Tc, bs, ubc, flip, dt=dt)
                want = D.dual_run(Tc, bs, ubc, flip)
                for form in ("old", "flags0"):
                    dt.restore(); dt.change_bounds(j, l, u)
                    if form == "old":
                        status, _ = dt.bounded_dual_run()
                    else:
                        o = gpu.default_opts(True)
                        st = gpu._lib.Stats()
                        status = gpu._lib.check(L.lpx_bounded_dual_run2(dt._h, C.byref(o), 0, gpu._lib.NULL_CB, None, C.byref(st)))
                    assert status == want[0] and dt.trace().tolist() == want[4].tolist()
                    assert np.array_equal(_u64(dt.download()[0]), _u64(want[1]))
        o = gpu.default_opts(True)
        assert L.lpx_bounded_dual_run2(dt._h, C.byref(o), 2, gpu._lib.NULL_CB, None, None) == gpu._lib.EINVAL
        assert "unknown flag" in gpu._lib.last_error()


def test_flagged_loop_does_not_depend_on_batch_graph_or_callback(gpu):
    T, basis, ub = _covering_with_fixed(20, 40, 1)
    seen = []
    for opts in ({"batch": 1}, {"batch": 7}, {"use_graph": 0}, {"batch": 3, "use_graph": 0}):
        _flagged(gpu, T, basis, ub, **opts)
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        status, _ = dt.bounded_dual_run(skip_fixed=True, cb=lambda it, r, q: seen.append((r, q)))
        ref = N.dual_run2(T, basis, ub, None, N.SKIP_FIXED)
        assert status == ref[0] and seen == [tuple(e) for e in ref[4].tolist()]
        assert np.array_equal(_u64(dt.download()[0]), _u64(ref[1]))


# ---- lpx_bounded_node --------------------------------------------------------------------------------------------------
REC_KEYS = ("status", "events", "kind0", "kind1", "flips", "unrepairable", "var", "candidates")


def _node_both(dt, h, cols, lower, upper, n, **kw):
    cols = np.atleast_1d(np.asarray(cols, dtype=np.int32))
    lower = np.broadcast_to(np.asarray(lower, dtype=np.float64), cols.shape)
    upper = np.broadcast_to(np.asarray(upper, dtype=np.float64), cols.shape)
    want = h.node(cols, lower, upper, n, **kw)
    got = dt.bounded_node(cols, lower, upper, n, **kw)
    assert {k: got[k] for k in REC_KEYS} == {k: want[k] for k in REC_KEYS}, (got, want)
    assert _bits(got["x_var"]) == _bits(want["x_var"]) and _bits(got["z"]) == _bits(want["z"]), (got, want)
    assert dt.trace().tolist() == h.trace.tolist()
    _same_state(dt, h.T, h.basis, h.ub, h.lo, h.flip, "after the node")
    return got


@pytest.mark.parametrize("n,m,seed", [(12, 6, 1), (40, 20, 1), (64, 32, 2)])
def test_node_on_the_children_of_a_root_and_with_no_change(gpu, n, m, seed):
    dt, root = _solved_handle(gpu, n, m, seed)
    with dt:
        got = _node_both(dt, N.Handle(*root), [], [], [], n)                      # K = 0: the root itself
        assert got["status"] == N.OPTIMAL and got["events"] == 0 and got["var"] >= 0
        for j, l, u in D.children(n, m, seed):
            dt.restore()
            _node_both(dt, N.Handle(*root), j, l, u, n)


def test_node_relaxing_after_fixing_forces_flips(gpu):
    n = 40
    dt, root = _solved_handle(gpu, n, 20, 1)
    with dt:
        h = N.Handle(*root)
        fixed, flips = [], 0
        for step in range(6):                                                     # a dive: fix the pick at 0, 1, 0, ...
            p = N.pick(h.T, h.basis, h.flip, h.ub, h.lo, n)
            if p["var"] < 0:
                break
            v = float(step % 2)
            got = _node_both(dt, h, p["var"], v, v, n)
            fixed.append(p["var"])
            if got["status"] != N.OPTIMAL:
                break
        assert len(fixed) >= 3
        got = _node_both(dt, h, sorted(fixed), 0.0, 1.0, n)                       # back to the root bounds in one call
        assert got["status"] == N.OPTIMAL and got["flips"] > 0, "relaxing the fixed columns needed no flip: the test shows nothing"
        assert abs(got["z"] - root[0][-1, -1]) <= REL * abs(root[0][-1, -1])       # the root's optimum again


def test_node_refuses_an_unrepairable_column_and_leaves_the_handle_alone(gpu):
    T, basis, ub, _ = B.binary_bounded(12, 6, 1)
    ub = ub.copy(); ub[2] = INF                          # T[m,2] = -c_2 < 0 with no upper bound
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        for cols, low, up in (([], [], []), ([0, 5], [0.0, 1.0], [0.0, 1.0])):
            with pytest.raises(gpu.LpxError) as e:
                dt.bounded_node(cols, low, up, 12)
            assert e.value.code == gpu._lib.EINVAL and "no upper bound" in str(e.value)
            _same_state(dt, T, basis, ub, np.zeros(len(ub)), np.zeros(len(ub), dtype=np.uint8), "after the refused node")
        with pytest.raises(gpu.LpxError) as e:                                     # argument errors, handle untouched
            dt.bounded_node([0], [0.0], [1.0], 99)
        assert "nint" in str(e.value)
        with pytest.raises(gpu.LpxError) as e:
            dt.bounded_node([0], [0.0], [1.0], 12, tol=0.5)
        assert "tol" in str(e.value)
        with pytest.raises(gpu.LpxError) as e:
            dt.bounded_node([0, 0], [0.0, 0.0], [1.0, 1.0], 12)
        assert "repeats a column" in str(e.value)
        _same_state(dt, T, basis, ub, np.zeros(len(ub)), np.zeros(len(ub), dtype=np.uint8), "after argument errors")


def test_change_bounds_and_node_share_one_staging_buffer_across_regrowth(gpu):
    """lpx_tableau_change_bounds and lpx_bounded_node stage their edits in one buffer of the handle, with one layout (lower, upper,
    shift, saved (ub, lo), cols: 44 bytes per column, grown to twice the need).  K = 1 sizes it (88 bytes), K = 3 regrows it (264),
    the refused K = 6 fills those 264 bytes to the last one and restores ub / lo from the save area, K = 2 and K = 0 then run on the
    larger buffer.  The seed is one for which the restatement accepts every step but the third and finds that one unrepairable
    (chosen on the CPU: steps two and five end OPTIMAL after 5 events each, the fifth with one flip)."""
    n, m, seed = 10, 4, 2
    dt, root = _solved_handle(gpu, n, m, seed)
    p = np.random.default_rng(seed).permutation(n)
    with dt:
        h = N.Handle(*root)

        def change(cols, lower, upper, what):
            dt.change_bounds(cols, lower, upper)
            h.T, h.ub, h.lo = D.change_bounds(h.T, h.ub, h.lo, h.flip, cols, lower, upper)
            _same_state(dt, h.T, h.basis, h.ub, h.lo, h.flip, what)

        change(p[:1], [1.0], [1.0], "after change_bounds with K = 1")
        got = _node_both(dt, h, np.sort(p[1:4]), [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], n)            # K = 3
        assert got["status"] == N.OPTIMAL and got["events"] > 0
        # K = 6: the four edited columns and two more relaxed, to +inf where the column is not flipped (+inf on a flipped one is an
        # argument error, not this refusal); a fixed column the loop left with a negative reduced cost is then beyond repair
        cols = np.sort(p[:6])
        upper = np.where(h.flip[cols] != 0, 1.0, INF)
        before = (h.T.copy(), h.basis.copy(), h.ub.copy(), h.lo.copy(), h.flip.copy())
        want = h.node(cols, np.zeros(6), upper, n)
        assert want["status"] is None and want["unrepairable"] > 0 and np.isinf(upper).any()
        with pytest.raises(gpu.LpxError) as e:
            dt.bounded_node(cols, np.zeros(6), upper, n)
        assert e.value.code == gpu._lib.EINVAL and "%d column(s)" % want["unrepairable"] in str(e.value)
        _same_state(dt, *before, "after the refused node")
        change(np.sort(p[[0, 2]]), [0.0, 0.0], [1.0, 1.0], "after change_bounds with K = 2")
        got = _node_both(dt, h, [], [], [], n)                                                   # K = 0
        assert got["status"] == N.OPTIMAL and got["flips"] > 0


# ---- the driver --------------------------------------------------------------------------------------------------------
def _problem(lpx, c, A, rel, b, sense=0):
    return lpx.LPProblem.from_arrays(sense, c, A, rel, b)


def _solve_both(lpx, c, A, rel, b, upper, lower=None, is_int=None, sense=0, **kw):
    want = N.solve(c, A, b, upper, lower=lower, is_int=is_int, sense=sense, rel=rel, **kw)
    res = lpx.LPSolver(**({"max_iter": kw["max_iter"]} if "max_iter" in kw else {})).SolveBnbBounded(
        _problem(lpx, c, A, rel, b, sense), upper, lower=lower, integer=is_int, max_nodes=kw.get("max_nodes", 0))
    return res, want


def _same_solve(res, want):
    log = res.BnbLog
    assert len(log) == len(want["log"]) == res.Nodes == want["nodes"]
    for k in ("depth", "K", "status", "events", "flips", "var"):
        assert np.array_equal(log[k], want["log"][k]), k
    assert np.array_equal(_u64(log["z"]), _u64(want["log"]["z"])), "z bits of some node differ"
    for k in ("nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K"):
        assert res.BnbInfo[k] == want[k], k
    assert _bits(res.BnbInfo["constant"]) == _bits(want["constant"])
    assert res.Aux == [float(want["nodes"]), float(want["events"]), float(want["flips"]), float(want["incumbents"])]
    assert res.Status == want["status"]
    if want["status"] == N.OPTIMAL:
        assert np.array_equal(_u64(res.Solution), _u64(want["x"])) and _bits(res.OptimalValue) == _bits(want["value"])


@pytest.mark.parametrize("n,m,seed", [(16, 8, 1), (32, 16, 2), (64, 32, 1)])
def test_driver_node_log_bit_for_bit(gpu, n, m, seed):
    c, A0, b0 = N.binary_model(n, m, seed)
    res, want = _solve_both(gpu, c, A0, np.zeros(m, dtype=np.int32), b0, np.ones(n))
    assert want["rc"] == 0 and want["nodes"] > 100 and want["flips"] > 0
    _same_solve(res, want)


def test_driver_against_the_rows_form_branch_and_bound(gpu):
    from linear_programming_solver_lpr381_amd import synth
    c, A, rel, b = synth.binary_ip(16, 8, 1)
    rows = gpu.LPSolver().Solve(_problem(gpu, c, A, rel, b), "Branch and Bound")
    res = gpu.LPSolver().SolveBnbBounded(_problem(gpu, c, A[:8], rel[:8], b[:8]), 1.0)
    print("bounded", res.OptimalValue, "rows form", rows.OptimalValue, "nodes", res.Nodes, rows.Nodes)
    assert res.Status == N.OPTIMAL and abs(res.OptimalValue - rows.OptimalValue) <= REL * abs(rows.OptimalValue)
    assert float(c @ res.Solution) == res.OptimalValue or abs(float(c @ res.Solution) - res.OptimalValue) <= REL * res.OptimalValue


@pytest.mark.parametrize("leg,n,m,seed", [("max_nodes", 16, 8, 1), ("max_iter", 32, 16, 2)])
def test_driver_limits_return_the_incumbent_so_far(gpu, leg, n, m, seed):
    c, A0, b0 = N.binary_model(n, m, seed)
    rel = np.zeros(m, dtype=np.int32)
    full = N.solve(c, A0, b0, np.ones(n))
    first = int(np.flatnonzero((full["log"]["var"] < 0) & (full["log"]["status"] == N.OPTIMAL))[0])    # the first incumbent
    # max_iter: one event short of the longest node (the root's primal solve needs fewer events than that)
    kw = {"max_nodes": first + 2} if leg == "max_nodes" else {"max_iter": int(full["log"]["events"].max()) - 1}
    want = N.solve(c, A0, b0, np.ones(n), **kw)
    assert want["rc"] == N.ITER_LIMIT and want["incumbents"] > 0 and want["status"] == N.OPTIMAL
    with pytest.raises(gpu.SolverException) as e:
        _solve_both(gpu, c, A0, rel, b0, np.ones(n), **kw)
    assert e.value.code == gpu._lib.ITER_LIMIT and "node" in str(e.value)
    _same_solve(e.value.result, want)
    if leg == "max_iter":
        assert want["log"]["status"][-1] == N.ITER_LIMIT and "iteration limit" in str(e.value)


@pytest.mark.parametrize("name", ["general", "lowers", "min", "mixed", "infeasible"])
def test_driver_on_small_models(gpu, name):
    c, A, rel, b, upper, lower, is_int, sense = N.small_models()[name]
    res, want = _solve_both(gpu, c, A, rel, b, upper, lower=lower, is_int=is_int, sense=sense)
    assert want["nodes"] > 1 and (want["status"] == N.INFEASIBLE) == (name == "infeasible")
    _same_solve(res, want)


def test_two_solves_in_a_row_give_identical_logs(gpu):
    c, A0, b0 = N.binary_model(32, 16, 2)
    p = _problem(gpu, c, A0, np.zeros(16, dtype=np.int32), b0)
    a = gpu.LPSolver().SolveBnbBounded(p, 1.0)
    b = gpu.LPSolver().SolveBnbBounded(p, 1.0)
    assert a.BnbLog.tobytes() == b.BnbLog.tobytes() and a.BnbInfo == b.BnbInfo
    assert np.array_equal(_u64(a.Solution), _u64(b.Solution)) and a.OptimalValue == b.OptimalValue


def test_cli_bnb_bounded(gpu):
    # Max 3 x1 + 5 x2 + 2 x3, x1 + 2 x2 + 2 x3 <= 10, 2 x1 + 4 x2 + 3 x3 <= 15, u = (4, 3, 3): the LP optimum is 20.75, the
    # integer optimum 19 (enumerated by hand: x = (4, 1, 1) and (3, 2, 0))
    r = subprocess.run([CLI, "--upper", "1=4", "--upper", "2=3", "--upper", "3=3", "--bnb-bounded", EXAMPLE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "z* = 19\n" in r.stdout and "nodes: " in r.stdout and "dual events: " in r.stdout
    r = subprocess.run([CLI, "--bnb-bounded", EXAMPLE], capture_output=True, text=True)
    assert r.returncode == 64 and "--bnb-bounded needs" in r.stderr
