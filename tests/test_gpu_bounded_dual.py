"""GPU tests of the bounded dual simplex (lpx_bounded_dual_run) and of the bound change on a solved tableau
(lpx_tableau_change_bounds), csrc/lpx_bounded_dual.hip: bit for bit against the NumPy restatement of the contract
(tests/_bounded_dual_ref.py) -- trace with its encoding, tableau, basis, flip, ub, lo, status, counts -- at the lane and wave
edges of the select kernel, on both global-scratch paths, on the children of solved 0/1 roots and a four-column change; the
decision edges on small exact tableaux; equality with lpx_dual_run when no column is bounded; independence of batching, graph
replay and callbacks; snapshot / restore; the argument errors that need a live handle; the bounded session."""
import numpy as np
import pytest

import _bounded_dual_ref as D
import _bounded_ref as B
from linear_programming_solver_lpr381_amd import synth

pytestmark = pytest.mark.gpu

INF = np.inf
REL = 1e-9


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _state(dt, status, st):
    Tg, bg = dt.download()
    lo, ub, flip = dt.bound_state()
    return status, Tg, bg, flip, dt.trace(), dt.bounded_counts(), ub, lo, st


def _gpu_dual(lpx, T, basis, ub, cap=None, cb=None, **opts):
    dt = lpx.DeviceTableau.from_host(T, basis) if cap is None else lpx.DeviceTableau.with_capacity(T, basis, *cap)
    with dt:
        if ub is not None:
            dt.set_bounds(ub)
        status, st = dt.bounded_dual_run(cb=cb, **opts)
        return _state(dt, status, st)


def _same(got, ref, ub=None, lo=None):
    status, Tg, bg, flip, tr, counts, gub, glo, st = got
    rstatus, Tr, br, rflip, rtr, rcounts = ref
    assert status == rstatus
    assert tr.tolist() == rtr.tolist()
    assert counts == rcounts
    assert bg.tolist() == br.tolist()
    assert flip.tolist() == rflip.tolist()
    assert np.array_equal(_u64(Tg), _u64(Tr)), "tableau bits differ from the restatement"
    assert st["pivots"] == rcounts[0] + rcounts[1] == len(rtr)
    if ub is not None:
        assert np.array_equal(_u64(gub), _u64(np.asarray(ub, dtype=np.float64)))
    assert np.array_equal(_u64(glo), _u64(np.zeros(len(glo)) if lo is None else lo))


def _check(lpx, T, basis, ub, cap=None, **opts):
    ref_opts = {k: v for k, v in opts.items() if k in ("eps", "max_iter")}
    if "ratio_tol" in opts:
        ref_opts["tol"] = opts["ratio_tol"]
    ref = D.dual_run(T, basis, ub, **ref_opts)
    got = _gpu_dual(lpx, T, basis, ub, cap=cap, **opts)
    _same(got, ref, ub=ub)
    return got, ref


# ---- lane and wave edges: C-1 = 1023 / 1024 / 1025, m across one wave and across the kernel's 1024 lanes -------------------------
@pytest.mark.parametrize("m,n,seed,events", [(1, 3, 1, 1), (2, 1, 1, 1), (63, 960, 1, 1052), (64, 960, 1, 1010), (65, 960, 1, 927),
                                             (1025, 40, 1, 107), (1025, 40, 4, 116)])
def test_lane_and_wave_edges(gpu, m, n, seed, events):
    T, basis, ub, _ = D.covering(m, n, seed)
    got, ref = _check(gpu, T, basis, ub)
    assert got[0] == D.OPTIMAL and len(got[4]) == events
    if m >= 63:
        assert got[5][0] > 0 and got[5][1] > 0          # both kinds of event


def test_column_ratios_in_global_scratch(gpu):
    T, basis, ub, _ = D.covering(8, 4100, 2)
    assert T.shape[1] - 1 == 4108
    got, ref = _check(gpu, T, basis, ub)
    assert got[0] == D.OPTIMAL and len(got[4]) == 1456 and got[5] == (11, 1445, 0)


def test_row_array_in_global_scratch(gpu):
    T, basis, ub, _ = D.covering(4100, 24, 3)
    assert T.shape == (4101, 4125)
    got, ref = _check(gpu, T, basis, ub)
    assert got[0] == D.OPTIMAL and len(got[4]) == 96 and got[5] == (93, 3, 0)


def test_spare_capacity(gpu):
    T, basis, ub, _ = D.covering(20, 40, 1)
    _check(gpu, T, basis, ub, cap=(40, 100))


# ---- children of solved roots: change_bounds + bounded_dual_run on the handle bounded_run solved ---------------------------------
class _Ref:
    """The restatement's copy of a handle: tableau, basis, ub, lo, flip."""

    def __init__(self, Ts, bs, ub, flip):
        self.T, self.basis, self.ub, self.flip = Ts.copy(), bs.copy(), ub.copy(), flip.copy()
        self.lo = np.zeros(len(ub))

    def edit(self, dt, cols, lower, upper, **opts):
        """The same edit on both sides, compared after the change and after the run."""
        cols = np.atleast_1d(np.asarray(cols, dtype=np.int32))
        lower = np.broadcast_to(np.asarray(lower, dtype=np.float64), cols.shape)
        upper = np.broadcast_to(np.asarray(upper, dtype=np.float64), cols.shape)
        self.T, self.ub, self.lo = D.change_bounds(self.T, self.ub, self.lo, self.flip, cols, lower, upper)
        dt.change_bounds(cols, lower, upper)
        Tg, bg = dt.download()
        lo, ub, flip = dt.bound_state()
        assert np.array_equal(_u64(Tg), _u64(self.T)), "tableau bits differ after the change"
        assert bg.tolist() == self.basis.tolist() and flip.tolist() == self.flip.tolist()
        assert np.array_equal(_u64(ub), _u64(self.ub)) and np.array_equal(_u64(lo), _u64(self.lo))
        ref = D.dual_run(self.T, self.basis, self.ub, self.flip)
        status, st = dt.bounded_dual_run(**opts)
        _same(_state(dt, status, st), ref, ub=self.ub, lo=self.lo)
        _, self.T, self.basis, self.flip, _, _ = ref
        return ref


def _solved_handle(lpx, n, m, seed):
    T, basis, ub, model, Ts, bs, flip = D.root(n, m, seed)
    dt = lpx.DeviceTableau.from_host(T, basis)
    dt.set_bounds(ub)
    status, _ = dt.bounded_run()
    Tg, bg = dt.download()
    assert status == B.OPTIMAL and np.array_equal(_u64(Tg), _u64(Ts)) and dt.bound_flags().tolist() == flip.tolist()
    dt.snapshot()
    return dt, (Ts, bs, ub, flip)


@pytest.mark.parametrize("seed", (1, 2))
@pytest.mark.parametrize("n,m", B.BINARY_SHAPES)
def test_children_of_binary_roots(gpu, n, m, seed):
    kids = D.children(n, m, seed)
    assert kids
    dt, root = _solved_handle(gpu, n, m, seed)
    with dt:
        for j, l, u in kids:
            dt.restore()
            ref = _Ref(*root)
            assert j in root[1].tolist()                # a fractional variable is basic: the change is on a basic column
            r = ref.edit(dt, j, l, u)
            assert r[0] == D.OPTIMAL
            x, z, _ = dt.bounded_solution(n)
            xr, zr, _ = D.solution(ref.T, ref.basis, ref.flip, ref.ub, ref.lo, n)
            assert np.array_equal(_u64(x), _u64(xr)) and z == zr
            r = ref.edit(dt, j, 0.0, 1.0)               # loosening back to [0, 1] continues from the child's tableau
            assert r[0] == D.OPTIMAL
            assert abs(dt.bounded_solution(n)[1] - root[0][-1, -1]) <= REL * max(1.0, abs(root[0][-1, -1]))


def test_four_column_change_and_zero_shift_on_a_flipped_column(gpu):
    cols, lower, upper = D.four_column_change()
    dt, root = _solved_handle(gpu, 64, 32, 1)
    with dt:
        ref = _Ref(*root)
        assert root[3][cols].any()
        r = ref.edit(dt, cols, lower, upper)
        assert r[0] == D.OPTIMAL and len(r[4]) > 0
        dt.restore()
        ref = _Ref(*root)
        j = int(np.flatnonzero(root[3][:64])[0])        # a flipped column given the bounds it has: s = ub - u' == 0
        before = dt.download()[0]
        r = ref.edit(dt, j, 0.0, 1.0)
        assert r[0] == D.OPTIMAL and len(r[4]) == 0 and np.array_equal(_u64(dt.download()[0]), _u64(before))
        k = int(np.flatnonzero(root[3][:64] == 0)[0])   # a zero shift beside a real one in the same call
        r = ref.edit(dt, [j, k], [0.0, 1.0], [1.0, 1.0])
        assert r[0] in (D.OPTIMAL, D.INFEASIBLE)


def test_the_two_bounded_loops_keep_their_graphs_apart(gpu):
    """Same options on both loops of one handle: each replays its own captured launches."""
    dt, root = _solved_handle(gpu, 40, 20, 2)
    with dt:
        j = D.children(40, 20, 2)[0][0]
        for _ in range(2):
            dt.restore()
            dt.change_bounds(j, 1.0, 1.0)
            Tc, ubc, lo = D.change_bounds(root[0], root[2], np.zeros(len(root[2])), root[3], [j], [1.0], [1.0])
            want = D.dual_run(Tc, root[1], ubc, root[3], tol=1e-9)
            status, st = dt.bounded_dual_run(ratio_tol=1e-9)
            _same(_state(dt, status, st), want, ub=ubc, lo=lo)
            T, basis, ub = D.root(40, 20, 2)[:3]
            dt.upload(T, basis)
            dt.set_bounds(ub)
            status, _ = dt.bounded_run(ratio_tol=1e-9)
            assert status == B.OPTIMAL and np.array_equal(_u64(dt.download()[0]), _u64(root[0]))


# ---- decision edges, small integer tableaux, every quantity exact -----------------------------------------------------------
def _tab(rows, obj, basis):
    return np.array(rows + [obj], dtype=np.float64), np.array(basis, dtype=np.int32)


@pytest.mark.parametrize("tol,second,q", [(1e-12, 2.0, 0), (0.5, 1.75, 0), (1e-12, 1.75, 1)])
def test_hysteresis_keeps_the_earlier_column_within_ratio_tol(gpu, tol, second, q):
    # columns x0, x1, s (basic in row 0), RHS; ratios 2 / 1 and second / 1
    T, basis = _tab([[-1, -1, 1, -2]], [2, second, 0, 0], [2])
    got, ref = _check(gpu, T, basis, np.array([INF, INF, INF]), ratio_tol=tol, max_iter=1)
    assert got[4].tolist() == [[0, q]]


def test_first_index_wins_among_equal_w(gpu):
    # row 0: basic s0 with u = 1 at 4 (w = 1 - 4 = -3, kind 1); row 1: basic s1 at -3 (w = -3, kind 0)
    T, basis = _tab([[1, 1, 0, 4], [-1, 0, 1, -3]], [1, 0, 0, 0], [1, 2])
    got, ref = _check(gpu, T, basis, np.array([INF, 1.0, INF]), max_iter=1)
    assert got[4].tolist() == [[-2, 0]] and got[3].tolist() == [0, 1, 0]
    T, basis = _tab([[-1, 1, 0, -3], [-2, 0, 1, -3]], [1, 0, 0, 0], [1, 2])
    got, ref = _check(gpu, T, basis, np.array([INF, INF, INF]), max_iter=1)
    assert got[4].tolist() == [[0, 0]]
    T, basis = _tab([[-1, 1, 0, -3], [-2, 0, 1, -4]], [1, 0, 0, 0], [1, 2])          # the strict minimum, not the first negative
    got, ref = _check(gpu, T, basis, np.array([INF, INF, INF]), max_iter=1)
    assert got[4].tolist() == [[1, 0]]


def test_a_bound_exceeded_by_less_than_eps_does_not_take_part(gpu):
    T, basis = _tab([[1, 1, 0, 1.0 + 5e-10], [1, 0, 1, 2]], [1, 0, 0, 0], [1, 2])
    got, ref = _check(gpu, T, basis, np.array([INF, 1.0, INF]))
    assert got[0] == D.OPTIMAL and len(got[4]) == 0 and np.array_equal(_u64(got[1]), _u64(T))
    T[0, 3] = 1.0 + 5e-9                                # above eps: the row leaves at its bound
    got, ref = _check(gpu, T, basis, np.array([INF, 1.0, INF]), max_iter=1)
    assert got[4].tolist() == [[-2, 0]]


def test_infeasible_after_a_complement_leaves_it_in_place(gpu):
    # columns x0, x1, s0 (u = 1, basic in row 0 at 3), s1, RHS: complemented, row 0 has no negative entry
    T, basis = _tab([[-1, -2, 1, 0, 3], [1, 1, 0, 1, 2]], [1, 1, 0, 0, 0], [2, 3])
    got, ref = _check(gpu, T, basis, np.array([INF, INF, 1.0, INF]))
    assert got[0] == D.INFEASIBLE and len(got[4]) == 0 and got[5] == (0, 0, 0)
    assert got[1][0].tolist() == [1.0, 2.0, 1.0, 0.0, -2.0] and got[3].tolist() == [0, 0, 1, 0]
    assert got[1][1:].tolist() == T[1:].tolist() and got[2].tolist() == [2, 3]
    T, basis = _tab([[1, 1, -3]], [1, 0, 0], [1])   # kind 0: nothing is rewritten
    got, ref = _check(gpu, T, basis, np.array([INF, INF]))
    assert got[0] == D.INFEASIBLE and np.array_equal(_u64(got[1]), _u64(T)) and not got[3].any()


@pytest.mark.parametrize("max_iter", [0, 1, 5])
def test_iteration_limit(gpu, max_iter):
    T, basis, ub, _ = D.covering(20, 40, 1)
    got, ref = _check(gpu, T, basis, ub, max_iter=max_iter)
    assert got[0] == D.ITER_LIMIT and len(got[4]) == max_iter


# ---- no bounded column = lpx_dual_run(fdf_guard = 0, cleanup = 0) -----------------------------------------------------------------
@pytest.mark.parametrize("m,n,seed", [(6, 12, 1), (64, 128, 2), (128, 256, 3)])
def test_without_bounds_it_is_the_dual_loop(gpu, m, n, seed):
    T, basis, _, _ = D.covering(m, n, seed)
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        ds, dst = dt.dual_run(fdf_guard=0, cleanup=0)
        dT, db = dt.download()
        dtr = dt.trace()
    assert len(dtr) > 0
    for ub in (np.full(T.shape[1] - 1, INF), None):     # every ub = +inf, and a handle that never had bounds
        got = _gpu_dual(gpu, T, basis, ub)
        assert got[0] == ds and got[4].tolist() == dtr.tolist() and got[2].tolist() == db.tolist()
        assert np.array_equal(_u64(got[1]), _u64(dT))
        assert not got[3].any() and got[5] == (len(dtr), 0, 0) and got[8]["pivots"] == dst["pivots"]


# ---- the bits do not depend on how the launches are issued ---------------------------------------------------------------------
def test_batching_graph_and_callback_do_not_change_the_result(gpu):
    T, basis, ub, _ = D.covering(20, 40, 1)
    ref = D.dual_run(T, basis, ub)
    assert ref[5][0] > 0 and ref[5][1] > 0
    for opts in ({"use_graph": 0}, {"batch": 1}, {"batch": 7}, {"batch": 7, "use_graph": 0}, {"profile": 1}, {}):
        _same(_gpu_dual(gpu, T, basis, ub, **opts), ref, ub=ub)
    seen = []
    _same(_gpu_dual(gpu, T, basis, ub, cb=lambda it, r, q: seen.append((it, r, q))), ref, ub=ub)
    assert seen == [(k + 1, int(r), int(q)) for k, (r, q) in enumerate(ref[4])]
    seen.clear()
    _same(_gpu_dual(gpu, T, basis, ub, cb=lambda it, r, q: seen.append((it, r, q)), batch=3), ref, ub=ub)
    assert [(r, q) for _, r, q in seen] == [tuple(e) for e in ref[4].tolist()]


def test_snapshot_restore_carry_lo_and_the_solution_adds_it(gpu):
    n, m = 40, 20
    dt, root = _solved_handle(gpu, n, m, 2)
    Ts, bs, ub, flip = root
    with dt:
        # a handle that never had a change: bounded_solution's bits are the bounded primal's
        x, z, up = dt.bounded_solution(n)
        xr, zr, upr = B.solution(Ts, bs, flip, ub, n)
        assert np.array_equal(_u64(x), _u64(xr)) and z == zr and up.tolist() == upr.tolist()
        lo, gub, gflip = dt.bound_state()
        assert not lo.any() and np.array_equal(_u64(gub), _u64(ub)) and gflip.tolist() == flip.tolist()
        j = D.children(n, m, 2)[0][0]
        ref = _Ref(*root)
        ref.edit(dt, j, 0.25, 0.75)                     # a non-zero lower shift
        dt.snapshot()
        kept = (ref.T.copy(), ref.basis.copy(), ref.ub.copy(), ref.lo.copy(), ref.flip.copy())
        x, z, _ = dt.bounded_solution(n)
        xr, zr, _ = D.solution(ref.T, ref.basis, ref.flip, ref.ub, ref.lo, n)
        assert np.array_equal(_u64(x), _u64(xr)) and z == zr and 0.25 - 1e-9 <= x[j] <= 0.75 + 1e-9
        ref.edit(dt, j, 1.0, 1.0)
        assert dt.bound_state()[0][j] == 1.0
        dt.restore()
        lo, gub, gflip = dt.bound_state()
        Tg, bg = dt.download()
        assert np.array_equal(_u64(Tg), _u64(kept[0])) and bg.tolist() == kept[1].tolist()
        assert np.array_equal(_u64(gub), _u64(kept[2])) and np.array_equal(_u64(lo), _u64(kept[3])) and gflip.tolist() == kept[4].tolist()
        x2, z2, _ = dt.bounded_solution(n)
        assert np.array_equal(_u64(x2), _u64(x)) and z2 == z
        dt.set_bounds(ub)                               # new bounds: every lo back to +0.0, every flip cleared
        lo, _, gflip = dt.bound_state()
        assert not lo.any() and not np.signbit(lo).any() and not gflip.any()


def test_bound_state_without_bounds(gpu):
    T, basis, _, _ = D.covering(6, 12, 1)
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        lo, ub, flip = dt.bound_state()
        assert not lo.any() and np.isposinf(ub).all() and not flip.any() and len(lo) == len(ub) == len(flip) == T.shape[1] - 1


def test_change_bounds_argument_errors_leave_the_handle_untouched(gpu):
    L, EINVAL = gpu._lib.lib(), gpu._lib.EINVAL
    dt, root = _solved_handle(gpu, 12, 6, 1)
    Ts, bs, ub, flip = root
    j = int(np.flatnonzero(flip[:12])[0])               # flipped in the root
    k = int(np.flatnonzero(flip[:12] == 0)[0])
    Cm = Ts.shape[1] - 1
    with dt:
        def err(cols, lower, upper, what):
            with pytest.raises(gpu.LpxError) as e:
                dt.change_bounds(cols, lower, upper)
            assert e.value.code == EINVAL and what in str(e.value), str(e.value)
            Tg, bg = dt.download()
            lo, gub, gflip = dt.bound_state()
            assert np.array_equal(_u64(Tg), _u64(Ts)) and np.array_equal(_u64(gub), _u64(ub)) and not lo.any()
            assert gflip.tolist() == flip.tolist()
        assert L.lpx_tableau_change_bounds(dt._h, -1, None, None, None) == EINVAL and "negative" in gpu._lib.last_error()
        assert L.lpx_tableau_change_bounds(dt._h, 1, None, None, None) == EINVAL and "null array" in gpu._lib.last_error()
        err([Cm], 0.0, 1.0, "outside")
        err([-1], 0.0, 1.0, "outside")
        err([k, k], 0.0, 1.0, "repeats")
        err([k], np.nan, 1.0, "NaN")
        err([k], 0.0, np.nan, "NaN")
        err([k], -INF, 1.0, "not finite")
        err([k], INF, INF, "not finite")
        err([k], 1.0, 0.5, "below")
        err([k, j], [0.0, 0.0], [1.0, INF], "flipped column")
        dt.change_bounds([k], 0.0, INF)                 # +inf on an unflipped column is fine
        assert np.isposinf(dt.bound_state()[1][k])
        dt.change_bounds([], [], [])                    # K = 0: nothing but the loop-state reset
        dt.set_shape(Ts.shape[0], Ts.shape[1] - 1)      # another live C: the bounds no longer belong to the tableau
        for call in (lambda: dt.change_bounds([0], 0.0, 1.0), dt.bounded_dual_run, dt.bound_state):
            with pytest.raises(gpu.LpxError) as e:
                call()
            assert e.value.code == EINVAL and "live shape changed" in str(e.value)
        dt.set_shape(*Ts.shape)
        with pytest.raises(gpu.LpxError) as e:
            dt.bounded_dual_run(resident=1)
        assert e.value.code == EINVAL and "resident" in str(e.value)
        dt.set_bounds(None)
        with pytest.raises(gpu.LpxError) as e:
            dt.change_bounds([0], 0.0, 1.0)
        assert e.value.code == EINVAL and "no bounds" in str(e.value)


# ---- the model level: a bounded session ----------------------------------------------------------------------------------------
def _problem(lpx, c, A, b, sense=0):
    return lpx.LPProblem.from_arrays(sense, c, A, np.zeros(len(b), dtype=np.int32), b)


def test_open_bounded_equals_solve_bounded(gpu):
    c, A, rel, b = synth.binary_ip(64, 32, 1)
    p = _problem(gpu, c, A[:32], b[:32])
    res = gpu.LPSolver().SolveBounded(p, upper=1.0)
    with gpu.LPSolver().OpenBounded(p, upper=1.0) as s:
        r = s.result
        assert r.Status == res.Status == gpu._lib.OPTIMAL and r.Trace.tolist() == res.Trace.tolist()
        assert np.array_equal(_u64(r.Tableau), _u64(res.Tableau)) and r.Basis.tolist() == res.Basis.tolist()
        assert np.array_equal(_u64(r.Solution), _u64(res.Solution)) and r.OptimalValue == res.OptimalValue
        assert r.Aux == res.Aux and r.Report == res.Report and r.Summary == res.Summary and r.BoundCounts == res.BoundCounts
    s.close()                                           # closing twice is harmless
    with pytest.raises(gpu.SolverException):
        s.set_bounds([0], 0.0, 1.0)
    hand = _problem(gpu, [3.0, 5.0, 2.0], [[1.0, 2.0, 2.0], [2.0, 4.0, 3.0]], [10.0, 15.0])
    for kw in ({}, {"upper": [4, 3, 3]}, {"upper": [4, 3, 3], "lower": [1, 0.5, 0]}):
        res = gpu.LPSolver().SolveBounded(hand, **kw)
        with gpu.LPSolver().OpenBounded(hand, **kw) as s:
            assert s.result.Trace.tolist() == res.Trace.tolist() and np.array_equal(_u64(s.result.Tableau), _u64(res.Tableau))
            assert np.array_equal(_u64(s.result.Solution), _u64(res.Solution)) and s.result.OptimalValue == res.OptimalValue


def test_session_children_match_highs_and_the_device_level_path(gpu):
    n, m, seed = 64, 32, 1
    c, A, rel, b = synth.binary_ip(n, m, seed)
    A0, b0 = A[:m], b[:m]
    kids = D.children(n, m, seed)
    assert len(kids) == 6
    dt, root = _solved_handle(gpu, n, m, seed)
    with dt, gpu.LPSolver().OpenBounded(_problem(gpu, c, A0, b0), upper=1.0) as s:
        state = {}                                      # the session keeps its edits: bounds of every variable so far
        for j, l, u in kids:
            res = s.set_bounds([j], l, u)
            state[j] = (l, u)
            lw, up = np.zeros(n), np.ones(n)
            for v, (a, z) in state.items():
                lw[v], up[v] = a, z
            hst, obj = D.highs_bounded(c, A0, b0, lw, up)
            assert hst == D.OPTIMAL and res.Status == gpu._lib.OPTIMAL
            print("session", j, l, res.OptimalValue, obj)
            assert abs(res.OptimalValue - obj) <= REL * max(1.0, abs(obj))
            x = res.Solution
            assert abs(float(c @ x) - obj) <= REL * max(1.0, abs(obj))
            assert (x >= lw - 1e-9).all() and (x <= up + 1e-9).all() and (A0 @ x <= b0 + 1e-6).all()
            assert res.Aux[2] == 1.0 and res.Aux[3] == 0.0 and res.BoundCounts[:2] == (int(res.Aux[0]), int(res.Aux[1]))
            # the device-level path, the same chain of edits on a handle of its own
            dt.change_bounds([j], l, u)
            status, st = dt.bounded_dual_run()
            assert status == res.Status and dt.trace().tolist() == res.Trace.tolist()
            assert np.array_equal(_u64(dt.download()[0]), _u64(res.Tableau))
            xd, zd, _ = dt.bounded_solution(n)
            assert np.array_equal(_u64(xd), _u64(x)) and zd == res.OptimalValue and st["pivots"] == res.Stats["pivots"]


def test_session_x_matches_highs_on_fresh_children(gpu):
    n, m, seed = 64, 32, 1
    c, A, rel, b = synth.binary_ip(n, m, seed)
    A0, b0 = A[:m], b[:m]
    from scipy.optimize import linprog
    for j, l, u in D.children(n, m, seed):
        with gpu.LPSolver().OpenBounded(_problem(gpu, c, A0, b0), upper=1.0) as s:
            res = s.set_bounds([j], l, u)
        bounds = [(0.0, 1.0)] * n
        bounds[j] = (l, u)
        hs = linprog(-c, A_ub=A0, b_ub=b0, bounds=bounds, method="highs")
        assert hs.status == 0 and res.Status == gpu._lib.OPTIMAL
        print("child", j, l, res.OptimalValue, -hs.fun, np.abs(res.Solution - hs.x).max())
        assert abs(res.OptimalValue + hs.fun) <= REL * max(1.0, abs(hs.fun))
        assert np.abs(res.Solution - hs.x).max() <= REL * max(1.0, np.abs(hs.x).max())


def test_session_infeasible_edit_then_loosening_ends_optimal(gpu):
    n, m = 64, 32
    c, A, rel, b = synth.binary_ip(n, m, 1)
    with gpu.LPSolver().OpenBounded(_problem(gpu, c, A[:m], b[:m]), upper=1.0) as s:
        root = s.result.OptimalValue
        allv = np.arange(n)
        res = s.set_bounds(allv, 1.0, 1.0)              # every x = 1 violates every row (b = half the row sum)
        assert res.Status == gpu._lib.INFEASIBLE
        res = s.set_bounds(allv, 0.0, 1.0)
        assert res.Status == gpu._lib.OPTIMAL
        assert abs(res.OptimalValue - root) <= REL * max(1.0, abs(root))
        with pytest.raises(gpu.SolverException) as e:
            s.set_bounds([0, 0], 0.0, 1.0)
        assert e.value.code == gpu._lib.EINVAL and "twice" in str(e.value)
        with pytest.raises(gpu.SolverException) as e:
            s.set_bounds([n], 0.0, 1.0)
        assert e.value.code == gpu._lib.EINVAL
        with pytest.raises(gpu.SolverException) as e:
            s.set_bounds([0], 1.0, 0.0)
        assert e.value.code == gpu._lib.EINVAL and "below its lower bound" in str(e.value)
        with pytest.raises(gpu.SolverException) as e:
            s.set_bounds([0], -INF, 0.0)
        assert e.value.code == gpu._lib.EINVAL and "not finite" in str(e.value)


def test_session_min_model_with_lower_bounds_at_open(gpu):
    c = np.array([3.0, 5.0, 2.0]); A = np.array([[1.0, 2.0, 2.0], [2.0, 4.0, 3.0]]); b = np.array([10.0, 15.0])
    l = np.array([1.0, 0.5, 0.0]); u = np.array([4.0, 3.0, 3.0])
    from scipy.optimize import linprog
    with gpu.LPSolver().OpenBounded(_problem(gpu, -c, A, b, sense=1), upper=u, lower=l) as s:
        hs = linprog(-c, A_ub=A, b_ub=b, bounds=list(zip(l, u)), method="highs")
        assert abs(s.result.OptimalValue - hs.fun) <= REL * max(1.0, abs(hs.fun))
        const = s.result.Aux[3]
        assert const == -(3.0 * 1.0) + -(5.0 * 0.5)
        for var, lv, uv in ((0, 1.5, 2.0), (1, 0.0, 1.0), (2, 0.5, 3.0), (0, 1.0, 4.0)):
            l[var], u[var] = lv, uv
            res = s.set_bounds([var], lv, uv)
            hs = linprog(-c, A_ub=A, b_ub=b, bounds=list(zip(l, u)), method="highs")
            assert res.Status == gpu._lib.OPTIMAL and hs.status == 0
            print("min model", var, res.OptimalValue, hs.fun, res.Solution, hs.x)
            assert abs(res.OptimalValue - hs.fun) <= REL * max(1.0, abs(hs.fun))
            assert abs(float(-c @ res.Solution) - hs.fun) <= REL * max(1.0, abs(hs.fun))
            assert (res.Solution >= l - 1e-9).all() and (res.Solution <= u + 1e-9).all() and (A @ res.Solution <= b + 1e-9).all()
            assert res.Aux[3] == const and res.Aux[2] == 1.0


def test_session_on_an_unbounded_open_solve_is_an_argument_error(gpu):
    p = _problem(gpu, [1.0, 1.0], [[1.0, -1.0]], [1.0])
    with gpu.LPSolver().OpenBounded(p) as s:
        assert s.result.Status == gpu._lib.UNBOUNDED
        with pytest.raises(gpu.SolverException) as e:
            s.set_bounds([0], 0.0, 1.0)
        assert e.value.code == gpu._lib.EINVAL and "did not end OPTIMAL" in str(e.value)
