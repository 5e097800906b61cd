"""GPU tests of the long-step ratio test, the objective cutoff and the dual start (csrc/lpx_bounded_long.hip,
lpx_bounded_dual_run3, lpx_bounded_node2, lpx_solve_bnb_bounded2, lpx_solve_bounded_dual), bit for bit against the NumPy
restatement of the contract (tests/_bounded_long_ref.py): trace, tableau as uint64, basis, flip, ub, lo, status, counts -- the
long step at the lane, wave and scratch edges of the select kernel, constructed events, the cutoff rule, every flag set on one
handle with graphs on, independence of batch, graph and callback, the node call, the whole node log of the flagged driver, the
dual start at the model level and one CLI run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bounded_dual_ref as D
import _bounded_long_ref as L
import _bounded_ref as B

pytestmark = pytest.mark.gpu

INF = np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
EXAMPLE = os.path.join(ROOT, "integration", "Input", "example_bounded.txt")
LONG, CUT, SKIP = L.LONG_STEP, L.CUTOFF_FLAG, L.SKIP_FIXED

_REF = {}


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _bits(x):
    return np.float64(x).view(np.uint64)


def _cached(key, fn):
    """A reference computed once and shared by the tests that need it (it is never written to)."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _run3(lpx, dt, flags, cutoff=0.0, cb=None, **opts):
    """lpx_bounded_dual_run3 itself, whatever the flags (the Python wrapper routes flags without a new bit to the old calls)."""
    from linear_programming_solver_lpr381_amd.tableau import _wrap_cb
    o = lpx.default_opts(True, **opts)
    st = lpx._lib.Stats()
    c = _wrap_cb(cb)
    rc = lpx._lib.check(lpx._lib.lib().lpx_bounded_dual_run3(dt._h, C.byref(o), int(flags), float(cutoff), c, None, C.byref(st)))
    return rc, st.as_dict()


def _same_state(dt, ref, ub, lo=None, what=""):
    Tg, bg = dt.download()
    glo, gub, gflip = dt.bound_state()
    assert np.array_equal(_u64(Tg), _u64(ref[1])), "tableau bits differ from the restatement " + what
    assert bg.tolist() == ref[2].tolist() and gflip.tolist() == ref[3].tolist(), what
    assert np.array_equal(_u64(gub), _u64(ub)), what
    assert np.array_equal(_u64(glo), _u64(np.zeros(len(ub)) if lo is None else lo)), what


def _long(lpx, T, basis, ub, flip=None, dt=None, flags=LONG, cutoff=-INF, ref=None, **opts):
    """One run on the device and in the restatement, compared in everything the contract names.  Returns the restatement's tuple."""
    ref_opts = {k: v for k, v in opts.items() if k in ("eps", "max_iter")}
    if ref is None:
        ref = L.dual_run3(T, basis, ub, flip, flags, cutoff, **ref_opts)
    own = dt is None
    if own:
        dt = lpx.DeviceTableau.from_host(T, basis)
        dt.set_bounds(ub)
    try:
        status, st = _run3(lpx, dt, flags, cutoff, **opts)
        assert status == ref[0], (status, ref[0])
        assert dt.trace().tolist() == ref[4].tolist(), "trace differs from the restatement"
        assert dt.bounded_counts() == ref[5] and st["pivots"] == ref[5][0] + ref[5][1]
        _same_state(dt, ref, ub, what="(flags %d)" % flags)
    finally:
        if own:
            dt.close()
    return ref


# ---- the long step at the edges of the select kernel ---------------------------------------------------------------------
@pytest.mark.parametrize("m,n,seed", [(1, 3, 1), (2, 1, 1), (63, 960, 1), (64, 960, 1), (65, 960, 1), (1025, 40, 1)])
def test_long_step_at_lane_and_wave_edges(gpu, m, n, seed):
    """From the slack basis, so that passes occur.  (63 / 64 / 65, 960): Cm = 1023, 1024, 1025, the edges of the 1024-lane ratio
    strip; (1025, 40): R = 1026, the second trip of the in-kernel column rewrite."""
    T, basis, ub, _ = D.covering(m, n, seed)
    ref = _long(gpu, T, basis, ub)
    assert ref[0] == L.OPTIMAL
    if m >= 63:
        assert ref[5][2] > 0, "no column passed"
        assert L.least_reduced_cost(ref[1], ref[2], ub) >= -1e-9


def test_long_step_on_both_scratch_paths(gpu):
    T, basis, ub, _ = D.covering(8, 4100, 2)
    assert T.shape[1] - 1 == 4108                                        # the ratios go through global scratch
    assert _long(gpu, T, basis, ub)[5][2] > 0
    T, basis, ub, _ = D.covering(4100, 24, 3)
    assert T.shape == (4101, 4125)                                       # w and the ratios both
    assert _long(gpu, T, basis, ub)[5][2] > 0


# ---- constructed events ------------------------------------------------------------------------------------------------
def _hand(costs, row, rhs, ub):
    from linear_programming_solver_lpr381_amd import synth
    T, basis = synth.primal_tableau_from(-np.asarray(costs, dtype=np.float64), np.array([row], dtype=np.float64),
                                         np.array([rhs], dtype=np.float64))
    return T, basis, np.array(list(ub) + [INF])


def _kind1_then_pass():
    """A child of a solved root whose first pivot is on a kind-1 row (the basic variable above its new upper bound) with at least
    one pass in front of it: (T, basis, ub, flip, lo) after the bound change."""
    for n, m, seed in ((40, 20, 1), (64, 32, 2), (64, 32, 1), (12, 6, 1)):
        _, _, ub, _, Ts, bs, flip = D.root(n, m, seed)
        for j, l, u in D.children(n, m, seed):
            Tc, ubc, lo = D.change_bounds(Ts, ub, np.zeros(len(ub)), flip, [j], [l], [u])
            Tz, fz, _, bad = N.dualize(Tc, ubc, flip)
            tr = L.dual_run3(Tz, bs, ubc, fz, LONG)[4]
            pivots = np.flatnonzero(tr[:, 0] != -1)
            if len(pivots) and pivots[0] > 0 and tr[pivots[0], 0] <= -2:
                return (n, m, seed), (j, l, u), (Tz, bs, ubc, fz, lo)
    return None


def test_kind1_row_followed_by_a_pass(gpu):
    """The complement trap: the passes subtract from the complemented T[r,Cm]; complementing after them rounds differently."""
    found = _cached("kind1", _kind1_then_pass)
    assert found is not None, "no instance with a pass in front of a kind-1 pivot"
    (n, m, seed), (j, l, u), (Tz, bs, ubc, fz, lo) = found
    T, basis, ub, *_ = D.root(n, m, seed)
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        assert dt.bounded_run()[0] == B.OPTIMAL
        dt.change_bounds(j, l, u)
        dt.dualize()
        assert np.array_equal(_u64(dt.download()[0]), _u64(Tz))
        ref = L.dual_run3(Tz, bs, ubc, fz, LONG)
        status, st = _run3(gpu, dt, LONG)
        assert status == ref[0] and dt.trace().tolist() == ref[4].tolist() and dt.bounded_counts() == ref[5]
        _same_state(dt, ref, ubc, lo, "after a kind-1 event with passes")


def test_every_candidate_passes_and_the_event_ends_infeasible(gpu):
    T, basis, ub = _hand([1.0, 2.0], [-1.0, -1.0], -3.0, [1.0, 1.0])             # x1 + x2 >= 3 over 0 <= x <= 1
    ref = _long(gpu, T, basis, ub)
    assert ref[0] == L.INFEASIBLE and ref[4].tolist() == [[-1, 0], [-1, 1]] and ref[5] == (0, 0, 2)
    assert ref[1][0].tolist() == [1.0, 1.0, 1.0, -1.0] and ref[3].tolist() == [1, 1, 0]      # the passes stay applied


@pytest.mark.parametrize("flags", [LONG, LONG | SKIP, CUT, CUT | LONG, CUT | LONG | SKIP])
def test_kind1_row_without_an_entering_column_stays_complemented(gpu, flags):
    """The tableau of test_gpu_bounded_dual.test_infeasible_after_a_complement_leaves_it_in_place: columns x0, x1, s0 (u = 1, basic
    in row 0 at 3), s1, RHS.  Row 0 is complemented in place in every form, has no negative entry afterwards, and stays so."""
    T = np.array([[-1, -2, 1, 0, 3], [1, 1, 0, 1, 2], [1, 1, 0, 0, 0]], dtype=np.float64)
    basis = np.array([2, 3], dtype=np.int32)
    ref = _long(gpu, T, basis, np.array([INF, INF, 1.0, INF]), flags=flags, cutoff=-INF)
    assert ref[0] == L.INFEASIBLE and len(ref[4]) == 0 and ref[5] == (0, 0, 0)
    assert np.array_equal(_u64(ref[1][0]), _u64(np.array([1.0, 2.0, 1.0, -0.0, -2.0])))      # the sign of the zero is part of the bits
    assert ref[3].tolist() == [0, 0, 1, 0]
    assert np.array_equal(_u64(ref[1][1:]), _u64(T[1:])) and ref[2].tolist() == [2, 3]


def test_an_unbounded_column_stops_the_chain(gpu):
    T, basis, ub = _hand([1.0, 2.0, 3.0], [-1.0, -1.0, -1.0], -3.5, [1.0, INF, 1.0])
    ref = _long(gpu, T, basis, ub)
    assert ref[0] == L.OPTIMAL and ref[4].tolist() == [[-1, 0], [0, 1]]          # x2 enters although row 0 stays below zero after it


def test_two_equal_ratios(gpu):
    T, basis, ub = _hand([1.0, 1.0, 2.0], [-1.0, -1.0, -1.0], -2.5, [1.0, 1.0, 1.0])
    ref = _long(gpu, T, basis, ub)
    assert ref[4].tolist() == [[-1, 0], [-1, 1], [0, 2]]                         # the tie goes to the lower index, then the other
    T, basis, ub = _hand([1.0, 1.0, 2.0], [-1.0, -1.0, -1.0], -1.5, [1.0, 1.0, 1.0])
    ref = _long(gpu, T, basis, ub)
    assert ref[4].tolist() == [[-1, 0], [0, 1]]


def test_a_fixed_column_passes_without_skip_fixed_and_stays_out_with_it(gpu):
    T, basis, ub = _hand([1.0, 2.0], [-1.0, -1.0], -0.5, [0.0, 1.0])
    ref = _long(gpu, T, basis, ub, flags=LONG)
    assert ref[4].tolist() == [[-1, 0], [0, 1]] and ref[3].tolist() == [1, 0, 0]
    ref = _long(gpu, T, basis, ub, flags=LONG | SKIP)
    assert ref[4].tolist() == [[0, 1]] and ref[3].tolist() == [0, 0, 0]


# ---- the cutoff --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [CUT, CUT | LONG, CUT | SKIP, CUT | LONG | SKIP])
def test_cutoff_rule(gpu, flags):
    T, basis, ub, _ = D.covering(20, 40, 1)
    full = _cached(("cut-full", flags), lambda: L.dual_run3(T, basis, ub, None, flags & ~CUT))
    # step 1b is tested once per pivot, in front of the leaving row: the events done there, and z as it stands there
    bnd = [0] + [int(i) + 1 for i in np.flatnonzero(full[4][:, 0] != -1)]
    zs = _cached(("cut-z", flags), lambda: [L.dual_run3(T, basis, ub, None, flags & ~CUT, max_iter=e)[1][-1, -1] for e in bnd])
    assert all(a >= b for a, b in zip(zs, zs[1:])), "z rose in the dual loop"
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        dt.snapshot()
        # fired in front of the first event: zero events, the handle untouched (<=: equality fires)
        ref = _long(gpu, T, basis, ub, dt=dt, flags=flags, cutoff=T[-1, -1])
        assert ref[0] == L.CUTOFF and len(ref[4]) == 0 and np.array_equal(_u64(ref[1]), _u64(T))
        # -inf never fires
        dt.restore()
        ref = _long(gpu, T, basis, ub, dt=dt, flags=flags, cutoff=-INF)
        assert ref[0] == L.OPTIMAL and ref[4].tolist() == full[4].tolist()
        # z exactly equal to the cutoff in the middle of the run; then two more cutoffs on the same handle with equal options:
        # each run obeys its own value (it is not baked into the cached graph)
        ends = []
        for k in (len(zs) // 2, len(zs) // 4, 3 * len(zs) // 4):
            dt.restore()
            ref = _long(gpu, T, basis, ub, dt=dt, flags=flags, cutoff=zs[k])
            first = next(i for i, z in enumerate(zs) if z <= zs[k])           # equality fires; a degenerate pivot may get there earlier
            assert ref[0] == L.CUTOFF and len(ref[4]) == bnd[first] and _bits(ref[1][-1, -1]) == _bits(zs[first])
            ends.append(len(ref[4]))
        assert len(set(ends)) == 3, "three cutoffs ended at %s" % ends
        # just above the optimum: the run is not cut off where z > cutoff holds to the end
        dt.restore()
        ref = _long(gpu, T, basis, ub, dt=dt, flags=flags, cutoff=np.nextafter(zs[-1], -INF))
        assert ref[0] == L.OPTIMAL
        with pytest.raises(gpu.LpxError) as e:
            _run3(gpu, dt, flags, float("nan"))
        assert e.value.code == gpu._lib.EINVAL and "NaN" in str(e.value)
        with pytest.raises(gpu.LpxError) as e:
            _run3(gpu, dt, flags | 8)
        assert "unknown flag" in str(e.value)


# ---- graphs and independence -------------------------------------------------------------------------------------------
def test_all_flag_sets_alternate_on_one_handle_with_graphs_on(gpu):
    T, basis, ub, _ = D.covering(20, 40, 1)
    ub = ub.copy(); ub[:40][np.random.default_rng(1).random(40) < 0.2] = 0.0     # fixed columns: SKIP_FIXED matters
    plain = N.dual_run2(T, basis, ub, None, 0)
    mid = 0.5 * (T[-1, -1] + plain[1][-1, -1])
    refs = {f: L.dual_run3(T, basis, ub, None, f, mid) for f in range(8)}
    assert len({r[4].tobytes() for r in refs.values()}) >= 6, "the flag sets do not differ on this instance"
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        dt.snapshot()
        for rnd in range(2):
            for f in (6, 0, 2, 1, 7, 4, 3, 5):
                dt.restore()
                _long(gpu, T, basis, ub, dt=dt, flags=f, cutoff=mid, ref=refs[f], use_graph=1)
        # flags without the new bits: lpx_bounded_dual_run2 on the device, bit for bit
        for f in (0, 1):
            dt.restore()
            status, _ = dt.bounded_dual_run(skip_fixed=bool(f))
            old = (status, dt.download(), dt.trace().tolist(), dt.bound_flags().tolist(), dt.bounded_counts())
            dt.restore()
            status, _ = _run3(gpu, dt, f, 123.0)
            new = (status, dt.download(), dt.trace().tolist(), dt.bound_flags().tolist(), dt.bounded_counts())
            assert old[0] == new[0] and old[2:] == new[2:] and old[1][1].tolist() == new[1][1].tolist()
            assert np.array_equal(_u64(old[1][0]), _u64(new[1][0]))


def test_long_step_does_not_depend_on_batch_graph_or_callback(gpu):
    T, basis, ub, _ = D.covering(20, 40, 1)
    ref = L.dual_run3(T, basis, ub, None, LONG)
    assert ref[5][2] > 0
    for opts in ({"batch": 1}, {"batch": 7}, {"use_graph": 0}, {"batch": 3, "use_graph": 0}):
        _long(gpu, T, basis, ub, ref=ref, **opts)
    seen = []
    with gpu.DeviceTableau.from_host(T, basis) as dt:
        dt.set_bounds(ub)
        status, st = dt.bounded_dual_run(long_step=True, cb=lambda it, r, q: seen.append((it, r, q)))
        assert status == ref[0] and [(r, q) for _, r, q in seen] == [tuple(e) for e in ref[4].tolist()]
        assert [it for it, _, _ in seen] == list(range(1, len(seen) + 1))
        _same_state(dt, ref, ub, what="with a callback")
    # the iteration limit is tested between pivots only: a run may end past it by the passes of its last launch
    limit = int(np.flatnonzero(ref[4][:, 0] == -1)[0]) + 1
    cut = _long(gpu, T, basis, ub, max_iter=limit)
    assert cut[0] == L.ITER_LIMIT and len(cut[4]) >= limit and cut[4].tolist() == ref[4][: len(cut[4])].tolist()


# ---- lpx_bounded_node2 -------------------------------------------------------------------------------------------------
REC_KEYS = ("status", "events", "kind0", "kind1", "flips", "unrepairable", "var", "candidates")


def _solved_handle(lpx, n, m, seed):
    T, basis, ub, model, Ts, bs, flip = D.root(n, m, seed)
    dt = lpx.DeviceTableau.from_host(T, basis)
    dt.set_bounds(ub)
    status, _ = dt.bounded_run()
    assert status == B.OPTIMAL and np.array_equal(_u64(dt.download()[0]), _u64(Ts))
    dt.snapshot()
    return dt, (Ts, bs, ub, flip)


def _node_both(dt, h, cols, lower, upper, n, flags, cutoff):
    cols = np.atleast_1d(np.asarray(cols, dtype=np.int32))
    lower = np.broadcast_to(np.asarray(lower, dtype=np.float64), cols.shape)
    upper = np.broadcast_to(np.asarray(upper, dtype=np.float64), cols.shape)
    want = h.node2(cols, lower, upper, n, flags=SKIP | flags | (0 if cutoff is None else CUT), cutoff=-INF if cutoff is None else cutoff)
    got = dt.bounded_node(cols, lower, upper, n, long_step=bool(flags & LONG), cutoff=cutoff)
    assert {k: got[k] for k in REC_KEYS} == {k: want[k] for k in REC_KEYS}, (got, want)
    assert _bits(got["x_var"]) == _bits(want["x_var"]) and _bits(got["z"]) == _bits(want["z"]), (got, want)
    assert dt.trace().tolist() == h.trace.tolist()
    Tg, bg = dt.download()
    glo, gub, gflip = dt.bound_state()
    assert np.array_equal(_u64(Tg), _u64(h.T)) and bg.tolist() == h.basis.tolist() and gflip.tolist() == h.flip.tolist()
    assert np.array_equal(_u64(gub), _u64(h.ub)) and np.array_equal(_u64(glo), _u64(h.lo))
    return got


@pytest.mark.parametrize("n,m,seed", [(12, 6, 1), (40, 20, 1), (64, 32, 2)])
def test_node2_on_the_children_of_a_root(gpu, n, m, seed):
    dt, root = _solved_handle(gpu, n, m, seed)
    z_root = root[0][-1, -1]
    statuses = set()
    with dt:
        for j, l, u in D.children(n, m, seed):
            plain = N.Handle(*root).node([j], [l], [u], n)
            for flags, cutoff in ((LONG, None), (0, 0.5 * (z_root + plain["z"])), (LONG, 0.5 * (z_root + plain["z"])),
                                  (0, -INF), (0, z_root)):
                dt.restore()
                got = _node_both(dt, L.Handle(*root), j, l, u, n, flags, cutoff)
                statuses.add(got["status"])
                if got["status"] == L.CUTOFF:
                    assert got["var"] == -1 and got["candidates"] == 0 and got["x_var"] == 0.0
            # flags = LPX_BDUAL_SKIP_FIXED: lpx_bounded_node bit for bit
            dt.restore()
            rec = gpu._lib.NodeRecord()
            cols = np.array([j], dtype=np.int32); lo = np.array([l]); up = np.array([u])
            o = gpu.default_opts(True)
            gpu._lib.check(gpu._lib.lib().lpx_bounded_node2(dt._h, 1, cols.ctypes.data_as(gpu._lib.ip), lo.ctypes.data_as(gpu._lib.dp),
                                                            up.ctypes.data_as(gpu._lib.dp), C.byref(o), SKIP, 0.0, n, None, 1e-6,
                                                            C.byref(rec)))
            a = (rec.status, rec.events, rec.kind0, rec.kind1, rec.flips, rec.pick.var, _bits(rec.pick.z), dt.trace().tolist(),
                 _u64(dt.download()[0]).tolist())
            dt.restore()
            old = dt.bounded_node(j, l, u, n)
            b = (old["status"], old["events"], old["kind0"], old["kind1"], old["flips"], old["var"], _bits(old["z"]),
                 dt.trace().tolist(), _u64(dt.download()[0]).tolist())
            assert a == b
    assert L.CUTOFF in statuses and L.OPTIMAL in statuses


# ---- the flagged driver ------------------------------------------------------------------------------------------------
def _problem(lpx, c, A, rel, b, sense=0):
    return lpx.LPProblem.from_arrays(sense, c, A, rel, b)


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


@pytest.mark.parametrize("flags", [LONG, CUT, LONG | CUT])
@pytest.mark.parametrize("n,m,seed", [(16, 8, 1), (32, 16, 2), (64, 32, 1)])
def test_flagged_driver_node_log_bit_for_bit(gpu, n, m, seed, flags):
    c, A0, b0 = N.binary_model(n, m, seed)
    want = L.solve2(c, A0, b0, np.ones(n), search_flags=flags)
    res = gpu.LPSolver().SolveBnbBounded(_problem(gpu, c, A0, np.zeros(m, dtype=np.int32), b0), np.ones(n),
                                         long_step=bool(flags & LONG), cutoff=bool(flags & CUT))
    assert want["rc"] == 0 and want["nodes"] > 100
    assert bool(flags & CUT) == bool((want["log"]["status"] == L.CUTOFF).any())
    _same_solve(res, want)


@pytest.mark.parametrize("n,m,seed", [(16, 8, 1), (32, 16, 2), (64, 32, 1)])
def test_search_flags_zero_is_the_old_driver_on_the_device(gpu, n, m, seed):
    c, A0, b0 = N.binary_model(n, m, seed)
    p = _problem(gpu, c, A0, np.zeros(m, dtype=np.int32), b0)
    old = gpu.LPSolver().SolveBnbBounded(p, np.ones(n))
    from linear_programming_solver_lpr381_amd.solver import _problem_struct, _solve_opts, BNB_LOG_DTYPE
    o, keep = _solve_opts(gpu.LPSolver().engine)
    ps, hold = _problem_struct(p)
    up = np.ones(n)
    r, info = gpu._lib.Result(), gpu._lib.BnbBoundedInfo()
    rc = gpu._lib.lib().lpx_solve_bnb_bounded2(C.byref(ps), None, up.ctypes.data_as(gpu._lib.dp), None, C.byref(o), 0, 0, C.byref(r),
                                               C.byref(info))
    try:
        assert rc == 0
        log = np.zeros(info.n_log, dtype=BNB_LOG_DTYPE)
        C.memmove(log.ctypes.data, info.log, info.n_log * C.sizeof(gpu._lib.BnbNodeLog))
        assert log.tobytes() == old.BnbLog.tobytes()
        assert _bits(r.optimal_value) == _bits(old.OptimalValue) and info.pruned_bound == old.BnbInfo["pruned_bound"]
    finally:
        gpu._lib.lib().lpx_bnb_bounded_info_free(C.byref(info))
        gpu._lib.lib().lpx_result_free(C.byref(r))


# ---- the dual start at the model level ---------------------------------------------------------------------------------
def _same_dual_start(res, want):
    assert res.Status == want["status"] == L.OPTIMAL
    assert res.Trace.tolist() == want["trace"].tolist()
    assert np.array_equal(_u64(res.Tableau), _u64(want["T"])) and res.Basis.tolist() == want["basis"].tolist()
    assert res.Flips.tolist() == want["flip"].tolist()
    assert np.array_equal(_u64(res.Solution), _u64(want["x"])) and _bits(res.OptimalValue) == _bits(want["value"])
    assert res.BoundCounts == want["counts"] and _bits(res.Aux[3]) == _bits(want["constant"])
    assert "dual start: %d dual-feasibility flips, %d passes" % (want["dualize_flips"], want["counts"][2]) in res.Summary


def test_dual_start_on_a_covering_model(gpu):
    c, A, rel, b = L.covering_model(32, 96, 1)
    p = _problem(gpu, c, A, rel, b, sense=1)
    for long_step in (True, False):
        want = L.solve_bounded_dual(c, A, rel, b, 1.0, sense=1, flags=LONG if long_step else 0)
        res = gpu.LPSolver().SolveBoundedDual(p, 1.0, long_step=long_step)
        _same_dual_start(res, want)
        assert (want["counts"][2] > 0) == long_step
    with pytest.raises(gpu.SolverException) as e:                            # the primal root refuses this model
        gpu.LPSolver().SolveBounded(p, upper=1.0)
    assert e.value.code == gpu._lib.E_GE_PRESENT


def test_dual_start_on_a_mixed_model(gpu):
    c, A, rel, b, upper, lower, sense = L.mixed_model()
    want = L.solve_bounded_dual(c, A, rel, b, upper, lower, sense)
    assert want["dualize_flips"] > 0 and min(want["counts"]) > 0
    res = gpu.LPSolver().SolveBoundedDual(_problem(gpu, c, A, rel, b, sense), upper, lower=lower)
    _same_dual_start(res, want)


def test_dual_start_reports_an_infeasible_model(gpu):
    # x1 + x2 >= 3 over 0 <= x <= 1
    p = _problem(gpu, [1.0, 2.0], [[1.0, 1.0]], [1], [3.0], sense=1)
    res = gpu.LPSolver().SolveBoundedDual(p, 1.0)
    assert res.Status == L.INFEASIBLE and res.Trace.tolist() == [[-1, 0], [-1, 1]] and res.BoundCounts == (0, 0, 2)


def test_cli_long_step_and_cutoff(gpu):
    # Max 3 x1 + 5 x2 + 2 x3, x1 + 2 x2 + 2 x3 <= 10, 2 x1 + 4 x2 + 3 x3 <= 15, u = (4, 3, 3): the integer optimum is 19
    bounds = ["--upper", "1=4", "--upper", "2=3", "--upper", "3=3"]
    r = subprocess.run([CLI] + bounds + ["--bnb-bounded", "--long-step", "--cutoff", EXAMPLE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "z* = 19\n" in r.stdout and "nodes: " in r.stdout and "dual events: " in r.stdout
    r = subprocess.run([CLI] + bounds + ["--long-step", EXAMPLE], capture_output=True, text=True)
    assert r.returncode == 64 and "need --bnb-bounded" in r.stderr
