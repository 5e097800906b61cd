"""GPU tests of reduced-cost bound tightening (csrc/lpx_bounded_fix.hip: lpx_bounded_fix_onchip with csrc/lpx_onchip_fix.h;
lpx_bounded_node5, lpx_node_batch_run3, lpx_solve_bnb_bounded10), everything bit for bit against the NumPy restatement of the
contract (tests/_bnb_tighten_ref.py): record, guard record, the list of triples, trace, tableau, basis, flip, ub, lo and counts,
and against the twin handle of the defining property (the node without tightening, then one more node call with the reported
triples: no event, no flip, equal state).  The edges: fix_bound = -inf and fix_bound >= z, nodes that end INFEASIBLE or CUTOFF, a
masked-out column, flipped columns with a lower shift and ranges of one or more on the general-integer models (whole searches
replayed node by node), nint = 63, 64 and 65 across a wave edge of the ballot compaction, the stall guard beside a bound; the
batch; the driver."""
import ctypes as C

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bnb_tighten_ref as R
import _bounded_dual_ref as D
import _bounded_long_ref as L
import _bounded_ref as B
from _node_helpers import (Pool as _Pool, fresh as _fresh, node as _node, reads as _reads, same_record as _same_record,
                           same_state as _same_state, state as _state, u64 as _u64, bits as _bits)

pytestmark = pytest.mark.gpu

INF = np.inf
SKIP, LONG, CUT = L.SKIP_FIXED, L.LONG_STEP, L.CUTOFF_FLAG


def _same_fixed(got, want):
    assert got[0].tolist() == want[0].tolist(), (got, want)
    assert np.array_equal(_u64(got[1]), _u64(want[1])) and np.array_equal(_u64(got[2]), _u64(want[2])), (got, want)


def _node5(dt, h, nd, nint, fb, S=0, flags=0, cutoff=None, is_int=None, **kw):
    """One node with tightening on the device and in the restatement: everything bit for bit.  Returns the restatement's record."""
    want = h.node5(*nd, nint, is_int=is_int, flags=SKIP | flags | (0 if cutoff is None else CUT), cutoff=-INF if cutoff is None else cutoff,
                   stall_events=S, fix_bound=fb, **kw)
    got = dt.bounded_node(*nd, nint, is_int=is_int, long_step=bool(flags & LONG), cutoff=cutoff, form="onchip", stall_events=S,
                          fix_bound=fb, **kw)
    _same_record(got, want)
    assert (got["bland_events"], got["first_bland"]) == (want["bland_events"], want["first_bland"]), (got, want)
    _same_fixed(got["fixed"], want["fixed"])
    assert dt.trace().tolist() == h.trace.tolist()
    _same_state(dt, h, "after the node with tightening")
    assert dt.bounded_counts() == (want["kind0"], want["kind1"], want["events"] - want["kind0"] - want["kind1"])
    return want


def _twin(twin, dt, nd, nint, fixed, S=0, flags=0, cutoff=None, is_int=None):
    """The defining property on the device: the node without tightening, then one more node call with the reported triples."""
    kw = dict(is_int=is_int, long_step=bool(flags & LONG), cutoff=cutoff, form="onchip", stall_events=S)
    twin.bounded_node(*nd, nint, **kw)
    second = twin.bounded_node(*fixed, nint, **kw)
    assert (second["status"], second["events"], second["flips"]) == (L.OPTIMAL, 0, 0), second
    assert _state(twin) == _state(dt), "the twin that took the triples as an edit differs"


def _root(gpu, T0, basis0, ub0):
    """A device handle and the restatement's handle at the solved root."""
    st, Ts, bs, flip, _, _ = B.run(T0, basis0, ub0)
    assert st == L.OPTIMAL
    dt = _fresh(gpu, T0, basis0, ub0)
    status, _ = dt.bounded_run()
    h = R.Handle(Ts, bs, ub0, flip)
    assert status == L.OPTIMAL
    _same_state(dt, h, "at the root")
    return dt, h


def _ip_root(gpu, n, m):
    c, A, b, up = R.ip_model(n, m)
    T0, basis0, ub0, *_ = N.prepare(c, A, b, None, up)
    return _root(gpu, T0, basis0, ub0)


def _child(h, n):
    """The ceil child of the root's pick, its objective, and the reduced costs of its nonbasic integer columns (restatement)."""
    rec = h.clone().node4(*_node(), n)
    assert rec["var"] >= 0
    nd = _node([rec["var"]], [np.ceil(rec["x_var"])], [h.ub[rec["var"]]])
    g = h.clone()
    kid = g.node4(*nd, n)
    assert kid["status"] == L.OPTIMAL
    d = g.T[-1, :n].copy()
    d[np.isin(np.arange(n), g.basis)] = 0.0
    return nd, kid["z"], d


# ---- 1. a single node -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(16, 4), (60, 12)])
def test_a_child_whose_bound_lies_just_under_its_objective(gpu, n, m):
    dt, h = _ip_root(gpu, n, m)
    assert dt.download()[0].shape == (m + 1, n + m + 1)
    nd, z, d = _child(h, n)
    gap = float(np.median(d[d > 1e-9]))                     # about half of the columns with a reduced cost have less than one step
    with _Pool() as pool:
        pool.add(dt)
        twin = pool.add(dt.clone())
        want = _node5(dt, h, nd, n, z - gap)
        fc, fl, fu = want["fixed"]
        print("tightened", len(fc), "of", n, "columns; flipped among them", int(h.flip[fc].sum()))
        assert len(fc) >= 2 and (h.ub[fc] == 0.0).all()
        _twin(twin, dt, nd, n, want["fixed"])


# ---- 2. the edges ---------------------------------------------------------------------------------------------------------------
def test_minus_infinity_is_node4_on_a_twin(gpu):
    dt, h = _ip_root(gpu, 16, 4)
    nd, z, d = _child(h, 16)
    with _Pool() as pool:
        pool.add(dt)
        twin = pool.add(dt.clone())
        for S in (0, 50):
            a = dt.bounded_node(*nd, 16, form="onchip", stall_events=S, fix_bound=-INF)
            b = twin.bounded_node(*nd, 16, form="onchip", stall_events=S)
            _same_record(a, b)
            assert (a["bland_events"], a["first_bland"]) == (b["bland_events"], b["first_bland"]) and len(a["fixed"][0]) == 0
            assert _reads(dt, 16) == _reads(twin, 16)
        a = dt.bounded_node(*_node(), 16, form="launches", fix_bound=-INF)       # every form
        b = twin.bounded_node(*_node(), 16, form="launches")
        _same_record(a, b)
        assert _reads(dt, 16) == _reads(twin, 16)


def test_a_bound_at_or_above_the_objective_tightens_nothing(gpu):
    dt, h = _ip_root(gpu, 16, 4)
    nd, z, d = _child(h, 16)
    with _Pool() as pool:
        pool.add(dt)
        twin = pool.add(dt.clone())
        b = twin.bounded_node(*nd, 16, form="onchip", stall_events=0)
        want = _node5(dt, h, nd, 16, z)
        assert len(want["fixed"][0]) == 0 and _reads(dt, 16) == _reads(twin, 16)
        for fb in (z + 1.0, INF):                              # again on the same handles: K = 0 nodes
            twin.bounded_node(*_node(), 16, form="onchip", stall_events=0)
            want = _node5(dt, h, _node(), 16, fb)
            assert len(want["fixed"][0]) == 0 and _reads(dt, 16) == _reads(twin, 16)


@pytest.mark.parametrize("end", ["infeasible", "cutoff"])
def test_a_node_that_does_not_end_optimal_tightens_nothing(gpu, end):
    dt, h = _ip_root(gpu, 16, 4)
    nd, z, d = _child(h, 16)
    with _Pool() as pool:
        pool.add(dt)
        twin = pool.add(dt.clone())
        if end == "infeasible":                                # every variable at 1: the rows cannot hold
            nd = _node(np.arange(16), np.ones(16), np.ones(16))
            cutoff = None
        else:
            cutoff = z + 1.0                                   # reached before the first event
        want = _node5(dt, h, nd, 16, -1e6, cutoff=cutoff)
        assert want["status"] == (L.INFEASIBLE if end == "infeasible" else L.CUTOFF) and len(want["fixed"][0]) == 0
        twin.bounded_node(*nd, 16, form="onchip", stall_events=0, cutoff=cutoff)
        assert _reads(dt, 16) == _reads(twin, 16)


def test_a_masked_out_column_with_a_large_reduced_cost_stays(gpu):
    dt, h = _ip_root(gpu, 16, 4)
    nd, z, d = _child(h, 16)
    order = np.argsort(d)
    big, second = int(order[-1]), int(order[-2])
    assert d[big] > d[second] > 1e-9
    gap = 0.5 * (d[big] + d[second])                        # only `big` has less than one step
    mask = np.ones(16, dtype=np.uint8); mask[big] = 0
    with _Pool() as pool:
        pool.add(dt)
        open_ = pool.add(dt.clone())
        masked = _node5(dt, h.clone(), nd, 16, z - gap, is_int=mask)
        assert len(masked["fixed"][0]) == 0
        free = _node5(open_, h.clone(), nd, 16, z - gap)
        assert free["fixed"][0].tolist() == [big]


@pytest.mark.parametrize("name", ["general", "lowers"])
def test_the_search_of_a_general_integer_model_node_by_node(gpu, name):
    """Every node of the restatement's search by one diver, replayed on one device handle: ranges of one or more ("general") and
    flipped columns that get a non-zero lower shift on a handle with lower bounds ("lowers") among them."""
    c, A, rel, b, upper, lower, is_int, sense = N.small_models()[name]
    n = len(c)
    nodes = []
    seen = {"t": 0.0, "flipped_lo": 0}

    def on_node(index, d, h, cols, lo, up, cutoff, fix_bound):
        nodes.append((cols.copy(), lo.copy(), up.copy(), fix_bound))

    def on_done(index, d, h, rec):
        for j, l, u in zip(*rec["fixed"]):
            seen["t"] = max(seen["t"], u - l)
            seen["flipped_lo"] += bool(h.flip[j] and l != 0.0)

    out = R.solve_tighten(c, A, b, upper, 1, lower=lower, is_int=is_int, sense=sense, rel=rel, on_node=on_node, on_done=on_done)
    assert out["rc"] == 0 and out["tightened_nodes"] >= 1 and len(nodes) == out["nodes"] <= 400
    assert seen["t"] >= 1.0 if name == "general" else seen["flipped_lo"] >= 1
    T0, basis0, ub0, *_ = N.prepare(c, A, b, lower, upper, sense, rel)
    dt, h = _root(gpu, T0, basis0, ub0)
    with _Pool() as pool:
        pool.add(dt)
        tightened = 0
        for i, (cols, lo, up, fb) in enumerate(nodes):
            twin = None
            if tightened < 3:                                  # the twin of the first few tightened nodes
                twin = dt.clone()
            want = _node5(dt, h, (cols, lo, up), n, fb)
            assert want["status"] == out["log"]["status"][i] and want["events"] == out["log"]["events"][i], i
            if twin is not None:
                with twin:
                    if len(want["fixed"][0]):
                        _twin(twin, dt, (cols, lo, up), n, want["fixed"])
                        tightened += 1
        assert tightened >= 1


@pytest.mark.parametrize("nint", [63, 64, 65])
def test_the_list_across_a_wave_edge(gpu, nint):
    """nint = 63, 64 and 65 integer columns of a model with four rows: with a bound just under the root's objective nearly every
    nonbasic column is tightened, so the ballot compaction fills a wave, ends on its edge and crosses it."""
    dt, h = _ip_root(gpu, nint, 4)
    z = float(h.T[-1, -1])
    with _Pool() as pool:
        pool.add(dt)
        twin = pool.add(dt.clone())
        want = _node5(dt, h, _node(), nint, z - 1e-6)
        fc = want["fixed"][0]
        print("tightened", len(fc), "of", nint)
        assert len(fc) >= nint - 12 and fc.min() < 8 and fc.max() == nint - 1, fc
        _twin(twin, dt, _node(), nint, want["fixed"])


@pytest.mark.parametrize("S", [8, 50])
def test_the_stall_guard_beside_a_bound_on_the_cycling_node(gpu, S):
    """The node of binary_bounded(64, 32, 1) on which the unflagged loop cycles, as one call with K = 31: the guard record is that
    of lpx_bounded_node4 whatever the bound."""
    T, basis, ub, model, Ts, bs, flip = D.root(64, 32, 1)
    cols = np.array(sorted(N.CYCLING_ONES + N.CYCLING_ZEROS), dtype=np.int32)
    vals = np.array([1.0 if j in N.CYCLING_ONES else 0.0 for j in cols])
    nd = (cols, vals, vals)
    dt, h = _root(gpu, T, basis, ub)
    with _Pool() as pool:
        pool.add(dt)
        twin = pool.add(dt.clone())
        plain = h.clone().node4(*nd, 64, stall_events=S)
        want = _node5(dt, h, nd, 64, plain["z"] - 2.0, S=S)
        assert (want["bland_events"], want["first_bland"], want["events"]) == (plain["bland_events"], plain["first_bland"], plain["events"])
        g4 = twin.bounded_node(*nd, 64, form="onchip", stall_events=S)
        assert (g4["bland_events"], g4["first_bland"], g4["events"]) == (want["bland_events"], want["first_bland"], want["events"])
        assert want["status"] == L.OPTIMAL and len(want["fixed"][0]) >= 1


# ---- 3. the batch ---------------------------------------------------------------------------------------------------------------
def test_batch_entries_equal_their_single_node_calls(gpu):
    dt, h = _ip_root(gpu, 16, 4)
    nd, z, d = _child(h, 16)
    rec = h.clone().node4(*_node(), 16)
    floor = _node([rec["var"]], [0.0], [np.floor(rec["x_var"])])
    zf = h.clone().node4(*floor, 16)["z"]
    gap = float(np.median(d[d > 1e-9]))
    nodes = [nd, floor, nd]
    fbs = [z - gap, -INF, z - 0.25 * gap]
    with _Pool() as pool:
        hs = [pool.add(dt), pool.add(dt.clone()), pool.add(dt.clone())]
        solo = [pool.add(dt.clone()) for _ in range(3)]
        refs = [h.clone() for _ in range(3)]
        order = [2, 0, 1]                                    # entry i runs on handles[order[i]]
        with gpu.NodeBatch(hs) as nb:
            got = nb.run(order, [nodes[s] for s in order], 16, fix_bounds=[fbs[s] for s in order])
        for i, s in enumerate(order):
            want = refs[s].node5(*nodes[s], 16, fix_bound=fbs[s])
            one = solo[s].bounded_node(*nodes[s], 16, form="onchip", fix_bound=fbs[s])
            for r in (got[i], one):
                _same_record(r, want)
                assert (r["bland_events"], r["first_bland"]) == (0, -1)
                _same_fixed(r["fixed"], want["fixed"])
            _same_state(hs[s], refs[s], "entry %d" % i)
            assert hs[s].trace().tolist() == refs[s].trace.tolist()
            assert _reads(hs[s], 16) == _reads(solo[s], 16)
        assert len(got[order.index(0)]["fixed"][0]) >= 2 and len(got[order.index(1)]["fixed"][0]) == 0
        assert len(got[order.index(2)]["fixed"][0]) >= 1
        # all -inf: the launch of lpx_node_batch_run2
        with gpu.NodeBatch(hs) as nb:
            off = nb.run([0, 1], [_node(), _node()], 16, fix_bounds=-INF)
        a = solo[0].bounded_node(*_node(), 16, form="onchip", stall_events=0)
        _same_record(off[0], a)
        assert len(off[0]["fixed"][0]) == 0 and _reads(hs[0], 16) == _reads(solo[0], 16)


# ---- 4. the driver --------------------------------------------------------------------------------------------------------------
def _solve(gpu, n, m, **kw):
    c, A, b, up = R.ip_model(n, m)
    p = gpu.LPProblem.from_arrays(0, c, A, np.zeros(m, dtype=np.int32), b)
    try:
        return gpu.LPSolver().SolveBnbBounded(p, up, **kw), 0
    except gpu.SolverException as e:
        return e.result, e.code


def _same_solve(res, rc, want):
    log = res.BnbLog
    assert rc == want["rc"] and len(log) == len(want["log"]) == res.Nodes == want["nodes"]
    for k in ("depth", "K", "status", "events", "flips", "var"):
        assert np.array_equal(log[k], want["log"][k]), k
    assert np.array_equal(_u64(log["z"]), _u64(want["log"]["z"])), "z bits of some node differ"
    assert res.BnbRound.tolist() == want["round"].tolist() and res.BnbDiver.tolist() == want["diver"].tolist()
    for k in ("nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K", "rounds", "steals", "largest_batch",
              "guarded_nodes", "bland_events", "max_events", "tightened_nodes", "tightened_cols", "max_per_node"):
        assert res.BnbInfo[k] == want[k], k
    assert res.Status == want["status"] == L.OPTIMAL
    assert np.array_equal(_u64(res.Solution), _u64(want["x"])) and _bits(res.OptimalValue) == _bits(want["value"])


@pytest.mark.parametrize("flags", [0, LONG | CUT])
@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("n,m", [(24, 6), (32, 8)])
def test_the_tightening_driver_bit_for_bit(gpu, n, m, W, flags):
    want = R.ip_search(n, m, W, flags)
    res, rc = _solve(gpu, n, m, divers=W, tighten=True, long_step=bool(flags & LONG), cutoff=bool(flags & CUT))
    _same_solve(res, rc, want)
    assert res.BnbInfo["tightened_nodes"] >= 1
    if W == 1 and flags == 0:
        base, brc = _solve(gpu, n, m, divers=1)
        assert brc == 0 and res.Nodes < base.Nodes and abs(res.OptimalValue - base.OptimalValue) <= 1e-9 * abs(base.OptimalValue)


@pytest.mark.parametrize("W", [1, 4])
def test_tighten_zero_is_the_driver_without_it_byte_for_byte(gpu, W):
    lib = gpu._lib.lib()
    c, A, b, up = R.ip_model(24, 6)
    p = gpu.LPProblem.from_arrays(0, c, A, np.zeros(6, dtype=np.int32), b)
    from linear_programming_solver_lpr381_amd.solver import _problem_struct
    ps, hold = _problem_struct(p)
    upp = np.ascontiguousarray(up).ctypes.data_as(gpu._lib.dp)
    logs = []
    for entry in (9, 10):
        r, info, dinfo, ginfo = gpu._lib.Result(), gpu._lib.BnbBoundedInfo(), gpu._lib.BnbDiversInfo(), gpu._lib.BnbGuardInfo()
        cinfo, finfo = gpu._lib.BnbCutInfo(), gpu._lib.BnbFixInfo(9, 9, 9)
        if entry == 9:
            rc = lib.lpx_solve_bnb_bounded9(C.byref(ps), None, upp, None, None, 0, LONG | CUT, W, 0, 0, None, C.byref(r), C.byref(info),
                                            C.byref(dinfo), C.byref(ginfo), C.byref(cinfo))
        else:
            rc = lib.lpx_solve_bnb_bounded10(C.byref(ps), None, upp, None, None, 0, LONG | CUT, W, 0, 0, None, 0, C.byref(r),
                                             C.byref(info), C.byref(dinfo), C.byref(ginfo), C.byref(cinfo), C.byref(finfo))
            assert (finfo.tightened_nodes, finfo.tightened_cols, finfo.max_per_node) == (0, 0, 0)
        assert rc == 0 and info.n_log >= 1
        logs.append((C.string_at(info.log, info.n_log * C.sizeof(gpu._lib.BnbNodeLog)), int(info.nodes), int(info.events), int(dinfo.rounds),
                     int(dinfo.steals), _bits(r.value) if hasattr(r, "value") else None))
        lib.lpx_bnb_bounded_info_free(C.byref(info)); lib.lpx_bnb_divers_info_free(C.byref(dinfo)); lib.lpx_bnb_cut_info_free(C.byref(cinfo))
        lib.lpx_result_free(C.byref(r))
    assert logs[0] == logs[1]
    off, orc = _solve(gpu, 24, 6, divers=W, long_step=True, cutoff=True)
    assert orc == 0 and off.BnbLog.tobytes() == logs[1][0]
