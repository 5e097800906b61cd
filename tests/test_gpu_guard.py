"""GPU tests of the stall guard (csrc/lpx_bounded_guard.hip: lpx_bounded_guard_onchip; lpx_bounded_node4, lpx_node_batch_run2,
lpx_solve_bnb_bounded7), everything bit for bit against the NumPy restatement of the contract (tests/_bounded_guard_ref.py):
record, guard record, trace, tableau, basis, flip, ub, lo and counts.  Without the guard the new entries are the existing ones
on twin handles; the node on which the plain search of binary_model(40, 16, 6) cycles ends; the threshold edges (Bland mode
that starts, ends on progress and starts again, under the long step and the cutoff, with kind-1 rows, ending infeasible); the
stride edges of the two new selections on a wide and on a tall tile; the batch; the driver."""
import functools

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bounded_guard_ref as G
import _bounded_long_ref as L
from _node_helpers import (Pool as _Pool, covering_with_fixed as _covering_with_fixed, fresh as _fresh, node as _node, reads as _reads,
                           same_record as _same_record, same_state as _same_state, u64 as _u64, bits as _bits)

pytestmark = pytest.mark.gpu

INF = np.inf
SKIP, LONG, CUT = L.SKIP_FIXED, L.LONG_STEP, L.CUTOFF_FLAG
NS = G.SMALL[0]


def _same_guard(got, want):
    _same_record(got, want)
    assert (got["bland_events"], got["first_bland"]) == (want["bland_events"], want["first_bland"]), (got, want)


def _handle(T, basis, ub):
    return G.Handle(T, basis, ub, np.zeros(len(ub), dtype=np.uint8))


def _node4(dt, h, nd, nint, S, flags=0, cutoff=None, **kw):
    """One guarded node on the device and in the restatement: everything bit for bit.  Returns (record, modes, picks)."""
    modes, picks = [], []
    want = h.node4(*nd, nint, flags=SKIP | flags | (0 if cutoff is None else CUT), cutoff=-INF if cutoff is None else cutoff,
                   stall_events=S, modes=modes, picks=picks, **kw)
    got = dt.bounded_node(*nd, nint, long_step=bool(flags & LONG), cutoff=cutoff, form="onchip", stall_events=S, **kw)
    _same_guard(got, want)
    assert dt.trace().tolist() == h.trace.tolist()
    _same_state(dt, h, "after the guarded node")
    assert dt.bounded_counts() == (want["kind0"], want["kind1"], want["events"] - want["kind0"] - want["kind1"])
    return want, modes, picks


def _zeroed(T, keep, seed):
    """The objective row mostly zeros: degenerate from the first pivot."""
    T = T.copy()
    z = T[-1, :-1]
    z[np.random.default_rng(1000 + seed).random(len(z)) >= keep] = 0.0
    return T


def _cut_value(T, basis, ub, flags, S, at=0.6):
    """The objective of the guarded run at `at` of its trips: a cutoff that fires inside the run."""
    zs = []
    G.dual_run4(T, basis, ub, None, SKIP | flags, stall_events=S, zs=zs)
    return float(zs[int(at * (len(zs) - 1))])


# ---- 1. without the guard: the existing entries, on twin handles ------------------------------------------------------------
@pytest.mark.parametrize("flags", L.FLAG_SETS)
def test_stall_zero_is_node3_and_run_on_twin_handles(gpu, flags):
    T, basis, ub = G.degenerate_cover(15, 48, 2)
    cut = _cut_value(T, basis, ub, flags & LONG, 0) if flags & CUT else None
    nd = _node()
    with _Pool() as pool:
        a, b, c, d = (pool.add(_fresh(gpu, T, basis, ub)) for _ in range(4))
        for form in ("onchip", "auto", "launches"):
            ra = a.bounded_node(*nd, 4, long_step=bool(flags & LONG), cutoff=cut, form=form, stall_events=0)
            rb = b.bounded_node(*nd, 4, long_step=bool(flags & LONG), cutoff=cut, form=form)
            _same_record(ra, rb)
            assert (ra["bland_events"], ra["first_bland"]) == (0, -1) and "bland_events" not in rb
            assert _reads(a, 4) == _reads(b, 4), form
        want = _handle(T, basis, ub).node4(*nd, 4, flags=SKIP | flags, cutoff=-INF if cut is None else cut)
        assert want["events"] > 0 and (want["status"] == L.CUTOFF) == bool(flags & CUT)
        with gpu.NodeBatch([c]) as nc, gpu.NodeBatch([d]) as nd_:
            rc = nc.run([0], [nd], 4, long_step=bool(flags & LONG), cutoffs=None if cut is None else [cut], stall_events=0)[0]
            rd = nd_.run([0], [nd], 4, long_step=bool(flags & LONG), cutoffs=None if cut is None else [cut])[0]
        _same_record(rc, rd); _same_record(rc, want)
        assert (rc["bland_events"], rc["first_bland"]) == (0, -1)
        assert _reads(c, 4) == _reads(d, 4)


# ---- 2. the cycling node -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cycling(gpu):
    """A device handle in front of the node on which the plain search of binary_model(40, 16, 6) cycles: the root, then diver
    0's nodes 0..2848 replayed with the existing on-chip node.  Tests work on clones of it."""
    out, nodes, before = G.cycling_case()
    T0, basis0, ub0, *_ = N.prepare(*N.binary_model(*G.SMALL), None, np.ones(NS))
    dt = _fresh(gpu, T0, basis0, ub0)
    status, _ = dt.bounded_run()
    assert status == L.OPTIMAL and np.array_equal(_u64(dt.download()[0]), _u64(out["root"][0]))
    log = out["log"]
    for i, nd in enumerate(nodes[:-1]):
        rec = dt.bounded_node(*nd, NS, form="onchip")
        assert rec["status"] == log["status"][i] and rec["events"] == log["events"][i], i
    _same_state(dt, before, "in front of the cycling node")
    yield dt, nodes[-1], before
    dt.close()


@pytest.mark.parametrize("S", [8, 50])
def test_the_cycling_node_ends(gpu, cycling, S):
    dt, nd, before = cycling
    with dt.clone() as c:
        want, modes, _ = _node4(c, before.clone(), nd, NS, S)
        assert want["status"] in (L.OPTIMAL, L.INFEASIBLE) and want["events"] < 1000
        assert want["bland_events"] >= 1 and want["first_bland"] >= S


def test_a_guard_that_never_fires_is_the_unguarded_node(gpu, cycling):
    dt, nd, before = cycling
    with dt.clone() as c, dt.clone() as twin:
        want, modes, _ = _node4(c, before.clone(), nd, NS, 10000, max_iter=400)
        assert want["status"] == L.ITER_LIMIT and want["events"] == 400 and want["bland_events"] == 0 and not any(modes)
        ref = twin.bounded_node(*nd, NS, form="onchip", max_iter=400)
        _same_record(ref, want)
        assert _reads(c, NS) == _reads(twin, NS)


# ---- 3. threshold edges --------------------------------------------------------------------------------------------------------
def _passes_inside_bland(trace, modes):
    """Passes of the long step that belong to a trip in Bland mode: the passes in front of a pivot are its trip's."""
    n, trip, inside = 0, 0, 0
    for r, _ in trace.tolist():
        if r == -1:
            n += 1
        else:
            inside += n if modes[trip] else 0
            n, trip = 0, trip + 1
    return inside


@pytest.mark.parametrize("flags", [0, LONG])
@pytest.mark.parametrize("S", [1, 2])
def test_bland_mode_starts_ends_on_progress_and_starts_again(gpu, S, flags):
    T, basis, ub = G.degenerate_cover(15, 48, 2)
    h = _handle(T, basis, ub)
    with _fresh(gpu, T, basis, ub) as dt:
        want, modes, picks = _node4(dt, h, _node(), 4, S, flags)
    assert want["status"] == L.OPTIMAL and G.bland_runs(modes) >= 2 and want["first_bland"] >= S
    pivots = h.trace[h.trace[:, 0] != -1]
    assert any(r <= -2 and modes[i] for i, (r, _) in enumerate(pivots.tolist())), "no kind-1 row left in Bland mode"
    if flags:                                                # passes before Bland mode, none inside it
        assert (h.trace[:want["first_bland"], 0] == -1).sum() >= 1 and _passes_inside_bland(h.trace, modes) == 0


@pytest.mark.parametrize("S", [1, 2])
def test_kind_one_rows_in_bland_mode_on_a_covering_instance(gpu, S):
    T, basis, ub = _covering_with_fixed(31, 32, 1)
    T = _zeroed(T, 0.1, 1)
    h = _handle(T, basis, ub)
    with _fresh(gpu, T, basis, ub) as dt:
        want, modes, picks = _node4(dt, h, _node(), 4, S)
    pivots = h.trace.tolist()
    assert want["bland_events"] >= 3 and sum(1 for i, (r, _) in enumerate(pivots) if r <= -2 and modes[i]) >= 2


@pytest.mark.parametrize("flags", [0, LONG])
def test_the_cutoff_fires_in_bland_mode(gpu, flags):
    T, basis, ub = G.degenerate_cover(15, 48, 2)
    cut = _cut_value(T, basis, ub, flags, 1)
    with _fresh(gpu, T, basis, ub) as dt:
        want, modes, _ = _node4(dt, _handle(T, basis, ub), _node(), 4, 1, flags, cutoff=cut)
    assert want["status"] == L.CUTOFF and want["bland_events"] >= 1 and want["events"] >= 3


def test_a_node_that_ends_infeasible_in_bland_mode(gpu):
    found = 0
    for seed, S in ((1, 1), (1, 2), (4, 1)):
        T, basis, ub = G.degenerate_cover(15, 48, seed, fixed=0.6)
        with _fresh(gpu, T, basis, ub) as dt:
            want, modes, _ = _node4(dt, _handle(T, basis, ub), _node(), 4, S)
        found += want["status"] == L.INFEASIBLE and modes[-1] and want["bland_events"] >= 1
    assert found >= 1, "no case ended INFEASIBLE in Bland mode"


# ---- 4. stride edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2])
def test_entering_column_across_the_strides_of_a_wide_tile(gpu, S):
    """Cm = 2000: a lane looks at columns t and t + 1024.  Two cases must both occur: the lowest column within ratio_tol lies
    in the second stride (every column of the band does), and it lies in the first stride while the first index of the least
    ratio lies in the second (the band is wider than the minimum)."""
    T, basis, ub = G.wide_cover(5)
    assert T.shape == (7, 2001) and gpu._lib.lib().lpx_bounded_node_fits(*T.shape) == 1
    with _fresh(gpu, T, basis, ub) as dt:
        want, modes, picks = _node4(dt, _handle(T, basis, ub), _node(), 4, S, max_iter=200)
    assert want["events"] == 200 and want["bland_events"] >= 100
    assert any(q >= 1024 for _, _, q, _, _ in picks) and any(q < 1024 <= jmin for _, _, q, _, jmin in picks)


@pytest.mark.parametrize("flags", [0, LONG])
@pytest.mark.parametrize("S", [1, 2])
def test_leaving_row_across_the_strides_of_a_tall_tile(gpu, S, flags):
    """m = 1099: a lane looks at rows t and t + 1024.  The least basic index lies in a row of the second stride while rows of
    the first are infeasible too."""
    T, basis, ub = G.tall_cover(1)
    assert T.shape == (1100, 14) and gpu._lib.lib().lpx_bounded_node_fits(*T.shape) == 1
    with _fresh(gpu, T, basis, ub) as dt:
        want, modes, picks = _node4(dt, _handle(T, basis, ub), _node(), 0, S, flags)
    assert want["bland_events"] >= 5 and any(r >= 1024 and lowest < 1024 for _, r, _, lowest, _ in picks)


# ---- 5. the batch ------------------------------------------------------------------------------------------------------------------
def test_batch_entries_do_not_depend_on_the_batch_or_the_slot(gpu, cycling):
    dt, nd, before = cycling
    S = 8
    Ta, ba, ua = G.degenerate_cover(15, 48, 2)
    Tb, bb, ub_ = _covering_with_fixed(31, 32, 1)
    Tb = _zeroed(Tb, 0.1, 1)
    with _Pool() as pool:
        hs = [pool.add(dt.clone()), pool.add(_fresh(gpu, Ta, ba, ua)), pool.add(_fresh(gpu, Tb, bb, ub_))]
        twins = [pool.add(dt.clone()), pool.add(_fresh(gpu, Ta, ba, ua)), pool.add(_fresh(gpu, Tb, bb, ub_))]
        solo = [pool.add(dt.clone()), pool.add(_fresh(gpu, Ta, ba, ua)), pool.add(_fresh(gpu, Tb, bb, ub_))]
        refs = [before.clone(), _handle(Ta, ba, ua), _handle(Tb, bb, ub_)]
        nodes = [nd, _node(), _node()]
        order = [2, 0, 1]                                    # entry i runs on handles[order[i]]
        with gpu.NodeBatch(hs) as nb:
            got = nb.run(order, [nodes[s] for s in order], 4, stall_events=S)
        for i, s in enumerate(order):
            want = refs[s].node4(*nodes[s], 4, stall_events=S)
            one = twins[s].bounded_node(*nodes[s], 4, form="onchip", stall_events=S)
            with gpu.NodeBatch([solo[s]]) as nb1:
                alone = nb1.run([0], [nodes[s]], 4, stall_events=S)[0]
            _same_guard(got[i], want); _same_guard(one, want); _same_guard(alone, want)
            _same_state(hs[s], refs[s], "entry %d" % i)
            assert hs[s].trace().tolist() == refs[s].trace.tolist()
            assert _reads(hs[s], 4) == _reads(twins[s], 4) == _reads(solo[s], 4)
        assert got[order.index(0)]["bland_events"] >= 1


# ---- 6. the driver -----------------------------------------------------------------------------------------------------------------
def _solve(gpu, **kw):
    c, A0, b0 = N.binary_model(*G.SMALL)
    p = gpu.LPProblem.from_arrays(0, c, A0, np.zeros(G.SMALL[1], dtype=np.int32), b0)
    try:
        return gpu.LPSolver().SolveBnbBounded(p, np.ones(NS), **kw), 0
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
              "guarded_nodes", "bland_events", "max_events"):
        assert res.BnbInfo[k] == want[k], k
    assert res.Status == want["status"]
    if want["status"] == L.OPTIMAL:
        assert np.array_equal(_u64(res.Solution), _u64(want["x"])) and _bits(res.OptimalValue) == _bits(want["value"])


@pytest.mark.parametrize("W", [1, 4, 16])
def test_the_guarded_driver_bit_for_bit(gpu, W):
    want = G.small_search(50, W)
    res, rc = _solve(gpu, divers=W, stall_events=50)
    _same_solve(res, rc, want)
    assert rc == 0 and abs(res.OptimalValue - 268.0) <= 1e-9 * 268.0
    if W == 1:
        assert (res.Nodes, res.BnbInfo["guarded_nodes"], res.BnbInfo["bland_events"]) == (3575, 2, 10)
        plain, prc = _solve(gpu, divers=1)                   # the search this one repairs
        assert prc == gpu._lib.ITER_LIMIT and plain.Nodes == 2850 and abs(plain.OptimalValue - 260.0) <= 1e-9 * 260.0


def test_no_guard_and_stall_zero_are_the_search_by_divers(gpu):
    base, brc = _solve(gpu, divers=4)
    none, nrc = _solve(gpu, divers=4, stall_events=None)
    zero, zrc = _solve(gpu, divers=4, stall_events=0)
    _same_solve(zero, zrc, G.small_search(0, 4))
    for r, code in ((none, nrc), (zero, zrc)):
        assert code == brc and r.BnbLog.tobytes() == base.BnbLog.tobytes()
        assert r.BnbRound.tolist() == base.BnbRound.tolist() and r.BnbDiver.tolist() == base.BnbDiver.tolist()
        assert {k: r.BnbInfo[k] for k in base.BnbInfo} == base.BnbInfo
        assert np.array_equal(_u64(r.Solution), _u64(base.Solution)) and _bits(r.OptimalValue) == _bits(base.OptimalValue)
    assert none.BnbInfo == base.BnbInfo and zero.BnbInfo["guarded_nodes"] == 0
