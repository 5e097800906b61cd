"""GPU tests of the batch of on-chip nodes and of the search by divers (csrc/lpx_bounded_node.hip: lpx_bounded_nodes_onchip;
lpx_tableau_clone, lpx_node_batch_*, lpx_solve_bnb_bounded4): every entry of a batch bit for bit against the single-node on-chip
form on a twin handle and against the NumPy restatement (tests/_bounded_long_ref.py) -- record, trace, tableau, basis, flip, ub,
lo, counts and solution; every outcome in one launch, refusals between good entries, mixed shapes, more workgroups than compute
units, independence of the slot; the driver's log, with the round and the diver of every record, against tests/_bnb_divers_ref.py."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bnb_divers_ref as V
import _bounded_dual_ref as D
import _bounded_long_ref as L
import _bounded_ref as B
from _node_helpers import (Pool as _Pool, bits as _bits, covering_with_fixed as _covering_with_fixed, fresh as _fresh, node as _node,
                           reads as _reads, ref_node as _ref_node, same_record as _same_record, same_state as _same_handle,
                           slack_handle as _slack_handle, state as _state, u64 as _u64)

pytestmark = pytest.mark.gpu

INF = np.inf
REL = 1e-9
SKIP, LONG, CUT = L.SKIP_FIXED, L.LONG_STEP, L.CUTOFF_FLAG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
EXAMPLE = os.path.join(ROOT, "integration", "Input", "example_bounded.txt")


def _same_state(dt, h, what=""):
    _same_handle(dt, h, what)
    assert dt.trace().tolist() == h.trace.tolist(), what


def _solved(lpx, n, m, seed):
    T, basis, ub, model, Ts, bs, flip = D.root(n, m, seed)
    dt = _fresh(lpx, T, basis, ub)
    status, _ = dt.bounded_run()
    assert status == B.OPTIMAL and np.array_equal(_u64(dt.download()[0]), _u64(Ts))
    return dt, (Ts, bs, ub, flip)


# ---- 1. clone -------------------------------------------------------------------------------------------------------------
def test_clone_of_a_solved_root_with_flips_and_a_lower_shift(gpu):
    n = 40
    with _Pool() as pool:
        src, root = _solved(gpu, n, 20, 1)
        twin, _ = _solved(gpu, n, 20, 1)
        pool.add(src); pool.add(twin)
        h = L.Handle(*root)
        j = N.pick(h.T, h.basis, h.flip, h.ub, h.lo, n)["var"]
        for dt in (src, twin):                               # a node that stores a non-zero lo
            got = dt.bounded_node([j], [1.0], [1.0], n, form="onchip")
        want = _ref_node(h, _node([j], [1.0], [1.0]), n)
        _same_record(got, want)
        assert h.flip[:n].any() and h.lo[j] == 1.0, "no flip or no lower shift: the test shows nothing"
        src.snapshot()
        before = _reads(src, n)
        c = pool.add(src.clone())
        assert (c.R, c.C, c.ld) == (src.R, src.C, src.ld)
        assert _state(c) == _state(src) == before[:5]
        xs, zs, us = src.bounded_solution(n)
        xc, zc, uc = c.bounded_solution(n)
        assert np.array_equal(_u64(xs), _u64(xc)) and _bits(zs) == _bits(zc) and np.array_equal(us, uc)
        assert c.trace().tolist() == [] and c.bounded_counts() == (0, 0, 0)
        assert _reads(src, n) == before, "the clone changed its source"
        # a node on the clone is the node on the source's twin, in both forms, and the branch pick reads the copied RHS
        assert c.branch_pick(n) == twin.branch_pick(n)
        k = [i for i in range(n) if h.ub[i] > 0.0 and i != j][0]
        for form in ("onchip", "launches"):
            a = c.bounded_node([k], [0.0], [0.0], n, form=form)
            b = twin.bounded_node([k], [0.0], [0.0], n, form=form)
            _same_record(a, b)
            assert _reads(c, n) == _reads(twin, n)
            k = [i for i in range(n) if h.ub[i] > 0.0 and i not in (j, k)][0]
        assert _reads(src, n) == before, "a node on the clone changed the source"
        # a clone of a handle without bounds, and the bounded loop on the clone of an unsolved handle
        T, basis, ub, _ = B.binary_bounded(12, 6, 1)
        with gpu.DeviceTableau.from_host(T, basis) as plain, plain.clone() as pc:
            assert np.array_equal(_u64(pc.download()[0]), _u64(T)) and pc.download()[1].tolist() == basis.tolist()
            plain.set_bounds(ub)
            with plain.clone() as bc:
                sa, sb = plain.bounded_run()[0], bc.bounded_run()[0]
                assert sa == sb == B.OPTIMAL and _state(plain) == _state(bc) and plain.trace().tolist() == bc.trace().tolist()


def test_a_refused_first_node_leaves_a_clone_as_it_was(gpu):
    """The clone's trace reads empty until a node RUNS on it: a node the kernel refuses, in either entry point, changes nothing."""
    n = 40
    with _Pool() as pool:
        src, root = _solved(gpu, n, 20, 1); pool.add(src)
        twin, _ = _solved(gpu, n, 20, 1); pool.add(twin)
        assert len(src.trace()) > 0
        flipped = int(np.flatnonzero(root[3][:n])[0])
        c = pool.add(src.clone())
        before = _reads(c, n)
        assert before[5] == []
        with pytest.raises(gpu.LpxError) as e:
            c.bounded_node([flipped], [0.0], [INF], n, form="onchip")
        assert "+inf on a flipped column" in str(e.value) and _reads(c, n) == before
        with gpu.NodeBatch([c]) as nb:
            got = nb.run([0], [_node([flipped], [0.0], [INF])], n)
            assert got[0]["status"] is None and _reads(c, n) == before
            got = nb.run([0], [_node([flipped], [0.0], [0.0])], n)
        _same_record(got[0], twin.bounded_node([flipped], [0.0], [0.0], n, form="onchip"))
        assert _reads(c, n) == _reads(twin, n)


# ---- 2. B = 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, LONG])
def test_batch_of_one_is_the_single_node_form(gpu, flags):
    n = 40
    with _Pool() as pool:
        dt, root = _solved(gpu, n, 20, 1)
        twin, _ = _solved(gpu, n, 20, 1)
        pool.add(dt); pool.add(twin)
        h = L.Handle(*root)
        with gpu.NodeBatch([dt]) as nb:
            for step in range(4):                            # a dive: K = 0, then the pick fixed at 0, 1, 0
                p = N.pick(h.T, h.basis, h.flip, h.ub, h.lo, n)
                node = _node() if step == 0 else _node([p["var"]], [float(step % 2)], [float(step % 2)])
                want = _ref_node(h, node, n, flags)
                got = nb.run([0], [node], n, long_step=bool(flags))
                ref = twin.bounded_node(*node, n, long_step=bool(flags), form="onchip")
                assert len(got) == 1
                _same_record(got[0], want); _same_record(got[0], ref)
                _same_state(dt, h, "step %d" % step)
                assert _reads(dt, n) == _reads(twin, n)
                assert dt.bounded_counts() == (want["kind0"], want["kind1"], want["events"] - want["kind0"] - want["kind1"])
                if want["status"] != L.OPTIMAL or p["var"] < 0:
                    break
            assert step >= 2
            # a following node of either form on the handle the batch left
            for form in ("launches", "onchip"):
                k = [i for i in range(n) if h.ub[i] > 0.0][0]
                _same_record(dt.bounded_node([k], [0.0], [0.0], n, form=form), twin.bounded_node([k], [0.0], [0.0], n, form=form))
                assert _reads(dt, n) == _reads(twin, n)
                h.node2(*_node([k], [0.0], [0.0]), n, flags=SKIP)


# ---- 3. one launch, many outcomes -----------------------------------------------------------------------------------------
def _outcome_entries(gpu, pool):
    """(handle, twin, restatement handle, node, nint) per entry; the shared event limit is 25."""
    out = []

    def solved(n, m, seed, node):
        dt, root = _solved(gpu, n, m, seed)
        twin, _ = _solved(gpu, n, m, seed)
        out.append((pool.add(dt), pool.add(twin), L.Handle(*root), node, n))

    def slack(m, n, node=_node()):
        T, basis, ub = _covering_with_fixed(m, n, 1)
        out.append((pool.add(_fresh(gpu, T, basis, ub)), pool.add(_fresh(gpu, T, basis, ub)), _slack_handle(T, basis, ub), node, n))

    solved(40, 20, 1, _node())                                                       # 0: K = 0
    j, l, u = D.children(40, 20, 1)[0]
    solved(40, 20, 1, _node([j], [l], [u]))                                          # 1: one triple
    cols = np.array(sorted(N.CYCLING_ONES + N.CYCLING_ZEROS), dtype=np.int32)
    vals = np.array([1.0 if c in N.CYCLING_ONES else 0.0 for c in cols])
    solved(64, 32, 1, (cols, vals, vals))                                            # 2: the cycling node, 31 triples
    slack(129, 4)                                                                    # 3: INFEASIBLE in 7 events
    slack(31, 32)                                                                    # 4: needs 29 events: the limit
    slack(31, 32)                                                                    # 5: cut off, with its own cutoff
    slack(15, 48)                                                                    # 6: its neighbour, cutoff -inf
    return out


@pytest.mark.parametrize("flags", [0, LONG])
def test_one_launch_with_every_outcome(gpu, flags):
    MAX_ITER = 25
    with _Pool() as pool:
        ent = _outcome_entries(gpu, pool)
        T, basis, ub = _covering_with_fixed(31, 32, 1)
        cut = float(L.dual_run3(T, basis, ub, None, SKIP | flags, max_iter=10)[1][-1, -1])      # the objective after 10 events
        cutoffs = [-INF] * len(ent)
        cutoffs[5] = cut
        assert len(ent[2][3][0]) == 31 and len(ent[1][3][0]) == 1 and len(ent[0][3][0]) == 0
        before = [_reads(e[0], e[4]) for e in ent]
        order = [3, 0, 6, 5, 2, 1, 4]                                                # entry i runs on handles[order[i]]
        with gpu.NodeBatch([e[0] for e in ent]) as nb:
            got = nb.run(order, [ent[s][3] for s in order], 4, long_step=bool(flags), cutoffs=[cutoffs[s] for s in order], max_iter=MAX_ITER)
        statuses = {}
        for i, s in enumerate(order):
            dt, twin, h, node, n = ent[s]
            want = h.node2(*node, 4, flags=SKIP | flags | CUT, cutoff=cutoffs[s], max_iter=MAX_ITER)
            ref = twin.bounded_node(*node, 4, long_step=bool(flags), cutoff=cutoffs[s], form="onchip", max_iter=MAX_ITER)
            _same_record(got[i], ref); _same_record(got[i], want)
            _same_state(dt, h, "entry %d" % i)
            assert _reads(dt, n) == _reads(twin, n), "entry %d differs from its twin on the single-node form" % i
            assert _reads(dt, n) != before[s] or want["events"] == 0
            statuses[s] = want["status"]
        assert statuses[0] == statuses[1] == L.OPTIMAL and statuses[3] == L.INFEASIBLE and statuses[4] == L.ITER_LIMIT
        assert statuses[5] == L.CUTOFF and statuses[6] != L.CUTOFF
        if not flags:
            assert statuses[2] == L.OPTIMAL and got[order.index(2)]["events"] == 21


# ---- 4. a refused entry between two good ones -----------------------------------------------------------------------------
def test_a_refused_entry_between_two_good_ones(gpu):
    T, basis, ub, _ = B.binary_bounded(12, 6, 1)
    bad_ub = ub.copy(); bad_ub[2] = INF                                              # T[m,2] = -c_2 < 0 with no upper bound
    n = 40
    with _Pool() as pool:
        good0 = pool.add(_fresh(gpu, T, basis, ub)); twin0 = pool.add(_fresh(gpu, T, basis, ub))
        bad = pool.add(_fresh(gpu, T, basis, bad_ub))
        good2, root = _solved(gpu, n, 20, 1); pool.add(good2)
        twin2, _ = _solved(gpu, n, 20, 1); pool.add(twin2)
        flipped = int(np.flatnonzero(root[3][:n])[0])
        before_bad, before2 = _reads(bad, 12), _reads(good2, n)
        with gpu.NodeBatch([good0, bad, good2]) as nb:
            edit = _node([0, 5], [0.0, 1.0], [0.0, 1.0])
            got = nb.run([0, 1, 2], [edit, edit, _node()], 12)
            msg = gpu._lib.last_error()
            assert got[1]["status"] is None and got[1]["unrepairable"] == 1 and got[1]["var"] == -1
            assert "lpx_node_batch_run: entry 1: 1 column(s) with a negative reduced cost and no upper bound" in msg
            assert _reads(bad, 12) == before_bad, "the refused entry changed its handle"
            _same_record(got[0], twin0.bounded_node(*edit, 12, form="onchip"))
            _same_record(got[2], twin2.bounded_node([], [], [], 12, form="onchip"))
            assert got[0]["status"] is not None and got[2]["status"] == L.OPTIMAL
            assert _reads(good0, 12) == _reads(twin0, 12) and _reads(good2, n) == _reads(twin2, n)
            # +inf on a flipped column: refused per entry too, and it is the lowest refused entry that speaks
            got = nb.run([2, 1], [_node([flipped], [0.0], [INF]), _node()], 12)
            assert got[0]["status"] is None and got[0]["unrepairable"] == 0 and got[1]["status"] is None and got[1]["unrepairable"] == 1
            assert "lpx_node_batch_run: entry 0: upper[0] = +inf on a flipped column" in gpu._lib.last_error()
            assert _reads(bad, 12) == before_bad and _reads(good2, n) == _reads(twin2, n)
            # the refused handle takes a valid node afterwards: column 2 gets a bound
            h = _slack_handle(T, basis, bad_ub)
            got = nb.run([1], [_node([2], [0.0], [1.0])], 12)
            _same_record(got[0], h.node2(*_node([2], [0.0], [1.0]), 12))
            _same_state(bad, h)
            # argument errors name their entry and touch nothing
            now = _reads(good0, 12)
            for slots, nodes, what in (([0, 0], [_node(), _node()], "entry 1: slot repeats a handle"),
                                       ([0, 3], [_node(), _node()], "entry 1: slot is outside [0, W)"),
                                       ([2, 0], [_node(), _node([0, 0], [0.0, 0.0], [1.0, 1.0])], "entry 1: cols[1] repeats a column"),
                                       ([0, 2], [_node([1], [0.0], [1.0]), _node([99], [0.0], [1.0])], "entry 1: cols[0] is outside")):
                with pytest.raises(gpu.LpxError) as e:
                    nb.run(slots, nodes, 12)
                assert e.value.code == gpu._lib.EINVAL and "lpx_node_batch_run: " + what in str(e.value), str(e.value)
            with pytest.raises(gpu.LpxError) as e:
                nb.run([0], [_node()], 99)
            assert "lpx_node_batch_run: entry 0: nint is outside [0, C-1]" in str(e.value)
            assert _reads(good0, 12) == now
        # what a batch cannot borrow
        with gpu.DeviceTableau.from_host(T, basis) as nobounds:
            for hs, what in (([good0, good0], "named twice"), ([good0, nobounds], "handle 1: the handle has no bounds")):
                with pytest.raises(gpu.LpxError) as e:
                    gpu.NodeBatch(hs)
                assert e.value.code == gpu._lib.EINVAL and what in str(e.value)
        Tb, bb, ubb = _covering_with_fixed(256, 512, 1)
        with _fresh(gpu, Tb, bb, ubb) as big:
            with pytest.raises(gpu.LpxError) as e:
                gpu.NodeBatch([good0, big])
            assert e.value.code == gpu._lib.EINVAL and "handle 1" in str(e.value) and "does not fit" in str(e.value)


# ---- 5. mixed shapes in one launch ----------------------------------------------------------------------------------------
MIXED = {(1, 3): (2, 5), (32, 32): (33, 65), (64, 190): (65, 255), (8, 1016): (9, 1025), (129, 4): (130, 134)}


@pytest.mark.parametrize("flags", [0, LONG])
def test_mixed_shapes_in_one_launch(gpu, flags):
    with _Pool() as pool:
        ent = []
        for (m, n), shape in sorted(MIXED.items()):
            T, basis, ub = _covering_with_fixed(m, n, 1)
            assert T.shape == shape and gpu._lib.lib().lpx_bounded_node_fits(*shape) == 1
            ent.append((pool.add(_fresh(gpu, T, basis, ub)), pool.add(_fresh(gpu, T, basis, ub)), n))
        with gpu.NodeBatch([e[0] for e in ent]) as nb:
            got = nb.run(list(range(len(ent))), [_node()] * len(ent), 1, long_step=bool(flags))
        for i, (dt, twin, n) in enumerate(ent):
            ref = twin.bounded_node([], [], [], 1, long_step=bool(flags), form="onchip")
            _same_record(got[i], ref)
            assert ref["events"] > 0 and _reads(dt, n) == _reads(twin, n), "shape %s differs from its twin" % (MIXED[sorted(MIXED)[i]],)


# ---- 6. more workgroups than compute units --------------------------------------------------------------------------------
def test_more_workgroups_than_compute_units(gpu):
    W = 260
    T, basis, ub = _covering_with_fixed(2, 1, 1)
    assert T.shape == (3, 4)
    h = _slack_handle(T, basis, ub)
    first = _ref_node(h, _node(), 1)
    after_first = L.Handle(h.T, h.basis, h.ub, h.flip, h.lo); after_first.trace = h.trace
    edit = _node([0], [0.5], [1.0])                          # a non-zero lower bound: one more pivot
    second = _ref_node(h, edit, 1)
    assert first["status"] == L.OPTIMAL and first["events"] == 1 and second["events"] > 0
    with _Pool() as pool:
        hs = [pool.add(_fresh(gpu, T, basis, ub)) for _ in range(W)]
        with gpu.NodeBatch(hs) as nb:
            got = nb.run(np.arange(W), [_node()] * W, 1)
            for i in range(W):
                _same_record(got[i], first)
            for i in (0, 1, 63, 64, 255, 256, 259):
                _same_state(hs[i], after_first, "handle %d" % i)
            states = {repr(_state(dt)) for dt in hs}
            assert len(states) == 1
            # a permuted subset; the handles not named are untouched
            g = np.random.default_rng(5)
            slots = g.permutation(W)[:97]
            got = nb.run(slots, [edit] * len(slots), 1)
            named = set(slots.tolist())
            for i in range(len(slots)):
                _same_record(got[i], second)
            for s in range(W):
                if s in named:
                    _same_state(hs[s], h, "slot %d" % s)
                else:
                    _same_state(hs[s], after_first, "unnamed slot %d" % s)
                    assert hs[s].bounded_counts() == (first["kind0"], first["kind1"], 0)


# ---- 7. independence of the slot and of the neighbours ------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, LONG])
def test_an_entry_does_not_depend_on_its_slot_or_its_neighbours(gpu, flags):
    n = 40
    j, l, u = D.children(n, 20, 1)[1]
    node = _node([j], [l], [u])
    with _Pool() as pool:
        alone, _ = _solved(gpu, n, 20, 1); pool.add(alone)
        crowd = []
        for k in range(7):
            T, basis, ub = _covering_with_fixed(*((15, 48), (31, 32), (1, 3), (63, 190), (2, 1), (16, 47), (129, 4))[k], 1)
            crowd.append(pool.add(_fresh(gpu, T, basis, ub)))
        last, _ = _solved(gpu, n, 20, 1); pool.add(last)
        with gpu.NodeBatch([alone]) as one, gpu.NodeBatch(crowd + [last]) as eight:
            a = one.run([0], [node], 3, long_step=bool(flags))[0]           # nint is shared: the narrowest handle has 3 columns
            b = eight.run(list(range(8)), [_node()] * 7 + [node], 3, long_step=bool(flags))[7]
        _same_record(a, b)
        assert a["events"] > 0 and _reads(alone, n) == _reads(last, n)


# ---- 8. the driver ----------------------------------------------------------------------------------------------------------
def _problem(lpx, c, A, rel, b, sense=0):
    return lpx.LPProblem.from_arrays(sense, c, A, rel, b)


@functools.lru_cache(maxsize=None)
def _want_divers(n, m, seed, W, flags, max_nodes=0):
    c, A0, b0 = N.binary_model(n, m, seed)
    return V.solve_divers(c, A0, b0, np.ones(n), W, search_flags=flags, max_nodes=max_nodes)


def _same_solve(res, want):
    log = res.BnbLog
    assert len(log) == len(want["log"]) == res.Nodes == want["nodes"]
    for k in ("depth", "K", "status", "events", "flips", "var"):
        assert np.array_equal(log[k], want["log"][k]), k
    assert np.array_equal(_u64(log["z"]), _u64(want["log"]["z"])), "z bits of some node differ"
    assert res.BnbRound.tolist() == want["round"].tolist() and res.BnbDiver.tolist() == want["diver"].tolist()
    for k in ("nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K", "rounds", "steals", "largest_batch"):
        assert res.BnbInfo[k] == want[k], k
    assert res.Status == want["status"]
    if want["status"] == L.OPTIMAL:
        assert np.array_equal(_u64(res.Solution), _u64(want["x"])) and _bits(res.OptimalValue) == _bits(want["value"])


@pytest.mark.parametrize("flags", [0, LONG | CUT])
@pytest.mark.parametrize("W", [1, 2, 8, 64])
@pytest.mark.parametrize("n,m,seed", [(16, 8, 1), (32, 16, 2)])
def test_driver_log_bit_for_bit(gpu, n, m, seed, W, flags):
    c, A0, b0 = N.binary_model(n, m, seed)
    want = _want_divers(n, m, seed, W, flags)
    p = _problem(gpu, c, A0, np.zeros(m, dtype=np.int32), b0)
    kw = dict(long_step=bool(flags & LONG), cutoff=bool(flags & CUT))
    res = gpu.LPSolver().SolveBnbBounded(p, np.ones(n), divers=W, **kw)
    assert want["rc"] == 0 and want["nodes"] > 50
    _same_solve(res, want)
    if W == 1:                                               # one diver is the sequential driver on chip
        ref = gpu.LPSolver().SolveBnbBounded(p, np.ones(n), node_form="onchip", **kw)
        assert res.BnbLog.tobytes() == ref.BnbLog.tobytes()
        assert {k: res.BnbInfo[k] for k in ref.BnbInfo} == ref.BnbInfo
        assert np.array_equal(_u64(res.Solution), _u64(ref.Solution)) and _bits(res.OptimalValue) == _bits(ref.OptimalValue)
        assert res.Summary == ref.Summary
        assert res.BnbInfo["rounds"] == res.Nodes and res.BnbInfo["steals"] == 0 and res.BnbInfo["largest_batch"] == 1


def test_driver_node_limit_cuts_a_round_short(gpu):
    n, m, seed, W = 16, 8, 1, 8
    full = _want_divers(n, m, seed, W, 0)
    limit = int(np.flatnonzero(full["round"] == 5)[1]) + 1                            # inside round 5
    want = _want_divers(n, m, seed, W, 0, limit)
    assert want["rc"] == L.ITER_LIMIT and want["nodes"] == limit and want["round"][-1] == 5
    c, A0, b0 = N.binary_model(n, m, seed)
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver().SolveBnbBounded(_problem(gpu, c, A0, np.zeros(m, dtype=np.int32), b0), np.ones(n), max_nodes=limit, divers=W)
    assert e.value.code == gpu._lib.ITER_LIMIT and "node limit of %d reached" % limit in str(e.value)
    _same_solve(e.value.result, want)


def test_driver_iteration_limit_ends_the_solve_at_that_record(gpu):
    n, m, seed, W = 40, 20, 1, 8                             # the root takes 31 events, node 351 would take more than 32
    c, A0, b0 = N.binary_model(n, m, seed)
    want = V.solve_divers(c, A0, b0, np.ones(n), W, max_iter=32)
    assert want["rc"] == L.ITER_LIMIT and want["log"]["status"][-1] == L.ITER_LIMIT and want["nodes"] == 352
    assert want["diver"][-1] == 0 and int((want["round"] == want["round"][-1]).sum()) == 1      # the round's later records are dropped
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver(max_iter=32).SolveBnbBounded(_problem(gpu, c, A0, np.zeros(m, dtype=np.int32), b0), np.ones(n), divers=W)
    assert e.value.code == gpu._lib.ITER_LIMIT and "node 351 (depth" in str(e.value) and "iteration limit of 32 events" in str(e.value)
    _same_solve(e.value.result, want)


def test_two_solves_in_a_row_give_identical_logs(gpu):
    c, A0, b0 = N.binary_model(32, 16, 2)
    p = _problem(gpu, c, A0, np.zeros(16, dtype=np.int32), b0)
    a = gpu.LPSolver().SolveBnbBounded(p, 1.0, divers=16, long_step=True, cutoff=True)
    b = gpu.LPSolver().SolveBnbBounded(p, 1.0, divers=16, long_step=True, cutoff=True)
    assert a.BnbLog.tobytes() == b.BnbLog.tobytes() and a.BnbInfo == b.BnbInfo
    assert a.BnbRound.tolist() == b.BnbRound.tolist() and a.BnbDiver.tolist() == b.BnbDiver.tolist()
    assert np.array_equal(_u64(a.Solution), _u64(b.Solution)) and a.OptimalValue == b.OptimalValue
    assert a.BnbInfo["largest_batch"] == 16 and a.BnbInfo["steals"] > 0 and a.BnbInfo["rounds"] < a.Nodes


@pytest.mark.parametrize("name", ["general", "lowers", "min", "mixed", "infeasible"])
def test_driver_on_small_models(gpu, name):
    c, A, rel, b, upper, lower, is_int, sense = N.small_models()[name]
    seq = L.solve2(c, A, b, upper, lower=lower, is_int=is_int, sense=sense, rel=rel)
    want = V.solve_divers(c, A, b, upper, 4, lower=lower, is_int=is_int, sense=sense, rel=rel)
    res = gpu.LPSolver().SolveBnbBounded(_problem(gpu, c, A, rel, b, sense), upper, lower=lower, integer=is_int, divers=4)
    assert res.Status == seq["status"] and (seq["status"] == L.INFEASIBLE) == (name == "infeasible")
    if seq["status"] == L.OPTIMAL:
        assert abs(res.OptimalValue - seq["value"]) <= REL * max(1.0, abs(seq["value"]))
    _same_solve(res, want)


def test_driver_refuses_a_root_that_does_not_fit(gpu):
    from linear_programming_solver_lpr381_amd import synth
    c, A, b = synth.dense_lp(256, 512, seed=1)
    p = _problem(gpu, np.abs(c), np.abs(A), np.zeros(256, dtype=np.int32), np.abs(A).sum(axis=1) * 0.3)
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver().SolveBnbBounded(p, 1.0, divers=4, max_nodes=1)
    assert e.value.code == gpu._lib.EINVAL and "does not fit" in str(e.value)


# ---- 9. the command line -------------------------------------------------------------------------------------------------
def test_cli_divers(gpu):
    def cli(*args):
        return subprocess.run([CLI, "--binary", "--bnb-bounded", *args, EXAMPLE], capture_output=True, text=True)
    one, chip = cli("--divers", "1"), cli("--node-form", "onchip")
    assert one.returncode == 0 and chip.returncode == 0, one.stderr + chip.stderr
    assert one.stdout == chip.stdout and "nodes: " in one.stdout
    p = gpu.ParseFromText(open(EXAMPLE).read())
    for W in (4, 64):
        r = cli("--divers", str(W), "--long-step", "--cutoff")
        assert r.returncode == 0, r.stderr
        res = gpu.LPSolver().SolveBnbBounded(p, 1.0, divers=W, long_step=True, cutoff=True)
        nodes, events, flips = map(int, re.search(r"nodes: (\d+), dual events: (\d+), dual-feasibility flips: (\d+)", r.stdout).groups())
        assert (nodes, events, flips) == (res.Nodes, res.BnbInfo["events"], res.BnbInfo["flips"])
        assert res.Summary.strip() in r.stdout
    r = subprocess.run([CLI, "--binary", "--divers", "4", EXAMPLE], capture_output=True, text=True)
    assert r.returncode == 64 and "--divers needs --bnb-bounded" in r.stderr
    r = cli("--divers", "4", "--node-form", "launches")
    assert r.returncode == 64 and "not with --node-form launches" in r.stderr
    for bad in ("0", "1025", "many"):
        r = cli("--divers", bad)
        assert r.returncode == 64 and "--divers takes a count in [1, 1024]" in r.stderr
