"""GPU tests of the plunge (csrc/lpx_bounded_plunge.hip: lpx_bounded_plunge_onchip; lpx_node_batch_plunge,
lpx_solve_bnb_bounded5): every chain bit for bit against a twin handle driven by single on-chip node calls and against the
NumPy restatement (tests/_bnb_plunge_ref.py) -- the record sequence and the final tableau, basis, flip, ub, lo, trace, counts and
solution; every way a chain ends; the lower-shift mark raised inside a launch; refusals; mixed launches; the driver's log with
round, diver and step against the restatement, and its two identities."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bnb_plunge_ref as P
import _bounded_dual_ref as D
import _bounded_long_ref as L
import _bounded_ref as B
from _node_helpers import (Pool as _Pool, bits as _bits, covering_with_fixed as _covering_with_fixed, fresh as _fresh, node as _node,
                           reads as _reads, same_record as _same_record, same_state as _same_handle, slack_handle as _slack_handle,
                           u64 as _u64)

pytestmark = pytest.mark.gpu

INF = np.inf
SKIP, LONG, CUT = L.SKIP_FIXED, L.LONG_STEP, L.CUTOFF_FLAG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
EXAMPLE = os.path.join(ROOT, "integration", "Input", "example_bounded.txt")


@functools.lru_cache(maxsize=None)
def _root(n, m, seed):
    """The solved root of binary_model(n, m, seed): (T, basis, ub) before the solve and (Ts, bs, ub, flip) after it."""
    T, basis, ub, model, Ts, bs, flip = D.root(n, m, seed)
    return (T, basis, ub), (Ts, bs, ub, flip)


def _solved(lpx, n, m, seed):
    (T, basis, ub), root = _root(n, m, seed)
    dt = _fresh(lpx, T, basis, ub)
    status, _ = dt.bounded_run()
    assert status == B.OPTIMAL and np.array_equal(_u64(dt.download()[0]), _u64(root[0]))
    return dt


def _goes_on(rec, prune):
    return rec["status"] == L.OPTIMAL and rec["var"] >= 0 and not rec["z"] <= prune


def _twin_chain(twin, nd, nint, depth, prune, flags, cutoff, **kw):
    """The chain as single on-chip node calls, one after another: the contract of lpx_node_batch_plunge."""
    cols, lower, upper = nd
    recs = []
    for s in range(depth):
        rec = twin.bounded_node(cols, lower, upper, nint, long_step=bool(flags & LONG), cutoff=cutoff, form="onchip", **kw)
        recs.append(rec)
        if not _goes_on(rec, prune):
            break
        v = rec["var"]
        lo, ub, _ = twin.bound_state()
        cols, lower, upper = [v], [np.ceil(rec["x_var"])], [lo[v] + ub[v]]
    return recs


def _want_chain(h, nd, nint, depth, prune, flags, cutoff, **kw):
    return P.chain(h, nd, nint, depth, prune, None, SKIP | flags | (0 if cutoff is None else CUT), -INF if cutoff is None else cutoff, **kw)


def _check_chain(got, dt, twin, h, nd, nint, depth, prune=-INF, flags=0, cutoff=None, what="", **kw):
    """got: the chain nb.plunge returned for this entry on dt.  Returns the restatement's records."""
    ref = _twin_chain(twin, nd, nint, depth, prune, flags, cutoff, **kw)
    want = _want_chain(h, nd, nint, depth, prune, flags, cutoff, **kw)
    assert len(got) == len(ref) == len(want), (what, len(got), len(ref), len(want))
    for g, r, w in zip(got, ref, want):
        _same_record(g, r); _same_record(g, w)
    _same_handle(dt, h, what)
    assert dt.trace().tolist() == h.trace.tolist(), what
    assert _reads(dt, nint) == _reads(twin, nint), "the chain differs from its twin on the single-node form " + what
    last = want[-1]
    assert dt.bounded_counts() == (last["kind0"], last["kind1"], last["events"] - last["kind0"] - last["kind1"])
    return want


# ---- 1. a chain at every cap, plain loop and long step, on the two benchmark shapes ------------------------------------------
@pytest.mark.parametrize("flags", [0, LONG])
@pytest.mark.parametrize("n,m,shape", [(60, 12, (13, 73)), (128, 64, (65, 193))])
def test_chain_at_every_cap(gpu, n, m, shape, flags):
    assert _root(n, m, 1)[0][0].shape == shape
    with _Pool() as pool:
        for depth, D_ in ((1, 1), (2, 2), (3, 3), (2, 5), (64, 64)):
            dt, twin = pool.add(_solved(gpu, n, m, 1)), pool.add(_solved(gpu, n, m, 1))
            h = L.Handle(*_root(n, m, 1)[1])
            with gpu.NodeBatch([dt]) as nb:
                got = nb.plunge([0], [_node()], n, depth, D_, -INF, long_step=bool(flags))
                assert len(got) == 1
                want = _check_chain(got[0], dt, twin, h, _node(), n, depth, flags=flags, what="depth %d" % depth)
                if depth < 64:
                    assert len(want) == depth and _goes_on(want[-1], -INF), "the chain does not end at its cap"
                else:
                    assert len(want) >= 28 and not _goes_on(want[-1], -INF)
                    assert any(w["flips"] > 0 for w in want[1:]) or any(w["events"] > 2 for w in want[1:])
                # node 0 had lo all zero: the lower-shift mark was raised inside the launch, and a following node of the
                # launches form on the same handle agrees
                if depth > 1:
                    assert np.any(h.lo != 0.0)
                k = int(np.flatnonzero((h.ub[:n] > 0.0) & (h.lo[:n] == 0.0))[0])
                a = dt.bounded_node([k], [0.0], [0.0], n, long_step=bool(flags), form="launches")
                b = twin.bounded_node([k], [0.0], [0.0], n, long_step=bool(flags), form="launches")
                _same_record(a, b)
                _same_record(a, h.node2(*_node([k], [0.0], [0.0]), n, flags=SKIP | flags))
                assert _reads(dt, n) == _reads(twin, n)


def test_depth_one_is_the_batch_run(gpu):
    n, m = 40, 20
    j, l, u = D.children(n, m, 1)[0]
    with _Pool() as pool:
        a, b = pool.add(_solved(gpu, n, m, 1)), pool.add(_solved(gpu, n, m, 1))
        with gpu.NodeBatch([a]) as na, gpu.NodeBatch([b]) as nbb:
            for nd in (_node(), _node([j], [l], [u])):
                got = na.plunge([0], [nd], n, 1, 1, -INF)
                ref = nbb.run([0], [nd], n)
                assert len(got[0]) == 1
                _same_record(got[0][0], ref[0])
                assert _reads(a, n) == _reads(b, n)


# ---- 2. every way a chain ends ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _free_chain(n, m, seed, flags=0):
    h = L.Handle(*_root(n, m, seed)[1])
    return P.chain(h, _node(), n, 64, flags=SKIP | flags)


@pytest.mark.parametrize("flags", [0, LONG])
def test_chain_ends(gpu, flags):
    n, m = 40, 20
    free = _free_chain(n, m, 1, flags)
    assert len(free) >= 10 and free[-1]["status"] == L.INFEASIBLE
    z = [r["z"] for r in free]
    most = max(range(1, len(free) - 1), key=lambda s: free[s]["events"])
    cases = {
        "infeasible": dict(depth=64),
        "prune": dict(depth=64, prune=z[3]),                              # record 3 is the first with z <= prune
        "prune_at_once": dict(depth=64, prune=INF),
        "cutoff": dict(depth=64, cutoff=0.5 * (z[4] + z[5])),             # node 5 starts above the cutoff and falls below it
        "iteration_limit": dict(depth=64, max_iter=free[most]["events"] - 1 if free[most]["events"] > 1 else 1),
    }
    with _Pool() as pool:
        names = sorted(cases)
        dts = [pool.add(_solved(gpu, n, m, 1)) for _ in names]
        twins = [pool.add(_solved(gpu, n, m, 1)) for _ in names]
        ends = {}
        with gpu.NodeBatch(dts) as nb:
            for i, name in enumerate(names):                              # max_iter and the cutoff flag are shared by a launch
                c = dict(cases[name])
                depth, prune, cutoff = c.pop("depth"), c.pop("prune", -INF), c.pop("cutoff", None)
                got = nb.plunge([i], [_node()], n, depth, 64, prune, long_step=bool(flags),
                                cutoffs=None if cutoff is None else [cutoff], **c)
                h = L.Handle(*_root(n, m, 1)[1])
                want = _check_chain(got[0], dts[i], twins[i], h, _node(), n, depth, prune, flags, cutoff, what=name, **c)
                ends[name] = (len(want), want[-1]["status"])
        assert ends["infeasible"] == (len(free), L.INFEASIBLE)
        assert ends["prune"] == (4, L.OPTIMAL) and ends["prune_at_once"] == (1, L.OPTIMAL)
        assert ends["cutoff"][1] == L.CUTOFF and 2 <= ends["cutoff"][0] <= 6
        assert ends["iteration_limit"][1] == L.ITER_LIMIT and ends["iteration_limit"][0] >= 1


@pytest.mark.parametrize("n,m,seed,length", [(12, 6, 3, 5), (16, 8, 2, 7), (128, 64, 1, 58)])
def test_chain_that_ends_in_an_incumbent(gpu, n, m, seed, length):
    with _Pool() as pool:
        dt, twin = pool.add(_solved(gpu, n, m, seed)), pool.add(_solved(gpu, n, m, seed))
        h = L.Handle(*_root(n, m, seed)[1])
        with gpu.NodeBatch([dt]) as nb:
            got = nb.plunge([0], [_node()], n, 64, 64, -INF)
        want = _check_chain(got[0], dt, twin, h, _node(), n, 64, what="incumbent")
        assert len(want) == length and want[-1]["status"] == L.OPTIMAL and want[-1]["var"] == -1
        x, z, _ = dt.bounded_solution(n)
        xr = N.values(h.T, h.basis, h.flip, h.ub, h.lo, n)
        assert np.array_equal(_u64(x), _u64(xr)) and _bits(z) == _bits(want[-1]["z"])
        assert np.all(np.abs(x - np.rint(x)) <= 1e-6), "not an integral point"


# ---- 3. the fit boundary and the staging offsets ----------------------------------------------------------------------------
def _ones_mostly(K):
    return (np.arange(K) % 3 != 0).astype(np.float64)


FIT = {"2x5055": (1, 5053, 0), "140x141": (139, 1, 0), "9x1837_K65": (8, 1828, 65), "9x1837_K1025": (8, 1828, 1025)}


@pytest.mark.parametrize("flags", [0, LONG])
@pytest.mark.parametrize("name", sorted(FIT))
def test_chain_at_the_fit_boundary_and_after_a_large_edit(gpu, name, flags):
    m, n, K = FIT[name]
    T, basis, ub = _covering_with_fixed(m, n, 1)
    lib = gpu._lib.lib()
    assert lib.lpx_bounded_node_fits(*T.shape) == 1
    if K == 0:                                                            # the persistent tile fills the LDS: one more row or column does not fit
        assert lib.lpx_bounded_node_fits(T.shape[0] + 1, T.shape[1]) == 0 or lib.lpx_bounded_node_fits(T.shape[0], T.shape[1] + 2) == 0
    free = np.flatnonzero(ub[:n] > 0)
    cols = free[:K].astype(np.int32)
    nd = (cols, _ones_mostly(K), _ones_mostly(K))
    depth = 4
    with _Pool() as pool:
        dt, twin = pool.add(_fresh(gpu, T, basis, ub)), pool.add(_fresh(gpu, T, basis, ub))
        h = _slack_handle(T, basis, ub)
        with gpu.NodeBatch([dt]) as nb:
            if K == 1025:                                                 # the slab and the staging grow between two calls
                warm = nb.plunge([0], [_node()], n, 1, 1, INF, long_step=bool(flags))
                _check_chain(warm[0], dt, twin, h, _node(), n, 1, INF, flags, what="warm")
            got = nb.plunge([0], [nd], n, depth, depth, -INF, long_step=bool(flags))
            want = _check_chain(got[0], dt, twin, h, nd, n, depth, flags=flags, what=name)
            assert want[0]["events"] > 0 and len(want) >= (2 if name == "140x141" else 3), [w["status"] for w in want]
            # what the staging held is gone from the contract's view: a further chain on the same handle and batch agrees
            more = nb.plunge([0], [_node()], n, 2, depth, -INF, long_step=bool(flags))
            _check_chain(more[0], dt, twin, h, _node(), n, 2, flags=flags, what=name + " again")


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_a_refused_entry_between_two_good_ones(gpu):
    T, basis, ub, _ = B.binary_bounded(12, 6, 1)
    bad_ub = ub.copy(); bad_ub[11] = INF                                  # T[m,11] = -c_11 < 0 with no upper bound
    n = 40
    with _Pool() as pool:
        good0, twin0 = pool.add(_fresh(gpu, T, basis, ub)), pool.add(_fresh(gpu, T, basis, ub))
        bad = pool.add(_fresh(gpu, T, basis, bad_ub))
        good2, twin2 = pool.add(_solved(gpu, n, 20, 1)), pool.add(_solved(gpu, n, 20, 1))
        before_bad = _reads(bad, 11)
        edit = _node([0, 5], [0.0, 1.0], [0.0, 1.0])
        with gpu.NodeBatch([good0, bad, good2]) as nb:
            got = nb.plunge([0, 1, 2], [edit, edit, _node()], 11, [3, 3, 2], 3, -INF)
            msg = gpu._lib.last_error()
            assert len(got[1]) == 1 and got[1][0]["status"] is None and got[1][0]["unrepairable"] == 1
            assert "lpx_node_batch_plunge: entry 1: 1 column(s) with a negative reduced cost and no upper bound" in msg
            assert _reads(bad, 11) == before_bad, "the refused entry changed its handle"
            _check_chain(got[0], good0, twin0, _slack_handle(T, basis, ub), edit, 11, 3, what="entry 0")
            _check_chain(got[2], good2, twin2, L.Handle(*_root(n, 20, 1)[1]), _node(), 11, 2, what="entry 2")
            # a column not known to be integral cannot be plunged into; depth 1 still runs
            with pytest.raises(gpu.LpxError) as e:
                nb.plunge([1], [_node()], 12, 2, 2, -INF)
            assert e.value.code == gpu._lib.EINVAL and "lpx_node_batch_plunge: entry 0: depth > 1 needs finite integral bounds" in str(e.value)
            assert "column 11" in str(e.value) and _reads(bad, 11) == before_bad
            half = _node([3], [0.0], [0.5])
            with pytest.raises(gpu.LpxError) as e:
                nb.plunge([0], [half], 11, 2, 2, -INF)
            assert "column 3 is not known" in str(e.value)
            # the entry's own triples count: giving column 11 a bound lets the chain run
            fix = _node([11], [0.0], [1.0])
            got = nb.plunge([1], [fix], 12, 3, 3, -INF)
            hb = _slack_handle(T, basis, bad_ub)
            want = P.chain(hb, fix, 12, 3)
            assert len(got[0]) == len(want)
            for g, w in zip(got[0], want):
                _same_record(g, w)
            _same_handle(bad, hb)


# ---- 5. one mixed launch, permuted; more entries than compute units; independence ------------------------------------------
@pytest.mark.parametrize("flags", [0, LONG])
def test_one_mixed_launch_and_its_permutation(gpu, flags):
    j, l, u = D.children(40, 20, 1)[0]
    cols = np.array(sorted(N.CYCLING_ONES + N.CYCLING_ZEROS), dtype=np.int32)
    vals = np.array([1.0 if c in N.CYCLING_ONES else 0.0 for c in cols])
    spec = [("root", (40, 20, 1), _node(), 5), ("root", (40, 20, 1), _node([j], [l], [u]), 3), ("root", (64, 32, 1), (cols, vals, vals), 4),
            ("root", (60, 12, 1), _node(), 1), ("cover", (31, 40), _node(), 2), ("cover", (15, 48), _node(), 6), ("root", (40, 20, 2), _node(), 8)]
    nint = 40                                                             # shared by the launch: the narrowest handles have 40 columns

    def make(pool):
        out = []
        for kind, arg, nd, depth in spec:
            if kind == "root":
                out.append((pool.add(_solved(gpu, *arg)), pool.add(_solved(gpu, *arg)), L.Handle(*_root(*arg)[1]), nd, depth))
            else:
                T, basis, ub = _covering_with_fixed(*arg, 1)
                out.append((pool.add(_fresh(gpu, T, basis, ub)), pool.add(_fresh(gpu, T, basis, ub)), _slack_handle(T, basis, ub), nd, depth))
        return out

    with _Pool() as pool:
        lengths = None
        for order in (list(range(len(spec))), [4, 6, 0, 2, 5, 1, 3]):
            ent = make(pool)
            with gpu.NodeBatch([e[0] for e in ent]) as nb:
                got = nb.plunge(order, [ent[s][3] for s in order], nint, [ent[s][4] for s in order], 8, -INF, long_step=bool(flags))
            seen = {}
            for i, s in enumerate(order):
                dt, twin, h, nd, depth = ent[s]
                want = _check_chain(got[i], dt, twin, h, nd, nint, depth, flags=flags, what="entry %d on slot %d" % (i, s))
                seen[s] = [(w["status"], w["events"], w["var"], _bits(w["z"])) for w in want]
            assert lengths is None or seen == lengths, "an entry depends on its place in the launch"
            lengths = seen
        assert len(lengths[0]) == 5 and len(lengths[6]) == 8 and len(lengths[3]) == 1


def test_more_entries_than_compute_units(gpu):
    W = 260
    T, basis, ub = _covering_with_fixed(139, 1, 1)
    h = _slack_handle(T, basis, ub)
    want = P.chain(h, _node(), 1, 4)
    assert len(want) == 2 and want[0]["var"] == 0 and want[-1]["var"] == -1
    Ts, bs, ubs = _covering_with_fixed(2, 1, 1)                           # the rest of the grid: tiny handles, chains of one
    with _Pool() as pool:
        hs = [pool.add(_fresh(gpu, T, basis, ub)) if i % 64 == 3 else pool.add(_fresh(gpu, Ts, bs, ubs)) for i in range(W)]
        with gpu.NodeBatch(hs) as nb:
            got = nb.plunge(np.arange(W), [_node()] * W, 1, 4, 4, -INF)
        first = _reads(hs[3], 1)
        small = _reads(hs[0], 1)
        for i in range(W):
            if i % 64 == 3:
                assert len(got[i]) == 2
                for g, w in zip(got[i], want):
                    _same_record(g, w)
                assert _reads(hs[i], 1) == first
            else:
                assert _reads(hs[i], 1) == small and len(got[i]) == len(got[0])
        _same_handle(hs[3], h)


def test_an_entry_does_not_depend_on_its_neighbours(gpu):
    n = 40
    with _Pool() as pool:
        alone, last = pool.add(_solved(gpu, n, 20, 1)), pool.add(_solved(gpu, n, 20, 1))
        crowd = []
        for k in range(5):
            T, basis, ub = _covering_with_fixed(*((15, 48), (31, 40), (8, 100), (63, 190), (20, 44))[k], 1)
            crowd.append(pool.add(_fresh(gpu, T, basis, ub)))
        with gpu.NodeBatch([alone]) as one, gpu.NodeBatch(crowd + [last]) as six:
            a = one.plunge([0], [_node()], n, 6, 6, -INF)[0]
            b = six.plunge(list(range(6)), [_node()] * 6, n, [1, 2, 3, 4, 5, 6], 6, -INF)[5]
        assert len(a) == len(b) == 6
        for x, y in zip(a, b):
            _same_record(x, y)
        assert _reads(alone, n) == _reads(last, n)


# ---- 6. the driver ----------------------------------------------------------------------------------------------------------
def _problem(lpx, c, A, rel, b, sense=0):
    return lpx.LPProblem.from_arrays(sense, c, A, rel, b)


@functools.lru_cache(maxsize=None)
def _want_plunge(n, m, seed, W, D_, flags, max_nodes=0):
    c, A0, b0 = N.binary_model(n, m, seed)
    return P.solve_plunge(c, A0, b0, np.ones(n), W, D_, search_flags=flags, max_nodes=max_nodes)


def _same_solve(res, want):
    log = res.BnbLog
    assert len(log) == len(want["log"]) == res.Nodes == want["nodes"]
    for k in ("depth", "K", "status", "events", "flips", "var"):
        assert np.array_equal(log[k], want["log"][k]), k
    assert np.array_equal(_u64(log["z"]), _u64(want["log"]["z"])), "z bits of some node differ"
    assert res.BnbRound.tolist() == want["round"].tolist() and res.BnbDiver.tolist() == want["diver"].tolist()
    assert res.BnbStep.tolist() == want["step"].tolist()
    for k in ("nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K", "rounds", "steals", "largest_batch",
              "launched", "dropped", "longest_chain"):
        assert res.BnbInfo[k] == want[k], k
    assert res.Status == want["status"]
    if want["status"] == L.OPTIMAL:
        assert np.array_equal(_u64(res.Solution), _u64(want["x"])) and _bits(res.OptimalValue) == _bits(want["value"])


@pytest.mark.parametrize("flags", [0, LONG | CUT])
@pytest.mark.parametrize("D_", [1, 2, 8, 64])
@pytest.mark.parametrize("W", [1, 2, 8, 64])
@pytest.mark.parametrize("n,m,seed", [(16, 8, 1), (32, 16, 2)])
def test_driver_log_bit_for_bit(gpu, n, m, seed, W, D_, flags):
    c, A0, b0 = N.binary_model(n, m, seed)
    want = _want_plunge(n, m, seed, W, D_, flags)
    p = _problem(gpu, c, A0, np.zeros(m, dtype=np.int32), b0)
    kw = dict(long_step=bool(flags & LONG), cutoff=bool(flags & CUT))
    res = gpu.LPSolver().SolveBnbBounded(p, np.ones(n), divers=W, plunge=D_, **kw)
    assert want["rc"] == 0 and want["nodes"] > 50
    _same_solve(res, want)
    if D_ == 1:                                              # the first identity: plunge = 1 is the search by W divers
        ref = gpu.LPSolver().SolveBnbBounded(p, np.ones(n), divers=W, **kw)
        assert res.BnbLog.tobytes() == ref.BnbLog.tobytes()
        assert res.BnbRound.tolist() == ref.BnbRound.tolist() and res.BnbDiver.tolist() == ref.BnbDiver.tolist()
        assert {k: res.BnbInfo[k] for k in ref.BnbInfo} == ref.BnbInfo and res.Summary == ref.Summary
        assert np.array_equal(_u64(res.Solution), _u64(ref.Solution)) and _bits(res.OptimalValue) == _bits(ref.OptimalValue)
    if W == 1:                                               # the second: one diver with any plunge is the sequential driver on chip
        ref = gpu.LPSolver().SolveBnbBounded(p, np.ones(n), node_form="onchip", **kw)
        assert res.BnbLog.tobytes() == ref.BnbLog.tobytes()
        assert {k: res.BnbInfo[k] for k in ref.BnbInfo} == ref.BnbInfo and res.Summary == ref.Summary
        assert np.array_equal(_u64(res.Solution), _u64(ref.Solution)) and _bits(res.OptimalValue) == _bits(ref.OptimalValue)
        assert res.BnbInfo["dropped"] == 0 and res.BnbInfo["launched"] == res.Nodes
        res2 = gpu.LPSolver().SolveBnbBounded(p, np.ones(n), plunge=D_, **kw)          # plunge without divers means one diver
        assert res2.BnbLog.tobytes() == res.BnbLog.tobytes() and res2.BnbInfo == res.BnbInfo
    if W == 8 and D_ == 8:
        assert res.BnbInfo["dropped"] > 0 and res.BnbInfo["longest_chain"] >= 7


def test_driver_node_limit_cuts_a_round_short(gpu):
    n, m, seed, W, D_ = 16, 8, 1, 8, 4
    full = _want_plunge(n, m, seed, W, D_, 0)
    limit = int(np.flatnonzero(full["round"] == 3)[2]) + 1                            # inside round 3
    want = _want_plunge(n, m, seed, W, D_, 0, limit)
    assert want["rc"] == L.ITER_LIMIT and want["nodes"] == limit
    assert any(cap < D_ for _, _, _, _, cap in want["chains"]), "no cap was cut by the node limit"
    c, A0, b0 = N.binary_model(n, m, seed)
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver().SolveBnbBounded(_problem(gpu, c, A0, np.zeros(m, dtype=np.int32), b0), np.ones(n), max_nodes=limit, divers=W, plunge=D_)
    assert e.value.code == gpu._lib.ITER_LIMIT and "node limit of %d reached" % limit in str(e.value)
    _same_solve(e.value.result, want)


def test_driver_iteration_limit_ends_the_solve_at_that_record(gpu):
    n, m, seed, W, D_ = 40, 20, 1, 8, 8                      # the root takes 31 events; some node would take more than 32
    c, A0, b0 = N.binary_model(n, m, seed)
    want = P.solve_plunge(c, A0, b0, np.ones(n), W, D_, max_iter=32)
    assert want["rc"] == L.ITER_LIMIT and want["log"]["status"][-1] == L.ITER_LIMIT
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver(max_iter=32).SolveBnbBounded(_problem(gpu, c, A0, np.zeros(m, dtype=np.int32), b0), np.ones(n), divers=W, plunge=D_)
    assert e.value.code == gpu._lib.ITER_LIMIT and "node %d (depth" % (want["nodes"] - 1) in str(e.value)
    _same_solve(e.value.result, want)


def test_two_solves_in_a_row_give_identical_logs(gpu):
    c, A0, b0 = N.binary_model(32, 16, 2)
    p = _problem(gpu, c, A0, np.zeros(16, dtype=np.int32), b0)
    a = gpu.LPSolver().SolveBnbBounded(p, 1.0, divers=16, plunge=8, long_step=True, cutoff=True)
    b = gpu.LPSolver().SolveBnbBounded(p, 1.0, divers=16, plunge=8, long_step=True, cutoff=True)
    assert a.BnbLog.tobytes() == b.BnbLog.tobytes() and a.BnbInfo == b.BnbInfo
    assert a.BnbRound.tolist() == b.BnbRound.tolist() and a.BnbDiver.tolist() == b.BnbDiver.tolist() and a.BnbStep.tolist() == b.BnbStep.tolist()
    assert np.array_equal(_u64(a.Solution), _u64(b.Solution)) and a.OptimalValue == b.OptimalValue
    assert a.BnbInfo["largest_batch"] == 16 and a.BnbInfo["longest_chain"] >= 3 and a.BnbInfo["rounds"] < a.Nodes


@pytest.mark.parametrize("name", ["general", "lowers", "min", "mixed", "infeasible"])
def test_driver_on_small_models(gpu, name):
    c, A, rel, b, upper, lower, is_int, sense = N.small_models()[name]
    want = P.solve_plunge(c, A, b, upper, 4, 4, lower=lower, is_int=is_int, sense=sense, rel=rel)
    res = gpu.LPSolver().SolveBnbBounded(_problem(gpu, c, A, rel, b, sense), upper, lower=lower, integer=is_int, divers=4, plunge=4)
    _same_solve(res, want)


def test_driver_refuses_a_root_that_does_not_fit(gpu):
    from linear_programming_solver_lpr381_amd import synth
    c, A, b = synth.dense_lp(256, 512, seed=1)
    p = _problem(gpu, np.abs(c), np.abs(A), np.zeros(256, dtype=np.int32), np.abs(A).sum(axis=1) * 0.3)
    with pytest.raises(gpu.SolverException) as e:
        gpu.LPSolver().SolveBnbBounded(p, 1.0, divers=4, plunge=4, max_nodes=1)
    assert e.value.code == gpu._lib.EINVAL and "does not fit" in str(e.value)


# ---- 7. the command line ----------------------------------------------------------------------------------------------------
def test_cli_plunge(gpu):
    def cli(*args):
        return subprocess.run([CLI, "--binary", "--bnb-bounded", *args, EXAMPLE], capture_output=True, text=True)
    one, chip = cli("--plunge", "8"), cli("--node-form", "onchip")
    assert one.returncode == 0 and chip.returncode == 0, one.stderr + chip.stderr
    assert one.stdout == chip.stdout and "nodes: " in one.stdout
    p = gpu.ParseFromText(open(EXAMPLE).read())
    r = cli("--divers", "4", "--plunge", "4", "--long-step", "--cutoff")
    assert r.returncode == 0, r.stderr
    res = gpu.LPSolver().SolveBnbBounded(p, 1.0, divers=4, plunge=4, long_step=True, cutoff=True)
    nodes, events, flips = map(int, re.search(r"nodes: (\d+), dual events: (\d+), dual-feasibility flips: (\d+)", r.stdout).groups())
    assert (nodes, events, flips) == (res.Nodes, res.BnbInfo["events"], res.BnbInfo["flips"])
    assert res.Summary.strip() in r.stdout
    r = subprocess.run([CLI, "--binary", "--plunge", "4", EXAMPLE], capture_output=True, text=True)
    assert r.returncode == 64 and "--plunge needs --bnb-bounded" in r.stderr
    r = cli("--plunge", "4", "--node-form", "launches")
    assert r.returncode == 64 and "not with --node-form launches" in r.stderr
    for bad in ("0", "65", "deep"):
        r = cli("--plunge", bad)
        assert r.returncode == 64 and "--plunge takes a depth in [1, 64]" in r.stderr
