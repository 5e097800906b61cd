"""GPU tests of strong branching by on-chip probes (csrc/lpx_bounded_probe.hip; lpx_bounded_probe, lpx_node_batch_run_probe,
lpx_solve_bnb_bounded6): every probe record bit for bit against the NumPy restatement (tests/_bnb_probe_ref.py) and against the
single-node on-chip form on a clone of the handle; the handle untouched; the early exits; the independence of a record from
cand_max, from the batch and from its place in it; the driver's log and counters against the restatement."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bnb_probe_ref as P
import _bounded_dual_ref as D
import _bounded_long_ref as L
import _bounded_ref as B
import _node_helpers as H

pytestmark = pytest.mark.gpu

INF = np.inf
EPS = N.EPS
SKIP, LONG, CUT = L.SKIP_FIXED, L.LONG_STEP, L.CUTOFF_FLAG
AMPLE = 10000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "linear_programming_solver_lpr381_amd", "lpx_cli")
EXAMPLE = os.path.join(ROOT, "integration", "Input", "example_bounded.txt")
REC_INT = ("status", "events", "kind0", "kind1", "flips", "var", "dir")
REC_F64 = ("x_var", "lower", "upper", "z")
BM, BN = 8, 1828                                # 9 x 1837: the widest slack-basis shape with 9 rows that fits


def _same_probe(got, want, what=""):
    assert (got["count"], got["candidates"]) == (want["count"], want["candidates"]), (what, got, want)
    assert H.bits(got["z"]) == H.bits(want["z"]), what
    assert len(got["records"]) == len(want["records"]) == 2 * want["count"], what
    for g, w in zip(got["records"], want["records"]):
        assert {k: g[k] for k in REC_INT} == {k: w[k] for k in REC_INT}, (what, g, w)
        assert all(H.bits(g[k]) == H.bits(w[k]) for k in REC_F64), (what, g, w)
    assert got["idle"] == [w >= 2 * want["count"] for w in range(len(got["idle"]))], what


def _probe(dt, h, nint, cand_max, probe_iter=AMPLE, flags=0, cutoff=None, prune=-INF, is_int=None, last=L.OPTIMAL, twins=True, what=""):
    """One probe call on the device against the restatement and, record by record, against the single-node on-chip form on a
    clone; the handle reads the same before and after."""
    nsol = min(nint, dt.C - 1) if nint else dt.C - 1
    before = H.reads(dt, nsol)
    got = dt.probe(nint, cand_max, probe_iter=probe_iter, is_int=is_int, long_step=bool(flags & LONG), cutoff=cutoff, prune=prune)
    assert H.reads(dt, nsol) == before, "the probe changed its handle " + what
    want = P.probe(h, nint, cand_max, probe_iter, last, is_int, EPS, SKIP | flags | (0 if cutoff is None else CUT),
                   -INF if cutoff is None else cutoff, prune)
    _same_probe(got, want, what)
    if twins:
        for g in got["records"]:
            with dt.clone() as c:
                try:
                    ref = c.bounded_node([g["var"]], [g["lower"]], [g["upper"]], nint, is_int=is_int, long_step=bool(flags & LONG),
                                         cutoff=cutoff, form="onchip", max_iter=probe_iter)
                except Exception as e:                          # the call refuses what the probe marks refused
                    assert g["status"] is None and "lpx_bounded_node3" in str(e), (what, g, e)
                    continue
            assert g["status"] is not None, (what, g, ref)
            assert {k: g[k] for k in REC_INT[:5]} == {k: ref[k] for k in REC_INT[:5]}, (what, g, ref)
            assert H.bits(g["z"]) == H.bits(ref["z"]), (what, g, ref)
        assert H.reads(dt, nsol) == before, "a node on a clone changed the handle " + what
    return got, want


def _solved(lpx, n, m, seed):
    T, basis, ub, model, Ts, bs, flip = D.root(n, m, seed)
    dt = H.fresh(lpx, T, basis, ub)
    status, _ = dt.bounded_run()
    assert status == B.OPTIMAL and np.array_equal(H.u64(dt.download()[0]), H.u64(Ts))
    return dt, L.Handle(Ts, bs, ub, flip)


def _cutoff_between(h, nint, is_int=None):
    """An objective between the children's: some probes end at the cutoff, some do not."""
    zs = sorted(r["z"] for r in P.probe(h, nint, 32, AMPLE, is_int=is_int)["records"] if r["status"] == L.OPTIMAL)
    return zs[len(zs) // 2] if zs else h.T[-1, -1] - 1.0


# ---- 1. records: solved roots, every flag set, every cand_max and probe_iter edge -------------------------------------------
@pytest.mark.parametrize("flags", L.FLAG_SETS)
@pytest.mark.parametrize("n,m,seed", [(16, 8, 1), (64, 32, 1)])
def test_probes_of_a_solved_root(gpu, n, m, seed, flags):
    dt, h = _solved(gpu, n, m, seed)
    with dt:
        cutoff = _cutoff_between(h, n) if flags & CUT else None
        count = len(P.candidates(h, n)[0])
        assert count >= 3
        full, want = _probe(dt, h, n, 32, AMPLE, flags & LONG, cutoff, what="cand_max 32")
        assert want["count"] == count and any(r["events"] > 1 for r in want["records"]), "the probes do no work: the test shows nothing"
        if flags & CUT:
            sts = {r["status"] for r in want["records"]}
            assert L.CUTOFF in sts and len(sts) > 1
        for cm in (1, count, min(count + 1, 32)):
            got, _ = _probe(dt, h, n, cm, AMPLE, flags & LONG, cutoff, twins=False, what="cand_max %d" % cm)
            assert got["records"] == full["records"][:2 * min(cm, count)], "a record depends on cand_max"
        for it in (0, 1):
            got, want = _probe(dt, h, n, 4, it, flags & LONG, cutoff, twins=(n == 16), what="probe_iter %d" % it)
            assert all(r["events"] <= it for r in got["records"])
            assert any(r["status"] == L.ITER_LIMIT for r in got["records"])
        # a node afterwards is the node on a clone taken before the probes
        j = want["records"][0]["var"]
        with dt.clone() as c:
            dt.probe(n, 8, long_step=bool(flags & LONG), cutoff=cutoff)
            a = dt.bounded_node([j], [1.0], [1.0], n, form="onchip")
            b = c.bounded_node([j], [1.0], [1.0], n, form="onchip")
            H.same_record(a, b)
            assert H.reads(dt, n) == H.reads(c, n)


def test_probes_two_levels_down(gpu):
    n = 40
    dt, h = _solved(gpu, n, 20, 1)
    with dt:
        for step in range(2):
            p = N.pick(h.T, h.basis, h.flip, h.ub, h.lo, n)
            nd = H.node([p["var"]], [float(1 - step)], [float(1 - step)])
            want = H.ref_node(h, nd, n)
            H.same_record(dt.bounded_node(*nd, n, form="onchip"), want)
            assert want["status"] == L.OPTIMAL and want["var"] >= 0
        assert h.flip[:n].any() and h.lo.any()
        for flags in (0, LONG):
            _probe(dt, h, n, 4, AMPLE, flags, what="two levels down")


# ---- 2. a lower shift, general integers, a mask -----------------------------------------------------------------------------
def _model_root(lpx, name):
    c, A, rel, b, upper, lower, is_int, sense = N.small_models()[name]
    T0, basis0, ub0, *_ = N.prepare(c, A, b, lower, upper, sense, rel)
    st, Ts, bs, flip, _, _ = B.run(T0, basis0, ub0)
    dt = H.fresh(lpx, T0, basis0, ub0)
    assert dt.bounded_run()[0] == st == B.OPTIMAL
    return dt, L.Handle(Ts, bs, ub0, flip), len(c), is_int


@pytest.mark.parametrize("name", ["lowers", "mixed"])
def test_probes_with_a_lower_shift_and_a_mask(gpu, name):
    dt, h, n, is_int = _model_root(gpu, name)
    with dt:
        p = N.pick(h.T, h.basis, h.flip, h.ub, h.lo, n, is_int)
        j, up = p["var"], h.ub[p["var"]]
        nd = H.node([j], [np.ceil(p["x_var"])], [up])                                  # the ceil child: a non-zero lo
        want = h.node2(*nd, n, is_int, EPS, SKIP)
        H.same_record(dt.bounded_node(*nd, n, is_int=is_int, form="onchip"), want)
        assert want["status"] == L.OPTIMAL and h.lo[j] != 0.0 and want["candidates"] >= 1
        for flags in (0, LONG):
            got, ref = _probe(dt, h, n, 4, AMPLE, flags, is_int=is_int, what=name)
            assert ref["count"] >= 1
            if is_int is not None:
                assert all(is_int[r["var"]] for r in got["records"])
        # a ceil child on the shifted column itself: lower = ceil(x), upper = lo + ub in one addition
        for r in ref["records"]:
            if r["dir"] == 1:
                assert r["upper"] == h.lo[r["var"]] + h.ub[r["var"]] and r["lower"] == np.ceil(r["x_var"])
            else:
                assert r["lower"] == h.lo[r["var"]] and r["upper"] == np.floor(r["x_var"])


# ---- 3. synthetic solved tableaux: ub = +inf candidates, nint edges, a mask --------------------------------------------------
@pytest.mark.parametrize("nint,m,seed", [(12, 9, 3), (70, 40, 5), (1100, 12, 9)])
def test_probes_of_pick_tableaux_with_unbounded_candidates(gpu, nint, m, seed):
    T, basis, ub = H.pick_tableau(nint, m, seed)
    Cm = T.shape[1] - 1
    T[:-1, Cm] = np.minimum(T[:-1, Cm], ub[basis])              # every RHS inside [0, ub] of its basic column: the node is OPTIMAL
    h = H.slack_handle(T, basis, ub)
    with H.fresh(gpu, T, basis, ub) as dt:
        H.same_record(dt.bounded_node([], [], [], Cm, form="onchip"), H.ref_node(h, H.node(), Cm))
        order, x = P.candidates(h, Cm)
        assert np.isinf(h.ub[order[:8]]).any() and np.isfinite(h.ub[order[:8]]).any(), "no unbounded candidate among the first"
        _probe(dt, h, Cm, 8, AMPLE, 0, what="nint = Cm")
        _probe(dt, h, Cm, 8, AMPLE, LONG, twins=False, what="nint = Cm, long step")
        got, _ = _probe(dt, h, 0, 4, AMPLE, twins=False, what="nint = 0")
        assert got["count"] == 0 and got["candidates"] == 0 and all(got["idle"])
        _probe(dt, h, 1, 4, AMPLE, twins=False, what="nint = 1")
        mask = (np.random.default_rng(seed).random(Cm) < 0.5).astype(np.uint8)
        got, _ = _probe(dt, h, Cm, 8, AMPLE, is_int=mask, twins=False, what="mask")
        assert got["count"] >= 1 and all(mask[r["var"]] for r in got["records"])


# ---- 4. the widest 9-row shape that fits ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wide():
    T, basis, ub = H.covering_with_fixed(BM, BN, 1)
    h = H.slack_handle(T, basis, ub)
    rec = H.ref_node(h, H.node(), BN, LONG)
    assert rec["status"] == L.OPTIMAL and rec["candidates"] >= 2
    return T, basis, ub, h, rec


def test_probes_at_the_fit_boundary(gpu):
    T, basis, ub, h, rec = _wide()
    assert T.shape == (9, 1837) and gpu._lib.lib().lpx_bounded_node_fits(9, 1837) == 1 and gpu._lib.lib().lpx_bounded_node_fits(9, 1838) == 0
    with H.fresh(gpu, T, basis, ub) as dt:
        H.same_record(dt.bounded_node([], [], [], BN, long_step=True, form="onchip"), rec)
        _probe(dt, h, BN, 4, AMPLE, LONG, what="9 x 1837")
        _probe(dt, h, BN, 32, AMPLE, 0, twins=False, what="9 x 1837, cand_max 32")


# ---- 5. more than 1024 candidates; ties go to the lowest index across lane blocks --------------------------------------------
def test_more_than_1024_candidates_and_ties_across_lane_blocks(gpu):
    Cm, m = 2200, 3
    g = np.random.default_rng(11)
    T = np.zeros((m + 1, Cm + 1))
    basis = np.array([Cm - 3, Cm - 2, Cm - 1], dtype=np.int32)
    T[np.arange(m), basis] = 1.0
    T[:m, Cm] = 2.0
    T[m, Cm] = 50.0
    J = np.arange(Cm - 3)
    T[m, J] = -1.0                                              # every one is flipped to its fractional upper bound by the K = 0 node
    frac = g.choice(np.array([0.0625, 0.125, 0.875, 0.9375]), size=Cm)      # distances 0.4375 and 0.375
    frac[[5, 5 + 1024]] = 0.25, 0.75                            # distance 0.25 at j and j + 1024: the same lane, the next block
    frac[[70, 70 + 2048]] = 0.75, 0.25
    frac[[1500, 1501]] = 0.625, 0.375                           # distance 0.125: the two first candidates
    ub = 1.0 + frac
    ub[basis] = INF
    h = H.slack_handle(T, basis, ub)
    with H.fresh(gpu, T, basis, ub) as dt:
        want = H.ref_node(h, H.node(), Cm)
        H.same_record(dt.bounded_node([], [], [], Cm, form="onchip"), want)
        assert want["flips"] == len(J) and want["candidates"] == len(J) > 2048 and h.flip[J].all()
        got, ref = _probe(dt, h, Cm, 8, AMPLE, twins=False, what="2197 candidates")
        assert [r["var"] for r in got["records"][::2]][:6] == [1500, 1501, 5, 70, 1029, 2118]
        assert got["candidates"] == len(J) and got["count"] == 8
        _probe(dt, h, Cm, 3, AMPLE, LONG, what="2197 candidates, twins")


# ---- 6. the early exits -------------------------------------------------------------------------------------------------------
def test_early_exits_write_no_record(gpu):
    n = 16
    dt, h = _solved(gpu, n, 8, 1)
    with dt:
        z = float(h.T[-1, -1])
        for prune in (z, np.nextafter(z, INF), INF):
            got, _ = _probe(dt, h, n, 4, prune=prune, twins=False, what="pruned")
            assert got["count"] == 0 and got["candidates"] == 0 and all(got["idle"]) and got["records"] == [] and got["z"] == z
        for prune in (np.nextafter(z, -INF), -INF):            # one ulp below z, and no pruning at all: the probes run
            got, _ = _probe(dt, h, n, 4, prune=prune, twins=False, what="not pruned")
            assert got["count"] == 3 and not any(got["idle"][:6]) and all(got["idle"][6:])
        # a handle whose last node ended INFEASIBLE
        cols = np.arange(n, dtype=np.int32)
        want = H.ref_node(h, H.node(cols, np.ones(n), np.ones(n)), n)
        H.same_record(dt.bounded_node(cols, np.ones(n), np.ones(n), n, form="onchip"), want)
        assert want["status"] == L.INFEASIBLE
        got, _ = _probe(dt, h, n, 4, last=L.INFEASIBLE, twins=False, what="after an infeasible node")
        assert got["count"] == 0 and all(got["idle"]) and H.bits(got["z"]) == H.bits(h.T[-1, -1])


def test_a_refused_node_in_front_of_the_probes(gpu):
    n = 40
    dt, h = _solved(gpu, n, 20, 1)
    good, h2 = _solved(gpu, n, 20, 1)
    with dt, good, gpu.NodeBatch([dt, good]) as nb:
        flipped = int(np.flatnonzero(h.flip[:n])[0])
        before = H.reads(dt, n)
        recs, probes = nb.run_probe([0, 1], [H.node([flipped], [0.0], [INF]), H.node()], n, 4)
        assert recs[0]["status"] is None and H.reads(dt, n) == before
        assert probes[0]["count"] == 0 and all(probes[0]["idle"]) and H.bits(probes[0]["z"]) == H.bits(h.T[-1, -1])
        H.same_record(recs[1], H.ref_node(h2, H.node(), n))
        _same_probe(probes[1], P.probe(h2, n, 4, AMPLE), "the good entry beside the refused one")


# ---- 7. independence: the batch, the order, run + probe, regrowth -----------------------------------------------------------
def _three(gpu):
    """Three handles in different states with their restatements: a root, a child of it, the 9-row wide shape."""
    n = 40
    a, ha = _solved(gpu, n, 20, 1)
    b, hb = _solved(gpu, n, 20, 1)
    j = N.pick(hb.T, hb.basis, hb.flip, hb.ub, hb.lo, n)["var"]
    H.same_record(b.bounded_node([j], [1.0], [1.0], n, form="onchip"), H.ref_node(hb, H.node([j], [1.0], [1.0]), n))
    c, hc = _solved(gpu, 16, 8, 1)
    return [(a, ha, n), (b, hb, n), (c, hc, 16)]


@pytest.mark.parametrize("flags", [0, LONG | CUT])
def test_an_entry_is_the_same_alone_and_among_three_in_any_order(gpu, flags):
    trio = _three(gpu)
    n = 16                                                   # the shared nint: the first 16 columns of every handle
    with H.Pool() as pool:
        for dt, _, _ in trio:
            pool.add(dt)
        k = [int(P.candidates(h, n)[0][-1]) for _, h, _ in trio]           # a K = 1 node on each: the least fractional candidate down
        nodes = [H.node([k[i]], [0.0], [0.0]) for i in range(3)]
        cut = [float(h.T[-1, -1]) - 2.0 for _, h, _ in trio] if flags & CUT else None
        kw = dict(long_step=bool(flags & LONG))
        alone = []
        for i, (dt, h, _) in enumerate(trio):                # alone on a clone, through a batch of one
            with dt.clone() as c, gpu.NodeBatch([c]) as nb:
                alone.append(nb.run_probe([0], [nodes[i]], n, 4, cutoffs=None if cut is None else [cut[i]], **kw))
        clones = [pool.add(dt.clone()) for dt, _, _ in trio]
        with gpu.NodeBatch([dt for dt, _, _ in trio]) as nb:
            recs, probes = nb.run_probe([2, 0, 1], [nodes[2], nodes[0], nodes[1]], n, 4,
                                        cutoffs=None if cut is None else [cut[2], cut[0], cut[1]], **kw)
        for pos, i in enumerate((2, 0, 1)):
            H.same_record(recs[pos], alone[i][0][0])
            assert probes[pos] == alone[i][1][0], "entry %d differs alone and in the batch" % i
            h = trio[i][1]
            want = h.node2(*nodes[i], n, None, EPS, SKIP | flags, -INF if cut is None else cut[i])
            H.same_record(recs[pos], want)
            _same_probe(probes[pos], P.probe(h, n, 4, AMPLE, want["status"], None, EPS, SKIP | flags, -INF if cut is None else cut[i]),
                        "entry %d against the restatement" % i)
        # run_probe is run, a wait, then probe
        with gpu.NodeBatch(clones) as nb:
            recs2 = nb.run([0, 1, 2], nodes, n, cutoffs=cut, **kw)
        for i, c in enumerate(clones):
            H.same_record(recs2[i], recs[(2, 0, 1).index(i)])
            assert H.reads(c, n) == H.reads(trio[i][0], n)
            got = c.probe(n, 4, cutoff=None if cut is None else cut[i], **kw)
            assert got == probes[(2, 0, 1).index(i)], "run + probe differs from run_probe on entry %d" % i
        assert any(p["count"] >= 1 and any(r["events"] > 0 for r in p["records"]) for p in probes)


def test_workspace_regrows_and_serves_a_small_probe_again(gpu):
    T, basis, ub, hw, rec = _wide()
    small, hs = _solved(gpu, 16, 8, 1)
    with H.fresh(gpu, T, basis, ub) as wide, small, gpu.NodeBatch([small, wide]) as nb:
        hw = P.clone(H.slack_handle(T, basis, ub))
        first = nb.run_probe([0], [H.node()], 16, 2)                                   # a small workspace first
        _same_probe(first[1][0], P.probe(hs, 16, 2, AMPLE), "small, before")
        want = H.ref_node(hw, H.node(), BN, LONG)
        recs, probes = nb.run_probe([1], [H.node()], BN, 32, long_step=True)           # it outgrows slab and workspace
        H.same_record(recs[0], want)
        _same_probe(probes[0], P.probe(hw, BN, 32, AMPLE, flags=SKIP | LONG), "wide")
        again = nb.run_probe([0], [H.node()], 16, 2)
        assert again[1] == first[1] and again[0] == first[0]
        both = nb.run_probe([1, 0], [H.node(), H.node()], 16, 3)                       # mixed shapes in one launch
        _same_probe(both[1][1], P.probe(hs, 16, 3, AMPLE), "small beside wide")
        _same_probe(both[1][0], P.probe(hw, 16, 3, AMPLE), "wide beside small")


# ---- 8. the driver ----------------------------------------------------------------------------------------------------------
def _problem(lpx, c, A, rel, b, sense=0):
    return lpx.LPProblem.from_arrays(sense, c, A, rel, b)


@functools.lru_cache(maxsize=None)
def _want_strong(n, m, seed, W, flags, cand_max, probe_iter):
    c, A0, b0 = N.binary_model(n, m, seed)
    return P.solve_strong(c, A0, b0, np.ones(n), W, search_flags=flags, cand_max=cand_max, probe_iter=probe_iter)


def _same_solve(res, want):
    log = res.BnbLog
    assert len(log) == len(want["log"]) == res.Nodes == want["nodes"]
    for k in ("depth", "K", "status", "events", "flips", "var"):
        assert np.array_equal(log[k], want["log"][k]), k
    assert np.array_equal(H.u64(log["z"]), H.u64(want["log"]["z"])), "z bits of some node differ"
    assert res.BnbRound.tolist() == want["round"].tolist() and res.BnbDiver.tolist() == want["diver"].tolist()
    for k in ("nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K", "rounds", "steals",
              "largest_batch") + P.SINFO_KEYS:
        assert res.BnbInfo[k] == want[k], k
    assert res.Status == want["status"]
    if want["status"] == L.OPTIMAL:
        assert np.array_equal(H.u64(res.Solution), H.u64(want["x"])) and H.bits(res.OptimalValue) == H.bits(want["value"])


@pytest.mark.parametrize("probe_iter", [4, AMPLE])
@pytest.mark.parametrize("cand_max", [1, 4])
@pytest.mark.parametrize("flags", [0, LONG | CUT])
@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("n,m,seed", [(16, 8, 1), (24, 8, 1)])
def test_driver_log_and_counters_bit_for_bit(gpu, n, m, seed, W, flags, cand_max, probe_iter):
    c, A0, b0 = N.binary_model(n, m, seed)
    want = _want_strong(n, m, seed, W, flags, cand_max, probe_iter)
    assert want["rc"] == 0 and want["nodes"] > 10 and want["probes"] > 0
    res = gpu.LPSolver().SolveBnbBounded(_problem(gpu, c, A0, np.zeros(m, dtype=np.int32), b0), np.ones(n), divers=W,
                                         long_step=bool(flags & LONG), cutoff=bool(flags & CUT), branching="strong",
                                         candidates=cand_max, probe_iter=probe_iter)
    _same_solve(res, want)
    assert res.BnbInfo["probe_launches"] == res.BnbInfo["rounds"]


@pytest.mark.parametrize("W,flags,cand_max,probe_iter", [(3, LONG | CUT, 4, AMPLE), (1, 0, 1, 4)])
@pytest.mark.parametrize("name", ["general", "lowers", "min", "mixed", "infeasible"])
def test_driver_on_small_models(gpu, name, W, flags, cand_max, probe_iter):
    c, A, rel, b, upper, lower, is_int, sense = N.small_models()[name]
    want = P.solve_strong(c, A, b, upper, W, lower=lower, is_int=is_int, sense=sense, rel=rel, search_flags=flags, cand_max=cand_max,
                          probe_iter=probe_iter)
    res = gpu.LPSolver().SolveBnbBounded(_problem(gpu, c, A, rel, b, sense), upper, lower=lower, integer=is_int, divers=W,
                                         long_step=bool(flags & LONG), cutoff=bool(flags & CUT), branching="strong",
                                         candidates=cand_max, probe_iter=probe_iter)
    assert (want["status"] == L.INFEASIBLE) == (name == "infeasible")
    _same_solve(res, want)


def test_most_fractional_is_the_search_by_divers_and_two_solves_agree(gpu):
    c, A0, b0 = N.binary_model(24, 8, 1)
    p = _problem(gpu, c, A0, np.zeros(8, dtype=np.int32), b0)
    S = gpu.LPSolver()
    plain = S.SolveBnbBounded(p, 1.0, divers=3, long_step=True, cutoff=True)
    most = S.SolveBnbBounded(p, 1.0, divers=3, long_step=True, cutoff=True, branching="most_fractional")
    assert plain.BnbLog.tobytes() == most.BnbLog.tobytes() and plain.Summary == most.Summary
    assert plain.BnbRound.tolist() == most.BnbRound.tolist() and plain.BnbDiver.tolist() == most.BnbDiver.tolist()
    assert {k: most.BnbInfo[k] for k in plain.BnbInfo} == plain.BnbInfo
    assert all(most.BnbInfo[k] == 0 for k in P.SINFO_KEYS)
    assert np.array_equal(H.u64(plain.Solution), H.u64(most.Solution)) and H.bits(plain.OptimalValue) == H.bits(most.OptimalValue)
    a = S.SolveBnbBounded(p, 1.0, divers=3, long_step=True, cutoff=True, branching="strong")
    b = S.SolveBnbBounded(p, 1.0, divers=3, long_step=True, cutoff=True, branching="strong")
    assert a.BnbLog.tobytes() == b.BnbLog.tobytes() and a.BnbInfo == b.BnbInfo
    assert a.Nodes < plain.Nodes and abs(a.OptimalValue - plain.OptimalValue) <= 1e-9 * abs(plain.OptimalValue)
    assert a.BnbInfo["changed_picks"] > 0 and a.BnbInfo["pruned_by_probe"] > 0


def test_cli_strong(gpu):
    r = subprocess.run([CLI, "--binary", "--bnb-bounded", "--branching", "strong", "--candidates", "4", "--probe-iter", "50",
                        "--divers", "2", "--long-step", "--cutoff", EXAMPLE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    p = gpu.ParseFromText(open(EXAMPLE).read())
    res = gpu.LPSolver().SolveBnbBounded(p, 1.0, divers=2, long_step=True, cutoff=True, branching="strong", candidates=4, probe_iter=50)
    nodes, events, flips = map(int, re.search(r"nodes: (\d+), dual events: (\d+), dual-feasibility flips: (\d+)", r.stdout).groups())
    assert (nodes, events, flips) == (res.Nodes, res.BnbInfo["events"], res.BnbInfo["flips"])
    assert res.Summary.strip() in r.stdout
    plain = subprocess.run([CLI, "--binary", "--bnb-bounded", "--branching", "most_fractional", "--divers", "2", EXAMPLE],
                           capture_output=True, text=True)
    ref = subprocess.run([CLI, "--binary", "--bnb-bounded", "--divers", "2", EXAMPLE], capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout == ref.stdout
