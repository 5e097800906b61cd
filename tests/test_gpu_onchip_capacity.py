"""GPU tests of every on-chip bounded kernel on a handle whose live window is not its capacity (the leading dimension is the
capacity's, the shape the live one): the on-chip primal loop alone and in a batch (csrc/lpx_bounded_primal.hip), the fix kernel
(csrc/lpx_bounded_fix.hip) and the guard kernel after rounds of GMI cuts -- cut rows, cut slack columns at or above nint with
ub = +inf, basic columns at or above nint -- with Bland mode entered inside the fix kernel, a batch whose entries have three
different live shapes, and the probe and plunge kernels on a handle with cut rows.  Every comparison is bit for bit against the
existing restatements (record, guard record, triples, trace, tableau, basis, flip, ub, lo), against the twin handle of the
defining property of tightening, and for the kernels that do not reshape the dead region of the handle must keep the values it
held before the call."""
import functools

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bnb_cuts_ref as X
import _bnb_probe_ref as P
import _bnb_tighten_ref as R
import _bounded_guard_ref as GG
import _bounded_long_ref as L
import _bounded_ref as B
import _gmi_ref as G
from _node_helpers import (Pool as _Pool, fresh as _fresh, node as _node, reads as _reads, same_record as _same_record,
                           same_state as _same_state, u64 as _u64)
from test_gpu_bnb_cuts import Pair, _after_rounds, _model as _cuts_model, sentinel_handle
from test_gpu_bnb_tighten import _node5, _same_fixed, _twin
from test_gpu_bounded_primal import _reads as _primal_reads, _record as _primal_record, _ref_reads
from test_gpu_guard import _node4
from test_gpu_plunge import _check_chain
from test_gpu_probe import AMPLE, _same_probe

pytestmark = pytest.mark.gpu

INF = np.inf
SKIP, LONG, CUT = L.SKIP_FIXED, L.LONG_STEP, L.CUTOFF_FLAG
ROOTS = ["lowers", (16, 6, 1)]


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def _cap_handle(gpu, T, basis, ub, extra, seed):
    """A handle of capacity (R + extra, C + extra) whose whole capacity held random finite values before T went into its live
    window, with the bounds ub.  Returns (handle, what the capacity held, the capacity)."""
    Rr, Cc = T.shape
    cap = (Rr + extra, Cc + extra)
    dt, dead = sentinel_handle(gpu, T, basis, *cap, seed)
    dt.set_bounds(ub)
    return dt, dead, cap


def _full(dt, cap):
    """Everything the handle's capacity holds; the live shape is put back."""
    Rr, Cc = dt.R, dt.C
    dt.set_shape(*cap)
    F, _ = dt.download()
    dt.set_shape(Rr, Cc)
    return F


def _dead_kept(before, after, live, what=""):
    dead = np.ones(before.shape, dtype=bool)
    dead[:live[0], :live[1]] = False
    assert np.array_equal(_u64(after)[dead], _u64(before)[dead]), "a kernel wrote outside the live window " + what


def _gap_bound(h, nd, n, mask=None, S=0, flags=0, shifted=False):
    """The node on a copy of the restatement's handle, and the fix_bound that lies the median positive reduced cost of its
    nonbasic integer columns under its objective: about half of those columns then have less than one step.  shifted: the bound
    must also leave some flipped column that stands on a non-zero lower shift less room than its range; where the median does
    not, the bound lies half of the largest d * ub of such a column under the objective.  Returns (fix_bound, the record, the copy)."""
    g = h.clone()
    rec = g.node4(*nd, n, mask, N.EPS, SKIP | flags, -INF, S)
    assert rec["status"] == L.OPTIMAL, rec
    d = g.T[-1, :n].copy()
    d[np.isin(np.arange(n), g.basis)] = 0.0
    assert (d > 1e-9).any()
    gap = float(np.median(d[d > 1e-9]))
    if shifted:
        J = [j for j in range(n) if g.flip[j] and g.lo[j] != 0.0 and d[j] > 1e-9 and g.ub[j] >= 1.0]
        assert J, "no flipped nonbasic column stands on a lower shift"
        if not any(np.floor(gap / d[j]) < g.ub[j] for j in J):
            gap = 0.5 * max(d[j] * g.ub[j] for j in J)
    return rec["z"] - gap, rec, g


def _tighten_handle(p):
    """The pair's restatement handle with lpx_bounded_node5."""
    p.h = R.Handle(p.h.T, p.h.basis, p.h.ub, p.h.flip, p.h.lo)
    return p


def _shifted_after_rounds(gpu, name, **kw):
    """_after_rounds whose node between the two rounds also raises, by one, the lower bound of a nonbasic column that stands at
    its upper bound (flipped) and has a range of two or more: the column does not move, stays flipped and carries a non-zero
    lower shift from then on (the handle's lo starts at zero: the preparation shifts the model's lower bounds out)."""
    p = Pair(gpu, name, 24, **kw)
    p.round(G.CutOpts(cuts_per_round=4))
    h = p.h
    basic = set(h.basis.tolist())
    f = next(j for j in range(p.n) if j not in basic and h.flip[j] and h.ub[j] >= 2.0)
    assert p.node([f], [h.lo[f] + 1.0], [h.lo[f] + h.ub[f]], LONG)["status"] == L.OPTIMAL
    assert p.h.flip[f] and p.h.lo[f] != 0.0 and f not in set(p.h.basis.tolist())
    src, _ = p.round(G.CutOpts(cuts_per_round=4))
    assert len(src) > 0
    return p


def _cut_column_edit(p):
    """A bound edit that moves a nonbasic column with entries in the cut rows by one."""
    h = p.h
    cut_rows = slice(p.first - p.n, h.T.shape[0] - 1)
    basic = set(h.basis.tolist())
    w = next(j for j in range(p.n) if j not in basic and h.ub[j] >= 1.0 and np.any(h.T[cut_rows, j] != 0.0))
    if h.flip[w]:                                                   # at its upper bound: lower that
        return _node([w], [h.lo[w]], [h.lo[w] + h.ub[w] - 1.0])
    return _node([w], [h.lo[w] + 1.0], [h.lo[w] + h.ub[w]])          # at its lower bound: raise that


def _model(name):
    if name[0] == "ip":
        c, A, b, up = R.ip_model(name[1], name[2])
        return c, A, np.zeros(len(b), dtype=np.int32), b, up, None, None, 0
    return _cuts_model(name)


@functools.lru_cache(maxsize=None)
def _lp(name):
    """(T0, basis0, ub0) of the prepared model and the restatement's primal run of it; shared, nothing writes them."""
    c, A, rel, b, upper, lower, mask, sense = _model(name)
    T0, basis0, ub0, *_ = N.prepare(c, A, b, lower, upper, sense, rel)
    return (T0, basis0, ub0), B.run(T0, basis0, ub0)


# ---- 1. the on-chip primal loop on spare capacity -------------------------------------------------------------------------------
PRIMAL = ["lowers", (16, 6, 1), ("ip", 24, 6)]


@pytest.mark.parametrize("extra", [1, 24])
@pytest.mark.parametrize("name", PRIMAL, ids=str)
def test_onchip_primal_on_spare_capacity(gpu, name, extra):
    """extra = 1: the row stride of the tile in LDS (C | 1) and the handle's leading dimension then differ by parity."""
    (T0, basis0, ub0), ref = _lp(name)
    assert ref[0] == B.OPTIMAL and sum(ref[5]) >= 3
    with _Pool() as pool:
        dt, dead, cap = _cap_handle(gpu, T0, basis0, ub0, extra, 100 + extra)
        pool.add(dt)
        twin = pool.add(_fresh(gpu, T0, basis0, ub0))                # exact capacity, the launches form
        assert (dt.R, dt.C) == T0.shape and gpu._lib.lib().lpx_bounded_node_fits(*cap) == 1
        sa, sta = dt.bounded_run(form="onchip")
        sb, stb = twin.bounded_run()
        print(name, "capacity", cap, "live", T0.shape, "ld", dt.ld, "twin ld", twin.ld, "events", ref[5])
        assert sa == sb == ref[0] and sta["launches"] == 1 and sta["pivots"] == stb["pivots"] == ref[5][0] + ref[5][1]
        assert _primal_reads(dt) == _primal_reads(twin), "the on-chip form on spare capacity differs from the launches form"
        assert _primal_reads(dt) == _ref_reads(ref), "the on-chip form on spare capacity differs from the restatement"
        lo, ub, _ = dt.bound_state()
        assert np.array_equal(_u64(ub), _u64(ub0)) and not lo.any()
        _dead_kept(dead, _full(dt, cap), T0.shape)


def test_onchip_primal_batch_over_three_capacities(gpu):
    """One lpx_node_batch_primal launch over three handles with 24, 0 and 1 spare rows and columns."""
    extras = [24, 0, 1]
    order = [2, 0, 1]
    with _Pool() as pool:
        made = [_cap_handle(gpu, *_lp(name)[0], extra, 200 + extra) for name, extra in zip(PRIMAL, extras)]
        hs = [pool.add(m[0]) for m in made]
        with gpu.NodeBatch(hs) as nb:
            recs = nb.solve(order)
        for i, s in enumerate(order):
            ref = _lp(PRIMAL[s])[1]
            assert recs[i] == _primal_record(ref[0], ref), PRIMAL[s]
            assert _primal_reads(hs[s]) == _ref_reads(ref), PRIMAL[s]
            _dead_kept(made[s][1], _full(hs[s], made[s][2]), _lp(PRIMAL[s])[0][0].shape, str(PRIMAL[s]))


# ---- 2. the fix kernel after cut rounds -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1])
@pytest.mark.parametrize("name", ROOTS, ids=str)
def test_fix_kernel_after_cut_rounds(gpu, name, K):
    """lpx_bounded_node5 on a handle two rounds of cuts in, 24 spare rows and columns: K = 0 (the node re-optimises the second
    round's cuts) and K = 1 (its edit moves a nonbasic column with entries in the cut rows).  The root in front of the rounds is
    solved on chip.  On "lowers", whose columns have ranges of three, a flipped column that stands on a non-zero lower shift is
    among the tightened: the flipped branch of the rule forms its upper end from that shift."""
    shifted = name == "lowers"
    make = _shifted_after_rounds if shifted else _after_rounds
    p = _tighten_handle(make(gpu, name, sentinel=300 + K, root_form="onchip"))
    try:
        h, n, cap = p.h, p.n, (p.Rcap, p.Ccap)
        assert h.T.shape[0] > p.T0.shape[0] and h.T.shape[0] < cap[0] and h.T.shape[1] < cap[1]
        nd = _node() if K == 0 else _cut_column_edit(p)
        fb, plain, _ = _gap_bound(h, nd, n, p.mask, shifted=shifted)
        assert plain["events"] >= 1
        before = _full(p.dt, cap)
        lo_before = h.lo.copy()
        with p.dt.clone() as twin:
            want = _node5(p.dt, h, nd, n, fb, is_int=p.mask)
            fc, fl, fu = want["fixed"]
            print(name, "K", K, "live", h.T.shape, "capacity", cap, "events", want["events"], "tightened", fc.tolist(), fl.tolist(), fu.tolist(),
                  "flipped", h.flip[fc].tolist(), "lower shift before", lo_before[fc].tolist(), "basic columns at or above nint", int((h.basis >= n).sum()))
            assert len(fc) >= 1, "no column was tightened"
            assert (h.basis >= n).any(), "no basic column at or above nint"
            assert np.isinf(h.ub[n:]).all() and not h.lo[n:].any() and not h.flip[p.first:].any()
            if shifted:
                assert any(h.flip[j] and lo_before[j] != 0.0 and j not in nd[0] for j in fc), \
                    "no flipped column that stood on a non-zero lower shift was tightened"
            _twin(twin, p.dt, nd, n, want["fixed"], is_int=p.mask)
        _dead_kept(before, _full(p.dt, cap), h.T.shape)
        p.round(G.CutOpts(cuts_per_round=4))                         # the spare capacity is still usable, the tightened bounds are carried
    finally:
        p.close()


# ---- 3. Bland mode inside the fix kernel, and the guard and fix kernels after a cut round ---------------------------------------
COVER = (15, 48, 2)


@pytest.mark.parametrize("extra", [0, 5])
@pytest.mark.parametrize("flags", [0, LONG])
@pytest.mark.parametrize("S", [1, 2])
def test_bland_mode_inside_the_fix_kernel(gpu, S, flags, extra):
    """degenerate_cover(15, 48, 2) as one K = 0 node with every structural column an integer column: the loop of
    lpx_bounded_fix_onchip enters Bland mode (26 to 66 events of it in the restatement) and the rule then tightens 12 to 13
    columns.  extra = 5: the same on a handle with spare capacity."""
    T, basis, ub = GG.degenerate_cover(*COVER)
    nint = COVER[1]
    h = R.Handle(T, basis, ub, np.zeros(len(ub), dtype=np.uint8))
    fb, plain, _ = _gap_bound(h, _node(), nint, None, S, flags)
    with _Pool() as pool:
        dt, dead, cap = _cap_handle(gpu, T, basis, ub, extra, 400 + extra)
        pool.add(dt)
        twin = pool.add(dt.clone())
        want = _node5(dt, h, _node(), nint, fb, S=S, flags=flags)
        print("S", S, "flags", flags, "extra", extra, "events", want["events"], "bland", want["bland_events"], "first", want["first_bland"],
              "tightened", len(want["fixed"][0]))
        assert want["status"] == L.OPTIMAL and want["bland_events"] >= 1 and want["first_bland"] >= S
        assert len(want["fixed"][0]) >= 1
        assert (want["bland_events"], want["first_bland"], want["events"]) == (plain["bland_events"], plain["first_bland"], plain["events"])
        _twin(twin, dt, _node(), nint, want["fixed"], S=S, flags=flags)
        _dead_kept(dead, _full(dt, cap), T.shape)


def test_guard_and_fix_kernels_after_a_cut_round(gpu):
    """degenerate_cover(15, 48, 2) on a handle with 24 spare rows and columns: the root, one bounded round of 4 cuts, and its
    re-optimisation with S = 1 -- by lpx_bounded_node4 (the guard kernel) on a clone and by lpx_bounded_node5 (the fix kernel) on
    the handle.  On this instance the guard fires in that re-optimisation (22 Bland events in the restatement), so
    covering_with_fixed(31, 32, 1), whose re-optimisation makes 3 events and none of them in Bland mode, is not needed."""
    T, basis, ub = GG.degenerate_cover(*COVER)
    nint = COVER[1]
    h = R.Handle(T, basis, ub, np.zeros(len(ub), dtype=np.uint8))
    with _Pool() as pool:
        dt, dead, cap = _cap_handle(gpu, T, basis, ub, 24, 500)
        pool.add(dt)
        root = h.node4(*_node(), nint)
        _same_record(dt.bounded_node(*_node(), nint, form="onchip"), root)
        assert root["status"] == L.OPTIMAL
        _same_state(dt, h, "at the root")
        Cm = T.shape[1] - 1
        flags = np.zeros(Cm, dtype=np.uint8)
        flags[:nint] = 1                                             # the rows have fractional coefficients: continuous slacks
        o = G.CutOpts(cuts_per_round=4)
        src, pcol, _ = X.handle_round(h, flags, Cm, Cm, o, *cap)
        gsrc, gpcol = dt.gmi_round(flags, Cm, opts=gpu.CutOpts(**vars(o)).to_c(), bounded=True)
        assert list(gsrc) == list(src) and list(gpcol) == list(pcol) and len(src) == 4
        _same_state(dt, h, "after the round")
        assert h.T.shape == (T.shape[0] + 4, T.shape[1] + 4)
        before = _full(dt, cap)
        a, twin = pool.add(dt.clone()), pool.add(dt.clone())
        ha = h.clone()
        r4, modes, _ = _node4(a, ha, _node(), nint, 1)
        print("guard kernel: events", r4["events"], "bland", r4["bland_events"], "first", r4["first_bland"])
        assert r4["status"] == L.OPTIMAL and r4["bland_events"] >= 1, "the guard did not fire after the cut round"
        fb, plain, _ = _gap_bound(h, _node(), nint, None, 1)
        want = _node5(dt, h, _node(), nint, fb, S=1)
        print("fix kernel: bland", want["bland_events"], "tightened", len(want["fixed"][0]), "basic at or above nint", int((h.basis >= nint).sum()))
        assert (want["bland_events"], want["first_bland"], want["events"]) == (r4["bland_events"], r4["first_bland"], r4["events"])
        assert len(want["fixed"][0]) >= 1 and (h.basis >= nint).any()
        _twin(twin, dt, _node(), nint, want["fixed"], S=1)
        _dead_kept(before, _full(dt, cap), h.T.shape)


# ---- 4. a batch whose entries have three live shapes ----------------------------------------------------------------------------
def _next_node(h, n, solved):
    """K = 0 on a handle a round has left to re-optimise; else a child of the pick that ends OPTIMAL (the ceil child first)."""
    if not solved:
        return _node()
    pk = N.pick(h.T, h.basis, h.flip, h.ub, h.lo, n)
    if pk["var"] < 0:
        return _node()
    v, xv = pk["var"], pk["x_var"]
    kids = [_node([v], [np.ceil(xv)], [h.lo[v] + h.ub[v]]), _node([v], [h.lo[v]], [np.floor(xv)])]
    for nd in kids:
        if h.clone().node4(*nd, n)["status"] == L.OPTIMAL:
            return nd
    return kids[0]


def test_a_batch_over_three_live_shapes(gpu):
    """One NodeBatch over three handles of binary_model(16, 6, 1): no cuts (and no spare capacity), one round, two rounds.  One
    lpx_node_batch_run, one lpx_node_batch_run2 with S = 1 and one lpx_node_batch_run3 whose fix_bounds mix finite values with -inf,
    the entry order permuted against the handle order: every entry equals its single-node call on a clone and the restatement."""
    name, n = (16, 6, 1), 16
    o = G.CutOpts(cuts_per_round=4)
    ps = [Pair(gpu, name, 0, sentinel=600), Pair(gpu, name, 24, sentinel=601, root_form="onchip"),
          _after_rounds(gpu, name, sentinel=602, root_form="onchip")]
    try:
        src, _ = ps[1].round(o)
        assert len(src) > 0
        for p in ps:
            _tighten_handle(p)
        shapes = [p.h.T.shape for p in ps]
        caps = [(p.Rcap, p.Ccap) for p in ps]
        print("live shapes", shapes, "capacities", caps)
        assert len(set(shapes)) == 3 and shapes[0] == caps[0] and shapes[1] != caps[1] and shapes[2] != caps[2]
        hs = [p.dt for p in ps]
        refs = [p.h for p in ps]
        solved = [True, False, False]
        order = [2, 0, 1]                                            # entry i runs on handles[order[i]]
        with gpu.NodeBatch(hs) as nb:
            for call in ("run", "run2", "run3"):
                nodes = [_next_node(refs[s], n, solved[s]) for s in range(3)]
                S = 1 if call == "run2" else 0
                fbs = [-INF] * 3
                if call == "run3":
                    fbs = [_gap_bound(refs[0], nodes[0], n)[0], -INF, _gap_bound(refs[2], nodes[2], n)[0]]
                before = [_full(hs[s], caps[s]) for s in range(3)]
                with _Pool() as pool:
                    solo = [pool.add(hs[s].clone()) for s in range(3)]
                    kw = {} if call == "run" else {"stall_events": S} if call == "run2" else {"fix_bounds": [fbs[s] for s in order]}
                    got = nb.run(order, [nodes[s] for s in order], n, **kw)
                    for i, s in enumerate(order):
                        want = refs[s].node5(*nodes[s], n, stall_events=S, fix_bound=fbs[s])
                        skw = {} if call == "run" else {"stall_events": S} if call == "run2" else {"fix_bound": fbs[s]}
                        one = solo[s].bounded_node(*nodes[s], n, form="onchip", **skw)
                        for r in (got[i], one):
                            _same_record(r, want)
                            if call != "run":
                                assert (r["bland_events"], r["first_bland"]) == (want["bland_events"], want["first_bland"]), (call, s)
                            if call == "run3":
                                _same_fixed(r["fixed"], want["fixed"])
                        _same_state(hs[s], refs[s], "%s, entry %d on handle %d" % (call, i, s))
                        assert hs[s].trace().tolist() == refs[s].trace.tolist()
                        assert _reads(hs[s], n) == _reads(solo[s], n), (call, s)
                        _dead_kept(before[s], _full(hs[s], caps[s]), shapes[s], "%s, handle %d" % (call, s))
                        print(call, "handle", s, "K", len(nodes[s][0]), "status", want["status"], "events", want["events"], "bland", want["bland_events"],
                              "tightened", len(want["fixed"][0]))
                        solved[s] = want["status"] == L.OPTIMAL
                    if call == "run":
                        assert all(g["events"] >= 1 for g in got), "an entry had nothing to do"
                    if call == "run2":
                        assert sum(g["bland_events"] for g in got) >= 1, "no entry entered Bland mode"
                    if call == "run3":
                        fixed = {s: len(got[i]["fixed"][0]) for i, s in enumerate(order)}
                        assert fixed[1] == 0 and fixed[0] >= 1 and fixed[2] >= 1, fixed
                assert all(solved), "a node of the batch did not end OPTIMAL"
    finally:
        for p in ps:
            p.close()


# ---- 5. the probe and the plunge kernels on a handle with cut rows --------------------------------------------------------------
def test_probe_kernel_on_a_cut_handle(gpu):
    """lpx_node_batch_run_probe on the handle two rounds of cuts in: the node re-optimises the second round's cuts, the probes run on
    the tableau with its cut rows.  cand_max = 2.  The drivers never make this call; the C ABI takes it."""
    p = _after_rounds(gpu, (16, 6, 1), sentinel=700, root_form="onchip")
    try:
        h, n, cap = p.h, p.n, (p.Rcap, p.Ccap)
        before = _full(p.dt, cap)
        want = h.node2(*_node(), n, None, N.EPS, SKIP, -INF)
        with gpu.NodeBatch([p.dt]) as nb:
            recs, probes = nb.run_probe([0], [_node()], n, 2)
        _same_record(recs[0], want)
        assert want["status"] == L.OPTIMAL and want["events"] >= 1
        p.same()
        assert p.dt.trace().tolist() == h.trace.tolist()
        ref = P.probe(h, n, 2, AMPLE, want["status"])
        print("probes", ref["count"], "of", ref["candidates"], "candidates:", [(r["var"], r["dir"], r["status"], r["events"]) for r in ref["records"]])
        assert ref["count"] == 2 and sum(r["events"] for r in ref["records"]) >= 1
        _same_probe(probes[0], ref, "behind the node")
        alone = p.dt.probe(n, 2)                                     # lpx_bounded_probe on the same tableau
        _same_probe(alone, ref, "alone")
        p.same()
        _dead_kept(before, _full(p.dt, cap), h.T.shape)
    finally:
        p.close()


def test_plunge_kernel_on_a_cut_handle(gpu):
    """lpx_node_batch_plunge on the handle two rounds of cuts in: a chain of two nodes, the first of which re-optimises the second
    round's cuts, the tableau with its cut rows staying in LDS between them."""
    p = _after_rounds(gpu, (16, 6, 1), sentinel=800, root_form="onchip")
    try:
        h, n, cap = p.h, p.n, (p.Rcap, p.Ccap)
        before = _full(p.dt, cap)
        with p.dt.clone() as twin, gpu.NodeBatch([p.dt]) as nb:
            got = nb.plunge([0], [_node()], n, 2, 2, -INF)
            want = _check_chain(got[0], p.dt, twin, h, _node(), n, 2, what="on the cut handle")
        print("chain", [(w["status"], w["events"], w["var"]) for w in want])
        assert len(want) == 2 and want[0]["events"] >= 1 and want[1]["events"] >= 1
        _dead_kept(before, _full(p.dt, cap), h.T.shape)
    finally:
        p.close()
