"""GPU checks of GMI cuts on bounded handles and of cut-and-branch at the bounded root, everything bit for bit against the
restatement (tests/_bnb_cuts_ref.py): lpx_tableau_gmi_round_bounded on solved roots that carry flips and non-zero lower shifts
(in place, with purges, purge-only, clamped by the capacity, at the block edges of the apply / carry kernels, with a fractional
upper bound on a flagged column), every bounded entry point on the reshaped handle, lpx_bounded_cut_loop in both forms, and the
driver lpx_solve_bnb_bounded9."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bnb_bounded_ref as N                  # noqa: E402
import _bnb_cuts_ref as X                     # noqa: E402
import _bounded_long_ref as L                 # noqa: E402
import _bounded_ref as B                      # noqa: E402
import _gmi_ref as G                          # noqa: E402

pytestmark = pytest.mark.gpu
LONG, CUT = L.LONG_STEP, L.CUTOFF_FLAG


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _model(name):
    if isinstance(name, str):
        return N.small_models()[name]
    n, m, seed = name
    c, A, b = N.binary_model(n, m, seed)
    return c, A, np.zeros(m, dtype=np.int32), b, np.ones(n), None, None, 0


def sentinel_handle(gpu, T, basis, Rcap, Ccap, seed):
    """A handle of capacity (Rcap, Ccap) whose whole capacity held random finite values before T went into its live window, so that
    a test can tell a write outside that window.  Returns (handle, what the capacity held)."""
    dead = np.random.default_rng(seed).uniform(-9.0, 9.0, size=(Rcap, Ccap))
    dt = gpu.DeviceTableau(Rcap, Ccap)
    dt.upload(dead)
    dt.set_shape(*T.shape)
    dt.upload(T, basis)
    return dt, dead


class Pair:
    """A device handle and the restatement's Handle in the same state: the solved root of a model, then one node whose edit
    raises a lower bound (so the handle carries flips and a non-zero lo), with `extra` spare rows and columns.  root_form: the form
    of the root solve.  sentinel (a seed): the handle is a sentinel_handle."""

    def __init__(self, gpu, name, extra, edit=True, ub_override=None, root_form="launches", sentinel=None):
        c, A, rel, b, upper, lower, mask, sense = _model(name)
        T0, basis0, ub0, _, _, _, _ = N.prepare(c, A, b, lower, upper, sense, rel)
        if ub_override:
            for j, u in ub_override.items():
                ub0[j] = u
        self.gpu, self.n, self.mask = gpu, len(c), mask
        self.T0 = T0
        R, C = T0.shape
        self.Rcap, self.Ccap, self.first = R + extra, C + extra, C - 1
        st, Ts, bs, flip, _, _ = B.run(T0, basis0, ub0)
        assert st == L.OPTIMAL
        self.h = L.Handle(Ts, bs, ub0, flip)
        if sentinel is None:
            self.dt = gpu.DeviceTableau.with_capacity(T0, basis0, self.Rcap, self.Ccap)
        else:
            self.dt, _ = sentinel_handle(gpu, T0, basis0, self.Rcap, self.Ccap, sentinel)
        self.dt.set_bounds(ub0)
        assert self.dt.bounded_run(form=root_form)[0] == L.OPTIMAL
        self.flags = X.slack_mask(T0, self.n, mask)
        if edit:
            pk = N.pick(self.h.T, self.h.basis, self.h.flip, self.h.ub, self.h.lo, self.n, mask)
            assert pk["var"] >= 0
            v = pk["var"]
            self.node([v], [np.ceil(pk["x_var"])], [ub0[v]])
            assert np.any(self.h.lo != 0.0) and np.any(self.h.flip != 0)
        self.same()

    def close(self):
        self.dt.close()

    def same(self, dt=None):
        dt = dt or self.dt
        Tg, bg = dt.download()
        lo, ub, flip = dt.bound_state()
        assert Tg.shape == self.h.T.shape
        assert np.array_equal(bg, self.h.basis)
        assert np.array_equal(_bits(Tg), _bits(self.h.T)), "tableau differs from the restatement"
        assert np.array_equal(_bits(ub), _bits(self.h.ub)) and np.array_equal(_bits(lo), _bits(self.h.lo))
        assert np.array_equal(flip, self.h.flip)

    def node(self, cols, lower, upper, flags=0, form=None, dt=None):
        """A node on both sides (dt: a clone in this pair's state instead of the pair's own handle): records compared.  Returns the
        restatement's record."""
        cols = np.asarray(cols, dtype=np.int32); lower = np.asarray(lower, dtype=np.float64); upper = np.asarray(upper, dtype=np.float64)
        self.rec = self.h.node2(cols, lower, upper, self.n, self.mask, N.EPS, L.SKIP_FIXED | flags, -np.inf)
        got = (dt or self.dt).bounded_node(cols, lower, upper, self.n, self.mask, long_step=bool(flags & LONG),
                                           cutoff=-np.inf if flags & CUT else None, form=form)
        want = self.rec
        assert got["status"] == want["status"]
        for k in ("events", "kind0", "kind1", "flips", "var", "candidates"):
            assert got[k] == want[k], k
        assert np.float64(got["z"]).view(np.uint64) == np.float64(want["z"]).view(np.uint64)
        assert np.float64(got["x_var"]).view(np.uint64) == np.float64(want["x_var"]).view(np.uint64)
        assert (dt or self.dt).trace().tolist() == self.h.trace.tolist()
        return want

    def round(self, o):
        """A bounded round on both sides: outputs and state compared.  Returns (src, pcol)."""
        self.last = X.handle_round(self.h, self.flags, len(self.flags), self.first, o, self.Rcap, self.Ccap)[:2]
        src, pcol = self.dt.gmi_round(self.flags, self.first, opts=self.gpu.CutOpts(**vars(o)).to_c(), bounded=True)
        assert list(src) == list(self.last[0]) and list(pcol) == list(self.last[1])
        self.same()
        return self.last


ROOTS = ["lowers", (16, 6, 1)]


@pytest.mark.parametrize("name", ROOTS, ids=str)
def test_round_in_place_then_with_purges_then_purge_only(gpu, name):
    p = Pair(gpu, name, 24)
    try:
        src, pcol = p.round(G.CutOpts(cuts_per_round=4))
        assert len(src) > 0 and not pcol                                # in place
        purged = 0
        for _ in range(6):                                              # rounds that purge what the re-optimisation made slack
            rec = p.node([], [], [], LONG)
            if rec["status"] != L.OPTIMAL:
                break
            src, pcol = p.round(G.CutOpts(cuts_per_round=4))
            purged += len(pcol)
            if purged and not src:
                break
        assert purged > 0, "no round purged"
        if p.rec["status"] == L.OPTIMAL and src:
            p.node([], [], [], LONG)
        src, pcol = p.round(G.CutOpts(cuts_per_round=0))                 # purge-only
        assert not src
        p.round(G.CutOpts(cuts_per_round=0, purge=0))                    # K = P = 0: nothing is touched
    finally:
        p.close()


@pytest.mark.parametrize("name", ROOTS, ids=str)
def test_capacity_clamps_k(gpu, name):
    p = Pair(gpu, name, 2)
    try:
        src, pcol = p.round(G.CutOpts(cuts_per_round=8))
        assert len(src) == 2 and not pcol
        p.node([], [], [], LONG)                                        # the handle is accepted at its full capacity
    finally:
        p.close()


@pytest.mark.parametrize("cm", [255, 256, 257])
def test_block_edges_of_apply_and_carry(gpu, cm):
    p = Pair(gpu, (cm - 3, 3, 1), 8)
    try:
        assert p.h.T.shape == (4, cm + 1)
        src, _ = p.round(G.CutOpts(cuts_per_round=3))
        assert len(src) > 0
        total = 0
        for _ in range(4):
            if p.node([], [], [], LONG)["status"] != L.OPTIMAL:
                break
            src, pcol = p.round(G.CutOpts(cuts_per_round=3))
            total += len(pcol)
        assert total > 0, "no purge at this width"
    finally:
        p.close()


def test_flagged_column_with_a_fractional_upper_bound_is_continuous(gpu):
    p = Pair(gpu, "general", 16, edit=False, ub_override={0: 2.5, 3: 2.5})
    try:
        eff = X.integer_columns(p.flags, len(p.flags), p.first, p.h.lo, p.h.ub, p.first)
        assert p.flags[0] and p.flags[3] and not eff[0] and not eff[3] and eff[1]
        src, _ = p.round(G.CutOpts(cuts_per_round=8))
        assert len(src) > 0
        p.node([], [], [], LONG)
    finally:
        p.close()


def _after_rounds(gpu, name, **kw):
    """A pair two rounds and one re-optimisation in: cut rows on the handle, bounds carried.  kw: Pair's."""
    p = Pair(gpu, name, 24, **kw)
    p.round(G.CutOpts(cuts_per_round=4))
    assert p.node([], [], [], LONG)["status"] == L.OPTIMAL
    src, _ = p.round(G.CutOpts(cuts_per_round=4))
    assert len(src) > 0
    return p


@pytest.mark.parametrize("name", ROOTS, ids=str)
def test_dual_run3_on_the_reshaped_handle(gpu, name):
    p = _after_rounds(gpu, name)
    try:
        h = p.h
        st, T, basis, flip, tr, counts = L.dual_run3(h.T, h.basis, h.ub, h.flip, L.SKIP_FIXED | LONG)
        got, _ = p.dt.bounded_dual_run(skip_fixed=True, long_step=True)
        assert got == st and p.dt.trace().tolist() == tr.tolist()
        h.T, h.basis, h.flip = T, basis, flip
        p.same()
    finally:
        p.close()


@pytest.mark.parametrize("form", ["launches", "onchip"])
@pytest.mark.parametrize("name", ROOTS, ids=str)
def test_nodes_on_the_reshaped_handle(gpu, name, form):
    """A K = 0 node; then a node whose bound edit moves a nonbasic column with entries in the cut rows, so its shift has to reach
    them; a clone of that state and a node on it; restore of the snapshot taken in front of the edit and a node from there."""
    p = _after_rounds(gpu, name)
    try:
        assert p.node([], [], [], LONG | CUT, form=form)["status"] == L.OPTIMAL
        p.same()
        h = p.h
        cut_rows = slice(p.first - p.n, h.T.shape[0] - 1)
        basic = set(h.basis.tolist())
        w = next(j for j in range(p.n) if j not in basic and h.ub[j] >= 1.0 and np.any(h.T[cut_rows, j] != 0.0))
        if h.flip[w]:                                                   # at its upper bound: lower that
            lower, upper = h.lo[w], h.lo[w] + h.ub[w] - 1.0
        else:                                                           # at its lower bound: raise that
            lower, upper = h.lo[w] + 1.0, h.lo[w] + h.ub[w]
        p.dt.snapshot()
        saved = (h.T.copy(), h.basis.copy(), h.ub.copy(), h.lo.copy(), h.flip.copy())
        p.node([w], [lower], [upper], LONG | CUT, form=form)
        p.same()
        c2 = p.dt.clone()
        try:
            p.same(c2)
            if p.rec["status"] == L.OPTIMAL:
                p.node([], [], [], LONG, form=form, dt=c2)
                p.same(c2)
        finally:
            c2.close()
        p.dt.restore()
        h.T, h.basis, h.ub, h.lo, h.flip = saved
        p.same()
        p.node([], [], [], LONG, form=form)
        p.same()
    finally:
        p.close()


@pytest.mark.parametrize("flags", [0, LONG | CUT])
@pytest.mark.parametrize("name", ROOTS + ["min", "infeasible"], ids=str)
def test_loop_in_both_forms(gpu, name, flags):
    o = G.CutOpts(cuts_per_round=4, max_rounds=4)
    recs = []
    for form in ("launches", "onchip"):
        p = Pair(gpu, name, 20, edit=isinstance(name, tuple) or name == "lowers")
        try:
            want = X.cut_loop(p.h, p.flags, len(p.flags), p.first, p.n, p.mask, o, flags, p.Rcap, p.Ccap)
            got = p.dt.cut_loop(p.flags, p.first, p.n, p.mask, opts=gpu.CutOpts(**vars(o)).to_c(), long_step=bool(flags & LONG),
                                cutoff=bool(flags & CUT), form=form)
            for k in ("rounds", "added", "purged", "events", "stop", "status", "R", "C", "var", "candidates"):
                assert got[k] == want[k], k
            assert np.array_equal(_bits(got["z_before"]), _bits(want["z_before"]))
            assert np.array_equal(_bits(got["z_after"]), _bits(want["z_after"]))
            assert np.float64(got["z"]).view(np.uint64) == np.float64(want["z"]).view(np.uint64)
            assert all(a >= b for a, b in zip(want["z_before"], want["z_after"]))
            p.same()
            recs.append({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in got.items()})
        finally:
            p.close()
    assert recs[0] == recs[1]
    if name == "infeasible":
        assert recs[0]["stop"] == "infeasible" and recs[0]["rounds"] == 1


# ---- the driver: lpx_solve_bnb_bounded9 through LPSolver.SolveBnbBounded(root_cuts=...) ---------------------------------------
DRIVER_MODELS = sorted(N.small_models()) + [(24, 8, 2), (40, 16, 6)]
COUNTERS = ("nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K", "rounds", "steals", "largest_batch")


def _problem(gpu, name):
    c, A, rel, b, upper, lower, mask, sense = _model(name)
    return gpu.LPProblem.from_arrays(sense, c, A, rel, b), dict(upper=upper, lower=lower, integer=mask)


def _reference(name, W, flags, o):
    c, A, rel, b, upper, lower, mask, sense = _model(name)
    return X.solve_cuts(c, A, b, upper, W, o, lower=lower, is_int=mask, sense=sense, rel=rel, search_flags=flags)


def _same_search(res, want):
    assert res.Status == want["status"]
    assert res.BnbLog.tobytes() == want["log"].tobytes(), "node log differs from the restatement"
    for k in COUNTERS:
        assert res.BnbInfo[k] == want[k], k
    assert res.BnbRound.tolist() == want["round"].tolist() and res.BnbDiver.tolist() == want["diver"].tolist()
    if want["status"] == L.OPTIMAL:
        assert np.array_equal(_bits(res.Solution), _bits(want["x"]))
        assert np.float64(res.OptimalValue).view(np.uint64) == np.float64(want["value"]).view(np.uint64)
    else:
        assert res.Nodes == want["nodes"]


def _same_cuts(res, cut):
    bi = res.BnbInfo
    assert (bi["cut_ran"], bi["cut_spare"]) == (cut["ran"], cut["spare"])
    if not cut["ran"]:
        assert bi["cut_rounds"] == bi["cuts_added"] == bi["cuts_purged"] == 0 and res.CutZ.shape == (0, 2)
        return
    assert (bi["cut_rounds"], bi["cuts_added"], bi["cuts_purged"], bi["cut_events"], bi["cut_stop"], bi["cut_R"], bi["cut_C"]) == \
           (cut["rounds"], cut["added"], cut["purged"], cut["events"], cut["stop"], cut["R"], cut["C"])
    assert np.array_equal(_bits(res.CutZ[:, 0]), _bits(cut["z_before"])) and np.array_equal(_bits(res.CutZ[:, 1]), _bits(cut["z_after"]))


@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("name", DRIVER_MODELS, ids=str)
def test_driver_with_root_cuts(gpu, name, W):
    o = G.CutOpts(cuts_per_round=8, max_rounds=4)
    want = _reference(name, W, LONG | CUT, o)
    prob, kw = _problem(gpu, name)
    res = gpu.LPSolver().SolveBnbBounded(prob, long_step=True, cutoff=True, divers=W, root_cuts=4, cuts_per_round=8, **kw)
    print(name, W, "nodes", res.Nodes, "cuts", res.BnbInfo["cuts_added"], res.BnbInfo["cut_stop"], res.BnbInfo["cut_R"], res.BnbInfo["cut_C"])
    _same_search(res, want)
    _same_cuts(res, want["cut"])
    assert want["cut"]["ran"] == 1
    if name == "infeasible":
        assert res.Status == L.INFEASIBLE and res.Nodes == 0 and res.BnbInfo["cut_stop"] == "infeasible" and res.BnbInfo["cut_rounds"] == 1


@pytest.mark.parametrize("W", [1, 4])
def test_driver_without_root_cuts_is_bounded8(gpu, W):
    """root_cuts = NULL through the C ABI: the log, the counters and the result of lpx_solve_bnb_bounded8, bit for bit."""
    import ctypes as C
    from linear_programming_solver_lpr381_amd import _lib, solver as S
    prob, kw = _problem(gpu, (24, 8, 2))
    base = gpu.LPSolver().SolveBnbBounded(prob, long_step=True, cutoff=True, divers=W, root_form="launches", **kw)
    n = prob.NumVars
    o, keep = S._solve_opts({})
    ps, hold = S._problem_struct(prob)
    up = np.ascontiguousarray(kw["upper"], dtype=np.float64)
    r, info, dinfo, ginfo, cinfo = _lib.Result(), _lib.BnbBoundedInfo(), _lib.BnbDiversInfo(), _lib.BnbGuardInfo(), _lib.BnbCutInfo()
    rc = _lib.lib().lpx_solve_bnb_bounded9(C.byref(ps), None, up.ctypes.data_as(_lib.dp), None, C.byref(o), 0,
                                           _lib.BDUAL_LONG_STEP | _lib.BDUAL_CUTOFF, W, 0, _lib.NODE_LAUNCHES, None, C.byref(r),
                                           C.byref(info), C.byref(dinfo), C.byref(ginfo), C.byref(cinfo))
    try:
        assert rc == 0 and info.n_log == len(base.BnbLog) > 0
        assert C.string_at(info.log, info.n_log * C.sizeof(_lib.BnbNodeLog)) == base.BnbLog.tobytes()
        for k in ("nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K"):
            assert getattr(info, k) == base.BnbInfo[k], k
        assert (dinfo.rounds, dinfo.steals, dinfo.largest_batch) == tuple(base.BnbInfo[k] for k in ("rounds", "steals", "largest_batch"))
        assert (cinfo.ran, cinfo.spare, cinfo.rounds, cinfo.n_z) == (0, 0, 0, 0)
        assert r.optimal_value == base.OptimalValue
        assert np.array_equal(_bits(np.ctypeslib.as_array(r.x, (n,))), _bits(base.Solution))
    finally:
        _lib.lib().lpx_bnb_bounded_info_free(C.byref(info)); _lib.lib().lpx_bnb_divers_info_free(C.byref(dinfo))
        _lib.lib().lpx_bnb_cut_info_free(C.byref(cinfo)); _lib.lib().lpx_result_free(C.byref(r))


def test_driver_on_a_shape_that_just_fits_runs_no_round(gpu):
    """4 x 3004 fits the on-chip node and 5 x 3005 does not: a = 0, no round, and the search of the driver without cuts."""
    name = (3000, 3, 1)
    assert X.node_fits(4, 3004) and not X.node_fits(5, 3005)
    c, A, rel, b, upper, lower, mask, sense = _model(name)
    o = G.CutOpts(cuts_per_round=8, max_rounds=4)
    want = X.solve_cuts(c, A, b, upper, 4, o, search_flags=LONG | CUT, max_nodes=24)
    assert want["cut"] == {"spare": 0, "ran": 0}
    prob, kw = _problem(gpu, name)
    try:
        res = gpu.LPSolver().SolveBnbBounded(prob, long_step=True, cutoff=True, divers=4, root_cuts=4, max_nodes=24, **kw)
    except gpu.SolverException as e:
        assert e.code == gpu._lib.ITER_LIMIT and want["rc"] == L.ITER_LIMIT
        res = e.result
    else:
        assert want["rc"] == 0
    assert res.BnbLog.tobytes() == want["log"].tobytes() and len(want["log"]) > 0
    for k in COUNTERS:
        assert res.BnbInfo[k] == want[k], k
    _same_cuts(res, want["cut"])
