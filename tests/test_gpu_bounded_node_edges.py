"""GPU tests of the on-chip node (csrc/lpx_bounded_node_body.h, the text of lpx_bounded_node_onchip and lpx_bounded_nodes_onchip)
at the edges its other tests do not reach: the ordered list of the dual-feasibility flips across waves and 1024-column blocks (A),
bound edits of up to 1025 triples in both orders, their refusals and the regrowth of the staging buffers (B), the pick inside
the kernel across waves and 1024-strides (C), the largest shapes the fit rule admits (D), wide rows with tied ratios (E), and all
of these as entries of a batch (F).  Everything is compared bit for bit -- record, trace, tableau, basis, flip, ub, lo, counts --
with the NumPy restatement (tests/_bounded_long_ref.py) and with a second device handle on the launches form.  A case that the
restatement shows to be vacuous (no flips where the flips are the subject, no events where the loop is) fails its condition."""
import functools

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bounded_dual_ref as D
import _bounded_long_ref as L
import _node_helpers as H
from _node_helpers import INF, LONG, SKIP

pytestmark = pytest.mark.gpu

FLAGS = [0, LONG]
LDS_LIMIT = 160 * 1024 - 2048          # the fit rule: the LDS of one compute unit less the reserve for the kernel's statics


def _lds_bytes(R, C):
    return 8 * (R * (C | 1) + C + max(R, C))


def _copy(h):
    c = L.Handle(h.T, h.basis, h.ub, h.flip, h.lo)
    c.trace = h.trace
    return c


def _with_pick(rec, h, nint, is_int=None):
    """The record of a reference node with the pick taken over the first nint columns (the pick does not change the handle)."""
    out = dict(rec)
    if rec["status"] == L.OPTIMAL:
        out.update(N.pick(h.T, h.basis, h.flip, h.ub, h.lo, nint, is_int))
    return out


def _same_node(dt, got, want, h, what=""):
    H.same_record(got, want)
    assert dt.trace().tolist() == h.trace.tolist(), what
    H.same_state(dt, h, what)
    assert dt.bounded_counts() == (want["kind0"], want["kind1"], want["events"] - want["kind0"] - want["kind1"]), what


def _both_forms(dt, other, nd, nint, flags, want, h, what="", **kw):
    """The node on chip on dt against the reference (want, h), and on the launches form on `other`: the same bits."""
    got = dt.bounded_node(*nd, nint, long_step=bool(flags), form="onchip", **kw)
    _same_node(dt, got, want, h, what)
    ref = other.bounded_node(*nd, nint, long_step=bool(flags), form="launches", **kw)
    H.same_record(got, ref)
    assert dt.trace().tolist() == other.trace().tolist() and H.state(dt) == H.state(other), what
    assert dt.bounded_counts() == other.bounded_counts(), what
    return got


def _batch_entry(dt, twin, got, nd, nint, flags, want, h, what, **kw):
    """An entry of a batch against the reference and against the single-node form on a twin handle."""
    _same_node(dt, got, want, h, what)
    ref = twin.bounded_node(*nd, nint, long_step=bool(flags), form="onchip", **kw)
    H.same_record(got, ref)
    assert H.reads(dt, nint) == H.reads(twin, nint), what + ": differs from its twin on the single-node form"


# ---- the instances ----------------------------------------------------------------------------------------------------------
def _integer_covering(m, n, seed):
    """The covering construction with A in 0..3 and c in 1..4, 20 % of the columns fixed: many dual ratios are equal."""
    from linear_programming_solver_lpr381_amd import synth
    g = np.random.default_rng(seed)
    A = g.integers(0, 4, size=(m, n)).astype(np.float64)
    c = g.integers(1, 5, size=n).astype(np.float64)
    b = np.floor(A.sum(axis=1) * g.uniform(0.2, 0.5, size=m))
    T, basis = synth.primal_tableau_from(-c, -A, -b)
    ub = np.full(T.shape[1] - 1, INF)
    ub[:n] = 1.0
    ub[:n][g.random(n) < 0.2] = 0.0
    return T, basis, ub


PATTERNS = ("empty", "first", "last", "63_64", "1023_1024", "lane0", "all", "r10", "r50")


def _pattern(name, n):
    """The structural columns that get a negative reduced cost; None where the shape does not have them."""
    if name == "empty":
        return np.zeros(0, dtype=np.int64)
    if name == "first":
        return np.array([0])
    if name == "last":                                  # the last structural column that is not fixed
        return np.array([max(j for j in range(n) if H.covering_fixed(n, 1)[j] == 0)])
    if name == "63_64":
        return np.array([63, 64]) if n > 64 else None
    if name == "1023_1024":
        return np.array([1023, 1024]) if n > 1024 else None
    if name == "lane0":
        return np.arange(0, n, 64)
    if name == "all":
        return np.arange(n)
    g = np.random.default_rng(1000 + n)
    return np.flatnonzero(g.random(n) < (0.1 if name == "r10" else 0.5))


def _planted(m, n, J, seed=1, integer=False):
    T, basis, ub = _integer_covering(m, n, seed) if integer else H.covering_with_fixed(m, n, seed)
    J = np.asarray(J, dtype=np.int64)
    T[m, J] = -np.abs(T[m, J]) - 0.5
    return T, basis, ub


@functools.lru_cache(maxsize=None)
def _ref(m, n, pattern, flags, integer=False, max_iter=10000):
    """The K = 0 node of a planted covering tableau in the restatement, once: (T, basis, ub, J, record with nint = n, handle).
    Shared by the single-node and the batch tests; nobody writes to what it returns."""
    J = _pattern(pattern, n)
    T, basis, ub = _planted(m, n, J, integer=integer)
    h = H.slack_handle(T, basis, ub)
    rec = H.ref_node(h, H.node(), n, flags, max_iter=max_iter)
    return T, basis, ub, J, rec, h


def _listed(ub, J):
    return [int(j) for j in J if 0.0 < ub[j] < INF]


# ---- A. flips on chip at every list edge (K = 0) ----------------------------------------------------------------------------
A_SHAPES = {(8, 55): (9, 64), (8, 56): (9, 65), (8, 57): (9, 66), (8, 1015): (9, 1024), (8, 1016): (9, 1025), (8, 1017): (9, 1026),
            (4, 2100): (5, 2105), (1, 5000): (2, 5002), (63, 190): (64, 254)}
A_CASES = [(m, n, p) for (m, n) in sorted(A_SHAPES) for p in PATTERNS if _pattern(p, n) is not None]
A_WITH_EVENTS = ("empty", "first", "last", "r10")      # the patterns that leave the dual loop work to do, on every shape
A_THREE_BLOCKS = [(4, 2100, "r10"), (4, 2100, "r50"), (1, 5000, "lane0"), (1, 5000, "r10")]


def _a_conditions(m, n, pattern, flags):
    T, basis, ub, J, rec, h = _ref(m, n, pattern, flags)
    assert T.shape == A_SHAPES[(m, n)]
    listed = _listed(ub, J)
    assert rec["status"] is not None and rec["flips"] == len(listed), "fixed columns are left alone, every other planted one is flipped"
    assert len(J) == 0 or rec["flips"] > 0, "pattern %s plants only fixed columns on %d x %d: the case shows nothing" % ((pattern,) + T.shape)
    if pattern in A_WITH_EVENTS:
        assert rec["events"] > 0, "no event after the flips of %s on %d x %d: the loop is not reached" % ((pattern,) + T.shape)
    if (m, n, pattern) in A_THREE_BLOCKS:
        assert len({j // 1024 for j in listed}) >= 3, "the listed columns do not span three 1024-blocks"
    return T, basis, ub, rec, h


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("m,n,pattern", A_CASES)
def test_flips_at_every_list_edge(gpu, m, n, pattern, flags):
    T, basis, ub, rec, h = _a_conditions(m, n, pattern, flags)
    assert gpu._lib.lib().lpx_bounded_node_fits(*T.shape) == 1
    with H.fresh(gpu, T, basis, ub) as dt, H.fresh(gpu, T, basis, ub) as other:
        got = _both_forms(dt, other, H.node(), n, flags, rec, h)
    assert got["flips"] == rec["flips"]


def test_family_a_has_a_case_with_events_on_every_shape_and_one_over_three_blocks():
    assert {(m, n) for m, n, p in A_CASES if p in A_WITH_EVENTS} == set(A_SHAPES)
    assert all(c in A_CASES for c in A_THREE_BLOCKS)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("bad", [(1023,), (1024,), (70, 1500, 2000)])
def test_unrepairable_columns_in_every_block_are_refused(gpu, bad, flags):
    m, n = 4, 2100
    J = _pattern("r10", n)
    T, basis, ub = _planted(m, n, np.union1d(J, bad))
    ub[list(bad)] = INF                                                 # a negative reduced cost and no upper bound
    listed = _listed(ub, J)
    h = H.slack_handle(T, basis, ub)
    want = H.ref_node(h, H.node(), n, flags)
    assert want["status"] is None and want["unrepairable"] == len(bad) and want["flips"] == 0 and len(listed) > 0
    with H.fresh(gpu, T, basis, ub) as dt, H.fresh(gpu, T, basis, ub) as other:
        before = H.state(dt)
        with pytest.raises(gpu.LpxError) as e:
            dt.bounded_node([], [], [], n, long_step=bool(flags), form="onchip")
        assert e.value.code == gpu._lib.EINVAL and "lpx_bounded_node3: %d column(s)" % len(bad) in str(e.value) and "no upper bound" in str(e.value)
        assert H.state(dt) == before, "the refused node changed the handle"
        nd = H.node(sorted(bad), [0.0] * len(bad), [1.0] * len(bad))    # a valid node follows: the columns get the bound 1
        want = H.ref_node(h, nd, n, flags)
        assert want["status"] is not None and want["flips"] == len(listed) + len(bad), "the columns that got a bound are flipped with the rest"
        _both_forms(dt, other, nd, n, flags, want, h)
        assert all(h.flip[j] or j in h.basis for j in bad)


# ---- B. bound edits at every K edge -----------------------------------------------------------------------------------------
BM, BN = 8, 1828                                # 9 x 1837: the widest slack-basis shape with 9 rows that fits
B_KS = [(1, False), (63, False), (64, False), (65, False), (1023, False), (1024, False), (1025, False), (65, True), (1025, True)]


def _edit(h, n, K, seed, shuffled=False):
    """One edit of K distinct structural columns of the handle h, by a seeded choice: fix at 0, fix at 1, tighten to [0, 0.5], the
    lower shift [0.25, 1], re-open a fixed column to [0, 1], an unchanged pair, upper = +inf on an unflipped column whose reduced
    cost is not negative.  A flipped column is always among them, a fixed column with a negative reduced cost from K = 2 on, and
    at least one lower bound is not zero.  Ascending unless shuffled."""
    g = np.random.default_rng(seed)
    cost = h.T[-1, :n]
    flipped = np.flatnonzero(h.flip[:n])
    fixed_neg = np.flatnonzero((h.ub[:n] == 0.0) & (cost < -1e-9))
    assert len(flipped) > 0 and len(fixed_neg) > 0, "the handle has no flipped column or no fixed column with a negative cost"
    must = [int(flipped[g.integers(len(flipped))])] + ([int(fixed_neg[g.integers(len(fixed_neg))])] if K >= 2 else [])
    rest = g.permutation(np.setdiff1d(np.arange(n), must))[:K - len(must)]
    cols = np.sort(np.concatenate([np.array(must, dtype=np.int64), rest]))
    if shuffled:
        cols = g.permutation(cols)
    lower, upper, ops = np.zeros(K), np.zeros(K), []
    for k, j in enumerate(cols):
        if h.flip[j]:
            choice = ["fix0", "fix1", "tight", "lower", "same"]
        elif h.ub[j] == 0.0:
            choice = ["reopen", "reopen", "same", "fix1"] + (["inf"] if cost[j] >= 0.0 else [])
        else:
            choice = ["fix0", "fix1", "tight", "lower", "same", "same"] + (["inf"] if cost[j] >= 0.0 and h.ub[j] < INF else [])
        op = "reopen" if j in must[1:] else str(g.choice(choice))
        ops.append(op)
    if not any(op in ("fix1", "lower") for op in ops):
        ops[int(np.flatnonzero(cols == must[0])[0])] = "lower"
    for k, (j, op) in enumerate(zip(cols, ops)):
        lower[k], upper[k] = {"fix0": (0.0, 0.0), "fix1": (1.0, 1.0), "tight": (0.0, 0.5), "lower": (0.25, 1.0), "reopen": (0.0, 1.0),
                              "same": (h.lo[j], h.lo[j] + h.ub[j]), "inf": (0.0, INF)}[op]
    return H.node(cols, lower, upper), ops


@functools.lru_cache(maxsize=None)
def _ref_b(K, shuffled, flags):
    """The family's edit of K columns on the handle the K = 0 node of the r10 pattern left: (node, ops, record, handle after)."""
    h = _copy(_ref(BM, BN, "r10", flags)[5])
    nd, ops = _edit(h, BN, K, 7 * K + shuffled, shuffled)
    flipped_edited = int(h.flip[nd[0]].sum())
    rec = H.ref_node(h, nd, BN, flags)
    assert rec["status"] is not None, "the seeded edit is refused"
    assert flipped_edited > 0 and np.any(nd[1] != 0.0), "no flipped column among the edited ones, or no non-zero lower bound"
    return nd, ops, rec, h


def _b_handles(gpu, pool, flags, count=2):
    """Device handles in the state behind the K = 0 node of the r10 pattern (checked against the restatement), snapshot taken."""
    T, basis, ub, J, rec, h = _ref(BM, BN, "r10", flags)
    assert T.shape == (9, 1837) and rec["flips"] > 0 and rec["events"] > 0
    out = []
    for i in range(count):
        dt = pool.add(H.fresh(gpu, T, basis, ub))
        got = dt.bounded_node([], [], [], BN, long_step=bool(flags), form="onchip" if i == 0 else "launches")
        _same_node(dt, got, rec, h, "the K = 0 node in front of the edit")
        dt.snapshot()
        out.append(dt)
    return out


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("K,shuffled", B_KS)
def test_bound_edit_at_every_k_edge(gpu, K, shuffled, flags):
    nd, ops, rec, h = _ref_b(K, shuffled, flags)
    assert len(nd[0]) == K and len(set(nd[0].tolist())) == K
    assert shuffled == bool(np.any(np.diff(nd[0]) < 0)) or K == 1
    if K >= 63:                                                     # K = 1 is the edit whose only shift is zero
        assert rec["status"] == L.OPTIMAL and rec["events"] > 0, "the edit of %d columns leaves the loop nothing to do, or no optimum" % K
        assert rec["flips"] > 0, "no flip after the edit of %d columns: re-opened columns with a negative cost are not listed" % K
        assert {"fix0", "fix1", "tight", "lower", "reopen", "same", "inf"} <= set(ops), "the mix misses an operation"
    with H.Pool() as pool:
        dt, other = _b_handles(gpu, pool, flags)
        _both_forms(dt, other, nd, BN, flags, rec, h, "K = %d" % K)


@pytest.mark.parametrize("flags", FLAGS)
def test_refusals_of_large_edits_leave_the_handle_alone(gpu, flags):
    h0 = _ref(BM, BN, "r10", flags)[5]
    (cols, lower, upper), _ = _edit(h0, BN, 1031, 99)
    outside = [int(j) for j in np.flatnonzero(h0.flip[:BN]) if j not in set(cols.tolist())]
    assert len(outside) >= 2
    with H.Pool() as pool:
        dt, other = _b_handles(gpu, pool, flags)
        before = H.state(dt)
        # upper = +inf on a flipped column at k = 1024 alone, and at k = 1024 and 1030: the lowest k is named
        for K, ks in ((1025, (1024,)), (1031, (1024, 1030))):
            c, lw, up = cols[:K].copy(), lower[:K].copy(), upper[:K].copy()
            for i, k in enumerate(ks):
                c[k], lw[k], up[k] = outside[i], 0.0, INF
            for handle, form in ((dt, "onchip"), (other, "launches")):
                with pytest.raises(gpu.LpxError) as e:
                    handle.bounded_node(c, lw, up, BN, long_step=bool(flags), form=form)
                assert e.value.code == gpu._lib.EINVAL and "lpx_bounded_node3: upper[1024] = +inf on a flipped column" in str(e.value)
                assert H.state(handle) == before
        # 1025 triples of which one re-opens a fixed column with a negative reduced cost to [0, +inf]: ub and lo of all are put back
        (c, lw, up), _ = _edit(h0, BN, 1025, 98)
        k = [k for k, j in enumerate(c) if h0.ub[j] == 0.0 and h0.T[-1, j] < -1e-9][-1]
        lw[k], up[k] = 0.0, INF
        h = _copy(h0)
        want = H.ref_node(h, (c, lw, up), BN, flags)
        assert want["status"] is None and want["unrepairable"] == 1
        assert np.count_nonzero((lw != h0.lo[c]) | (up - lw != h0.ub[c])) > 500, "the edit changes too few bounds to show the restore"
        with pytest.raises(gpu.LpxError) as e:
            dt.bounded_node(c, lw, up, BN, long_step=bool(flags), form="onchip")
        assert "lpx_bounded_node3: 1 column(s)" in str(e.value) and "no upper bound" in str(e.value)
        assert H.state(dt) == before, "ub or lo of a refused edit of 1025 columns were not restored"
        nd, _, rec, h = _ref_b(1025, False, flags)                       # the handle takes the family's node afterwards
        _both_forms(dt, other, nd, BN, flags, rec, h)


@pytest.mark.parametrize("flags", FLAGS)
def test_staging_buffers_regrow_from_both_forms(gpu, flags):
    T, basis, ub, J, rec, h0 = _ref(BM, BN, "r10", flags)
    h = H.slack_handle(T, basis, ub)
    with H.fresh(gpu, T, basis, ub) as dt:
        for step, (K, form) in enumerate(((0, "launches"), (2, "onchip"), (1025, "onchip"), (3, "launches"), (1025, "onchip"))):
            nd = H.node() if K == 0 else _edit(h, BN, K, 40 + step)[0]
            got, want = H.node3(dt, h, *nd, BN, flags, form=form)
            assert want["status"] is not None and (step > 0 or want["flips"] > 0)


# ---- C. the pick inside the kernel ------------------------------------------------------------------------------------------
TIES = [({70: 2.75, 1500: 1.25}, 70, 4000),             # equal distance in different waves and different 1024-lane strides
        ({5: 0.75, 1029: 0.25}, 5, 4000),               # the same lane, two strides
        ({7: 0.75, 1030: 0.25}, 7, 4000),               # the lower index sits in the higher lane
        ({1030: 0.25, 2055: 0.75, 3000: 0.125}, 1030, 3100),   # a farther candidate behind the tie; four rows fit up to 3 400 columns
        ({63: 0.25, 64: 0.75}, 63, 4000),               # across a wave edge
        ({3999: 0.4}, 3999, 4000)]                      # a candidate only at the last index


def _tie_case(gpu, entries, nint):
    T, basis, ub = H.exact(nint, entries)
    assert T.shape[0] <= 4 and gpu._lib.lib().lpx_bounded_node_fits(*T.shape) == 1
    return T, basis, ub


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("entries,winner,nint", TIES)
def test_pick_ties_on_chip_go_to_the_lowest_index(gpu, entries, winner, nint, flags):
    T, basis, ub = _tie_case(gpu, entries, nint)
    h = H.slack_handle(T, basis, ub)
    with H.fresh(gpu, T, basis, ub) as dt, H.fresh(gpu, T, basis, ub) as other:
        want = H.ref_node(h, H.node(), nint, flags)
        assert want["status"] == L.OPTIMAL and want["events"] == 0 and want["flips"] == 0
        got = _both_forms(dt, other, H.node(), nint, flags, want, h)
        assert got["var"] == winner and got["candidates"] == len(entries) and got["x_var"] == entries[winner]
        want = H.ref_node(h, H.node(), 0, flags)                       # nint = 0
        got = _both_forms(dt, other, H.node(), 0, flags, want, h)
        assert got["var"] == -1 and got["candidates"] == 0


PICK_CM = 1836                                      # nint = Cm on 9 x 1837, the widest fitting shape with 9 rows
PICK_NINT = [1, 63, 64, 65, 1023, 1024, 1025, PICK_CM]


def _pick_case(nint, seed):
    """pick_tableau with 8 rows whose node is OPTIMAL without an event: every RHS inside [0, ub] of its basic column.  A third of
    the nonbasic bounded columns get a fractional bound and a negative reduced cost, so the node flips them and they stand at
    that bound: candidates, and ties among them, over the whole range of the pick."""
    T, basis, ub = H.pick_tableau(nint, 8, seed, extra=0 if nint == PICK_CM else 3)
    m, Cm = T.shape[0] - 1, T.shape[1] - 1
    T[:m, Cm] = np.minimum(T[:m, Cm], ub[basis])
    g = np.random.default_rng(seed + 1)
    nonbasic = np.ones(Cm, dtype=bool); nonbasic[basis] = False
    J = np.flatnonzero(nonbasic & (ub < INF) & (g.random(Cm) < 1.0 / 3.0))
    ub[J] = g.choice(np.array([0.5, 1.5, 2.25, 2.75, 1.125, 3.0]), size=len(J))
    T[m, J] = -1.0
    return T, basis, ub, J


def _pick_steps(nint, T, basis, ub, h):
    """The nodes of one pick case, in order, with their reference records: plain, a half mask that removes the plain winner, an
    all-zero mask, and a K-edit that puts the lower bound 1 on every 7th column that is not basic."""
    steps = []
    want = H.ref_node(h, H.node(), nint, 0)
    steps.append((H.node(), None, want))
    g = np.random.default_rng(nint)
    mask = (g.random(nint) < 0.5).astype(np.uint8)
    if want["var"] >= 0:
        mask[want["var"]] = 0
    for is_int in (mask, np.zeros(nint, dtype=np.uint8)):
        steps.append((H.node(), is_int, h.node2(*H.node(), nint, is_int=is_int)))
    basic = set(h.basis.tolist())
    cols = np.array([j for j in range(0, nint, 7) if j not in basic], dtype=np.int32)
    nd = H.node(cols, np.ones(len(cols)), 1.0 + np.where(np.isinf(ub[cols]), 5.0, ub[cols]))
    steps.append((nd, None, h.node2(*nd, nint)))
    return steps


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("nint", PICK_NINT)
def test_pick_on_chip_at_every_edge(gpu, nint, flags):
    T, basis, ub, J = _pick_case(nint, nint)
    assert gpu._lib.lib().lpx_bounded_node_fits(*T.shape) == 1
    with H.fresh(gpu, T, basis, ub) as dt, H.fresh(gpu, T, basis, ub) as other:
        h, href = H.slack_handle(T, basis, ub), H.slack_handle(T, basis, ub)
        plain = None
        for step, (nd, is_int, _) in enumerate(_pick_steps(nint, T, basis, ub, href)):
            got, want = H.node3(dt, h, *nd, nint, flags, other=other, is_int=is_int)
            assert want["status"] == L.OPTIMAL and want["events"] == 0, "the node is not optimal as it stands: the pick is not all that runs"
            if step == 0:
                plain = want
                assert want["flips"] == len(J) and (nint < 63 or want["candidates"] > 8), "no candidate beyond the basic columns"
            elif step == 1 and plain["var"] >= 0:
                assert want["var"] != plain["var"] and want["candidates"] < plain["candidates"] and (nint < 63 or want["candidates"] > 0)
            elif step == 2:
                assert want["var"] == -1 and want["candidates"] == 0
            elif step == 3 and len(nd[0]):
                assert np.all(h.lo[nd[0]] == 1.0) and want["candidates"] == plain["candidates"]
        if nint > 1024:                                                  # ties across the 1024-strides: the lowest index wins
            x = N.values(h.T, h.basis, h.flip, h.ub, h.lo, nint)
            f = x - np.floor(x)
            assert np.count_nonzero(np.abs(f - 0.5) == abs(f[plain["var"]] - 0.5)) > 1 and plain["var"] < 1024


# ---- D. the fit boundary ----------------------------------------------------------------------------------------------------
# (m, n): R x C, the dynamic LDS of the shape; R x (C + 1) is refused
D_SHAPES = {(1, 5053): ((2, 5055), 161760), (8, 1828): ((9, 1837), 161656), (64, 236): ((65, 301), 161336), (139, 1): ((140, 141), 160176)}
D_FLIP_PATTERN = {(1, 5053): "r10", (8, 1828): "r10", (64, 236): "r10", (139, 1): "all"}


def test_fit_rule_at_its_boundary(gpu):
    fits = gpu._lib.lib().lpx_bounded_node_fits
    assert LDS_LIMIT == 161792
    for (m, n), ((R, C), lds) in D_SHAPES.items():
        assert (R, C) == (m + 1, n + m + 1) and _lds_bytes(R, C) == lds <= LDS_LIMIT < _lds_bytes(R, C + 1)
        assert fits(R, C) == 1 and fits(R, C + 1) == 0, (R, C)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("pattern", ["empty", "flips"])
@pytest.mark.parametrize("m,n", sorted(D_SHAPES))
def test_node_at_the_fit_boundary(gpu, m, n, pattern, flags):
    T, basis, ub, J, rec, h = _ref(m, n, "empty" if pattern == "empty" else D_FLIP_PATTERN[(m, n)], flags)
    assert T.shape == D_SHAPES[(m, n)][0]
    if pattern == "empty":
        assert rec["events"] > 0, "the covering node has nothing to do on %d x %d" % T.shape
    else:
        assert rec["flips"] > 0, "no flip on %d x %d" % T.shape
    with H.fresh(gpu, T, basis, ub) as dt, H.fresh(gpu, T, basis, ub) as other:
        assert dt.bounded_node_fits()
        _both_forms(dt, other, H.node(), n, flags, rec, h)


@pytest.mark.parametrize("m,n", sorted(D_SHAPES))
def test_one_column_more_does_not_fit(gpu, m, n):
    T, basis, ub = H.covering_with_fixed(m, n + 1, 1)
    assert T.shape == (D_SHAPES[(m, n)][0][0], D_SHAPES[(m, n)][0][1] + 1)
    with H.fresh(gpu, T, basis, ub) as dt, H.fresh(gpu, T, basis, ub) as other:
        assert not dt.bounded_node_fits()
        before = H.state(dt)
        with pytest.raises(gpu.LpxError) as e:
            dt.bounded_node([], [], [], n + 1, form="onchip")
        assert e.value.code == gpu._lib.EINVAL and "does not fit" in str(e.value)
        assert H.state(dt) == before
        dt.snapshot(); other.snapshot()
        for flags in FLAGS:
            dt.restore(); other.restore()
            H.node3(dt, H.slack_handle(T, basis, ub), [], [], [], n + 1, flags, form="auto", other=other, max_iter=12)


# ---- E. wide rows with tied ratios ------------------------------------------------------------------------------------------
E_SHAPES = {(4, 2100): (5, 2105), (8, 1017): (9, 1026)}


def _counting_hysteresis(calls, plain):
    """An instrumented copy of the restatement's sequential scan: it also records whether the accepted ratio is met twice."""
    def scan(rho, tol):
        best, k = INF, -1
        for j in np.flatnonzero(rho < INF):
            if rho[j] < best - tol:
                best, k = rho[j], int(j)
        assert k == plain(rho, tol)
        calls.append(k >= 0 and int(np.count_nonzero(rho == rho[k])) > 1)
        return k
    return scan


@functools.lru_cache(maxsize=None)
def _ref_e(m, n, flags):
    calls = []
    plain = D._hysteresis
    D._hysteresis = _counting_hysteresis(calls, plain)
    try:
        out = _ref(m, n, "r10", flags, True, 500)
    finally:
        D._hysteresis = plain
    return out, sum(calls)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("m,n", sorted(E_SHAPES))
def test_wide_rows_with_tied_ratios(gpu, m, n, flags):
    (T, basis, ub, J, rec, h), tied = _ref_e(m, n, flags)
    assert T.shape == E_SHAPES[(m, n)] and np.array_equal(T[:m], np.rint(T[:m]))
    assert tied > 0, "no selection of the run has two equal least ratios"
    assert rec["events"] > 0 and rec["flips"] > 0
    if not flags:                                                       # the long step replaces them by passes on the wider shape
        assert rec["kind1"] > 0, "no kind-1 event on %d x %d" % T.shape
    with H.fresh(gpu, T, basis, ub) as dt, H.fresh(gpu, T, basis, ub) as other:
        _both_forms(dt, other, H.node(), n, flags, rec, h, max_iter=500)


# ---- F. the batch -----------------------------------------------------------------------------------------------------------
def _run_k0_batch(gpu, cases, nint, flags, **kw):
    """K = 0 entries (T, basis, ub, record, handle) in one launch, each against the reference and its twin."""
    with H.Pool() as pool:
        hs = [pool.add(H.fresh(gpu, c[0], c[1], c[2])) for c in cases]
        twins = [pool.add(H.fresh(gpu, c[0], c[1], c[2])) for c in cases]
        with gpu.NodeBatch(hs) as nb:
            got = nb.run(list(range(len(cases))), [H.node()] * len(cases), nint, long_step=bool(flags), **kw)
        for i, (T, basis, ub, rec, h) in enumerate(cases):
            _batch_entry(hs[i], twins[i], got[i], H.node(), nint, flags, _with_pick(rec, h, nint), h, "entry %d" % i, **kw)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("m,n", sorted(A_SHAPES))
def test_batch_of_the_flip_patterns_of_a_shape(gpu, m, n, flags):
    cases = [_a_conditions(m, n, p, flags) for mm, nn, p in A_CASES if (mm, nn) == (m, n)]
    _run_k0_batch(gpu, cases, n, flags)


@pytest.mark.parametrize("flags", FLAGS)
def test_batch_of_the_edits_at_every_k_edge(gpu, flags):
    with H.Pool() as pool:
        src, twin_src = _b_handles(gpu, pool, flags)
        hs = [pool.add(src.clone()) for _ in B_KS]
        twins = [pool.add(twin_src.clone()) for _ in B_KS]
        refs = [_ref_b(K, shuffled, flags) for K, shuffled in B_KS]
        with gpu.NodeBatch(hs) as nb:
            got = nb.run(list(range(len(hs))), [r[0] for r in refs], BN, long_step=bool(flags))
        for i, (nd, ops, rec, h) in enumerate(refs):
            _batch_entry(hs[i], twins[i], got[i], nd, BN, flags, rec, h, "K = %d" % len(nd[0]))


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("nint", PICK_NINT)
def test_batch_pick_at_every_edge(gpu, nint, flags):
    seeds = (nint, nint + 5000)
    cases = [_pick_case(nint, s)[:3] for s in seeds]
    with H.Pool() as pool:
        hs = [pool.add(H.fresh(gpu, *c)) for c in cases]
        twins = [pool.add(H.fresh(gpu, *c)) for c in cases]
        ref = [H.slack_handle(*c) for c in cases]
        steps = [_pick_steps(nint, *c, H.slack_handle(*c)) for c in cases]
        with gpu.NodeBatch(hs) as nb:
            for step in range(4):
                is_int = steps[0][step][1]                              # the mask is per call: that of the first entry
                nodes = [s[step][0] for s in steps]
                got = nb.run([0, 1], nodes, nint, is_int=is_int, long_step=bool(flags))
                for i in range(2):
                    want = ref[i].node2(*nodes[i], nint, is_int=is_int, flags=SKIP | flags)
                    assert want["status"] == L.OPTIMAL and want["events"] == 0
                    _batch_entry(hs[i], twins[i], got[i], nodes[i], nint, flags, want, ref[i], "entry %d, step %d" % (i, step), is_int=is_int)


@pytest.mark.parametrize("flags", FLAGS)
def test_batch_pick_ties(gpu, flags):
    for nint in sorted({t[2] for t in TIES}):
        group = [t for t in TIES if t[2] == nint]
        cases = []
        for entries, winner, _ in group:
            T, basis, ub = _tie_case(gpu, entries, nint)
            h = H.slack_handle(T, basis, ub)
            cases.append((T, basis, ub, H.ref_node(h, H.node(), nint, flags), h))
        assert [c[3]["var"] for c in cases] == [t[1] for t in group]
        _run_k0_batch(gpu, cases, nint, flags)


@pytest.mark.parametrize("flags", FLAGS)
def test_batch_at_the_fit_boundary_and_on_wide_tied_rows(gpu, flags):
    cases, nint = [], min(n for m, n in D_SHAPES)
    for (m, n) in sorted(D_SHAPES):
        for pattern in ("empty", D_FLIP_PATTERN[(m, n)]):
            T, basis, ub, J, rec, h = _ref(m, n, pattern, flags)
            cases.append((T, basis, ub, rec, h))
    _run_k0_batch(gpu, cases, nint, flags)
    cases = []
    for (m, n) in sorted(E_SHAPES):
        (T, basis, ub, J, rec, h), tied = _ref_e(m, n, flags)
        cases.append((T, basis, ub, rec, h))
    _run_k0_batch(gpu, cases, min(n for m, n in E_SHAPES), flags, max_iter=500)


def _mixed_entries(gpu, pool, flags):
    """The entries of the mixed launch: (handle, twin, reference handle before the node, node, refused message or None)."""
    out = []

    def add(T, basis, ub, nd, h=None, refused=None, prepared=None):
        pair = prepared or (pool.add(H.fresh(gpu, T, basis, ub)), pool.add(H.fresh(gpu, T, basis, ub)))
        out.append((pair[0], pair[1], h if h is not None else H.slack_handle(T, basis, ub), nd, refused))

    add(*H.covering_with_fixed(1, 3, 1), H.node())                                              # 0: 2 x 5
    T, basis, ub, J, rec, h = _ref(1, 5053, "r10", flags)
    add(T, basis, ub, H.node())                                                                 # 1: 2 x 5055, the boundary shape
    J = np.union1d(_pattern("r10", 2100), [1500])
    T, basis, ub = _planted(4, 2100, J)
    ub[1500] = INF
    add(T, basis, ub, H.node(), refused="1 column(s) with a negative reduced cost and no upper bound")       # 2: second block
    h0 = _ref(BM, BN, "r10", flags)[5]
    src, twin_src = _b_handles(gpu, pool, flags)
    (cols, lower, upper), _ = _edit(h0, BN, 1025, 99)
    cols, lower, upper = cols.copy(), lower.copy(), upper.copy()
    cols[1024] = [int(j) for j in np.flatnonzero(h0.flip[:BN]) if j not in set(cols.tolist())][0]
    lower[1024], upper[1024] = 0.0, INF
    add(None, None, None, (cols, lower, upper), h=_copy(h0), refused="upper[1024] = +inf on a flipped column",
        prepared=(src, twin_src))                                                                # 3: +inf on a flipped column
    for K in (1, 3, 65, 1025):                                                                   # 4-7: odd K in front of later entries
        nd = _edit(h0, BN, K, 7 * K)[0]
        add(None, None, None, nd, h=_copy(h0), prepared=(pool.add(src.clone()), pool.add(twin_src.clone())))
    return out


@pytest.mark.parametrize("flags", FLAGS)
def test_mixed_launch_and_its_permutation(gpu, flags):
    nint = 3
    for order in (list(range(8)), [5, 2, 7, 0, 3, 6, 1, 4]):             # entry i runs on handles[order[i]]
        with H.Pool() as pool:
            ent = _mixed_entries(gpu, pool, flags)
            before = [H.reads(e[0], nint) for e in ent]
            with gpu.NodeBatch([e[0] for e in ent]) as nb:
                got = nb.run(order, [ent[s][3] for s in order], nint, long_step=bool(flags))
                msg = gpu._lib.last_error()
            first_refused = min(i for i, s in enumerate(order) if ent[s][4])
            assert "lpx_node_batch_run: entry %d: %s" % (first_refused, ent[order[first_refused]][4]) in msg
            for i, s in enumerate(order):
                dt, twin, h, nd, refused = ent[s]
                want = H.ref_node(h, nd, nint, flags) if not refused or "column(s)" in refused else None
                if refused:
                    assert got[i]["status"] is None and H.reads(dt, nint) == before[s], "the refused entry %d changed its handle" % i
                    assert want is None or (want["status"] is None and got[i]["unrepairable"] == want["unrepairable"] == 1)
                    continue
                _batch_entry(dt, twin, got[i], nd, nint, flags, want, h, "entry %d on slot %d" % (i, s))


def test_batch_buffers_regrow_and_serve_small_batches_again(gpu):
    flags = 0
    h0 = _ref(BM, BN, "r10", flags)[5]
    with H.Pool() as pool:
        src, twin_src = _b_handles(gpu, pool, flags)
        hs = [src, pool.add(src.clone()), pool.add(src.clone())]
        twins = [twin_src, pool.add(twin_src.clone()), pool.add(twin_src.clone())]
        ref = [_copy(h0) for _ in hs]
        with gpu.NodeBatch(hs) as nb:
            for step, Ks in enumerate(((1, 3, 0), (1025, 65, 1025), (3, 0, 1))):
                assert sum(Ks) == 4 or sum(Ks) > 2100
                nodes = [H.node() if K == 0 else _edit(ref[i], BN, K, 60 + 3 * step + i)[0] for i, K in enumerate(Ks)]
                got = nb.run([0, 1, 2], nodes, BN)
                for i in range(3):
                    want = H.ref_node(ref[i], nodes[i], BN, flags)
                    assert want["status"] is not None
                    _batch_entry(hs[i], twins[i], got[i], nodes[i], BN, flags, want, ref[i], "step %d, entry %d" % (step, i))
