"""The five knapsack bound kernels (csrc/lpx_knapsack.hip) at their edges, against the CPU oracle bit for bit and, for data
whose sums round, against the exact restatement tests/_knap_ref.py: the 512-lane scan kernel that negative weights select
(no other GPU test runs it), zero weights, exact-fit breaks, n = 1 .. 3, the node-store lists on chains that insert at the
front, at the end and on both sides of the fractional item at every parent length where a kernel changes its step, dyadic and
real data, whole searches off the default path, and the argument checks.  Instances, nodes and chains come from _knap_ref;
tests/test_knapsack_reference.py pins them to the oracle and asserts their coverage on the CPU."""
import ctypes as C
import json
import os
import subprocess
import sys
import textwrap
from fractions import Fraction

import numpy as np
import pytest

import _knap_ref as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (2, 256)


def _assigned(n, nd):
    a = -np.ones(n, np.int32)
    for i, v in nd.items():
        a[i] = v
    return a


def _oracle(oracle, p, w, cap, order, nd):
    """(profit, weight, frac, fracval) of the oracle."""
    rp, rw, rf, rx = oracle.knapsack_relax(p, w, cap, order, _assigned(len(p), nd), want_vector=True)
    return rp, rw, rf, (float(rx[order[rf]]) if rf >= 0 else 0.0)


def _slot(P, W, F, X, *ix):
    return float(P[ix]), float(W[ix]), int(F[ix]), float(X[ix])


def _einval(gpu, call):
    with pytest.raises(gpu._lib.LpxError) as e:
        call()
    assert e.value.code == gpu._lib.EINVAL
    return True


# ---- 1. the scan kernel ---------------------------------------------------------------------------------------------------
def test_scan_kernel_on_mixed_sign_weights(gpu, oracle):
    """knap_relax_batch, selected by a negative weight alone: per = ceil(n / 512) = 1, 1, 2, 3, 9 with and without empty tail
    lanes, the last-lane exit (`allfit`), the owner-of-the-break exit (`frac`, `tie`) and the overflow exit."""
    lib = gpu._lib.lib()
    for n in K.SIZES:
        c = K.case("mixed", n)
        K.check_coverage(c)
        for cap, ex, nodes in c.handles():
            dk = gpu.DeviceKnapsack(c.profit, c.weight, cap)
            try:
                assert dk.order().tolist() == c.order.tolist() == oracle.knapsack_order(c.profit, c.weight).tolist()
                negative = bool((c.weight < 0).any())
                assert lib.lpx_knapsack_has_prefix(dk._h) == (0 if negative else 1), n
                got = dk.relax_batch(nodes)
                for j, nd in enumerate(nodes):
                    want = _oracle(oracle, c.profit, c.weight, cap, c.order, nd)
                    assert _slot(*got, j) == want, (n, cap, j)
                    assert want == K.doubles(K.relax(c.profit, c.weight, cap, c.order, nd, ex), c.profit, c.weight, cap, c.order)
                if negative:
                    _einval(gpu, lambda: dk.relax_batch2(nodes[:2]))
                    _einval(gpu, lambda: dk.expand_batch([-1], [0], [0]))
                    again = dk.relax_batch(nodes)
                    assert all(np.array_equal(a, b) for a, b in zip(got, again))
            finally:
                dk.close()
    assert sum(bool((K.instance("mixed", n)[1] < 0).any()) for n in K.SIZES) >= 9


# ---- 2. scan against prefix, 5. searches under the switches: child processes ----------------------------------------------
CHILD = textwrap.dedent('''
    import json, os, sys
    import numpy as np
    import linear_programming_solver_lpr381_amd as L
    import _knap_ref as K

    def searches(kinds):
        out = {}
        for kind in kinds:
            for n, cap_nodes in K.SEARCH_SIZES:
                p, w, cap = K.search_model(kind, n)
                kp = L.LPProblem(L.Sense.Max, p.tolist(), [L.Constraint(w.tolist(), L.Rel.LE, cap)])
                for width in (2, 256):
                    r = L.BranchAndBoundKnapsack(max_nodes=cap_nodes, concurrent_nodes=width).Solve(kp)
                    fin = bool(np.isfinite(r.OptimalValue))
                    out["%s/%d/%d" % (kind, n, width)] = [int(r.Nodes), int(r.Aux[0]), int(r.Aux[2]), int(r.Aux[3]),
                                                         float(r.OptimalValue) if fin else None,
                                                         r.Extra.astype(int).tolist() if fin else None]
        return out

    res = {}
    if os.environ.get("LPX_KNAP_SCAN") == "1":
        relax = {}
        for family in ("nonneg", "ties", "fraccap"):
            for n in K.SIZES:
                c = K.case(family, n)
                for h, (cap, ex, nodes) in enumerate(c.handles()):
                    dk = L.DeviceKnapsack(c.profit, c.weight, cap)
                    assert L._lib.lib().lpx_knapsack_has_prefix(dk._h) == 1
                    relax["%s/%d/%d" % (family, n, h)] = [a.tolist() for a in dk.relax_batch(nodes)]
                    try:                         # the switch took: the scan path has no depth-2 form
                        dk.relax_batch2(nodes[:1]); refused = False
                    except L._lib.LpxError as e:
                        refused = e.code == L._lib.EINVAL
                    assert refused
                    dk.close()
        res["relax"] = relax
        res["search"] = searches(("nonneg",))
        os.environ["LPX_KNAP_DEPTH2"] = "0"     # read by every Solve: now every relaxation of the search is a scan
        res["search_depth2_off"] = searches(("nonneg", "zero"))
    else:
        res["search"] = searches(("nonneg", "zero"))
    print(json.dumps(res))
''')


def _child(**env):
    """One fresh Python process with the given switches; they are read once per process (LPX_KNAP_SCAN) or per solve."""
    full = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **env)
    r = subprocess.run([sys.executable, "-c", CHILD], env=full, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def scan_child():
    return _child(LPX_KNAP_SCAN="1")


def test_scan_equals_prefix_on_the_same_data(gpu, oracle, scan_child):
    """LPX_KNAP_SCAN=1 in a child process against the prefix kernel in this one and the oracle, bit for bit: zero weights at
    the front of the scan's first slices, ratio ties, a cap that is not an integer."""
    for family in ("nonneg", "ties", "fraccap"):
        for n in K.SIZES:
            c = K.case(family, n)
            K.check_coverage(c)
            for h, (cap, ex, nodes) in enumerate(c.handles()):
                scan = scan_child["relax"]["%s/%d/%d" % (family, n, h)]
                dk = gpu.DeviceKnapsack(c.profit, c.weight, cap)
                try:
                    mine = dk.relax_batch(nodes)
                finally:
                    dk.close()
                for j, nd in enumerate(nodes):
                    want = _oracle(oracle, c.profit, c.weight, cap, c.order, nd)
                    assert _slot(*mine, j) == want, (family, n, h, j)
                    assert (scan[0][j], scan[1][j], scan[2][j], scan[3][j]) == want, (family, n, h, j)


# ---- 3. the prefix kernels on the new data ----------------------------------------------------------------------------------
@pytest.mark.parametrize("family", K.PREFIX_FAMILIES)
def test_prefix_kernels_on_zero_weights_ties_and_exact_fits(gpu, oracle, family):
    """knap_relax_prefix<false> and <true>: slot 0 against the oracle, slots 1 / 2 against the oracle with the fractional item
    fixed to 0 / 1, -2 exactly where the node has no fractional item (`over`, `allfit` and `tie` alike), and never a
    fractional item of zero weight."""
    for n in K.SIZES:
        c = K.case(family, n)
        K.check_coverage(c)
        for cap, ex, nodes in c.handles():
            dk = gpu.DeviceKnapsack(c.profit, c.weight, cap)
            try:
                P1, W1, F1, X1 = dk.relax_batch(nodes)
                P, W, F, X = dk.relax_batch2(nodes)
            finally:
                dk.close()
            for a, b in ((P, P1), (W, W1), (F, F1), (X, X1)):
                assert np.array_equal(a[:, 0], b), (family, n)
            for j, nd in enumerate(nodes):
                assert _slot(P, W, F, X, j, 0) == _oracle(oracle, c.profit, c.weight, cap, c.order, nd), (family, n, cap, j)
                cat = K.relax(c.profit, c.weight, cap, c.order, nd, ex).category
                if cat != "frac":
                    assert F[j, 0] == -1 and F[j, 1] == -2 and F[j, 2] == -2, (family, n, cap, j, cat)
                    continue
                item = int(c.order[F[j, 0]])
                assert c.weight[item] > 0
                for v in (0, 1):
                    nd2 = dict(nd); nd2[item] = v
                    assert _slot(P, W, F, X, j, 1 + v) == _oracle(oracle, c.profit, c.weight, cap, c.order, nd2), (family, n, cap, j, v)
                    if F[j, 1 + v] >= 0:
                        assert c.weight[c.order[F[j, 1 + v]]] > 0


# ---- 4. the store kernels on deterministic chains -----------------------------------------------------------------------
def _check_job(dk, oracle, cc, cap, fx, node_id, P, W, F, X, j, where):
    """One expand job: the stored list of the node, all three slots against the oracle, the stored lists of its two children."""
    assert dk.node_list(node_id) == fx, where
    assert _slot(P, W, F, X, j, 0) == _oracle(oracle, cc.profit, cc.weight, cap, cc.order, fx), where
    if F[j, 0] < 0:
        assert F[j, 0] == -1 and F[j, 1] == -2 and F[j, 2] == -2, where
        return
    item = int(cc.order[F[j, 0]])
    for v in (0, 1):
        fx2 = dict(fx); fx2[item] = v
        assert dk.node_list(node_id + 1 + v) == fx2, (where, v)
        assert _slot(P, W, F, X, j, 1 + v) == _oracle(oracle, cc.profit, cc.weight, cap, cc.order, fx2), (where, v)


@pytest.mark.parametrize("wide", ["1", "0"])
def test_store_kernels_on_deterministic_chains(gpu, oracle, monkeypatch, wide):
    """knap_expand_w (LPX_KNAP_WIDE=1, parents of at most 512 entries) and knap_expand: four chains per handle -- always
    appended, always inserted at the front, alternating ends, random -- checked at EVERY generation, so parents of 0, 1, 7,
    8, 9, 63, 64, 65, 255, 256, 257, 511, 512 and 513 entries all occur; then one batch that mixes a parent of 513 entries
    with shallow ones against the same jobs without it."""
    monkeypatch.setenv("LPX_KNAP_WIDE", wide)
    met = K.chain_coverage(wide)
    assert met["x2<x1"] >= 10 and met["x2>x1"] >= 10 and all(met[cat] >= 1 for cat in K.CATEGORIES), met
    assert {0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513} <= met["parents"]
    for n in K.CHAIN_SIZES:
        cc = K.chain_case(n)
        for cap in cc.caps:
            dk = gpu.DeviceKnapsack(cc.profit, cc.weight, cap)
            try:
                parent = dict.fromkeys(K.PATTERNS, -1)
                fixed = {pat: {} for pat in K.PATTERNS}
                at_depth = {0: (-1, {})}                       # the random chain: depth -> (node id, fixed set)
                for g in range(cc.length):
                    ids, P, W, F, X = dk.expand_batch([parent[pat] for pat in K.PATTERNS], [cc.chains[pat][g][0] for pat in K.PATTERNS],
                                                      [cc.chains[pat][g][1] for pat in K.PATTERNS])
                    for j, pat in enumerate(K.PATTERNS):
                        item, val = cc.chains[pat][g]
                        fixed[pat][item] = val
                        parent[pat] = int(ids[j])
                        _check_job(dk, oracle, cc, cap, fixed[pat], int(ids[j]), P, W, F, X, j, (n, cap, pat, g))
                    at_depth[g + 1] = (parent["random"], dict(fixed["random"]))
                if n == 600 and cap == cc.caps[0]:
                    # parents of 0, 8, 512 and 513 entries in one call (WIDE=1: the 513 sends all of them through knap_expand),
                    # then the first three alone (WIDE=1: knap_expand_w)
                    depths = (0, 8, 512, 513)
                    free = [i for i in range(n) if i not in at_depth[513][1]][:4]
                    vals = [0, 1, 0, 1]
                    runs = []
                    for count in (4, 3):
                        ids, P, W, F, X = dk.expand_batch([at_depth[d][0] for d in depths[:count]], free[:count], vals[:count])
                        for j in range(count):
                            fx = dict(at_depth[depths[j]][1]); fx[free[j]] = vals[j]
                            _check_job(dk, oracle, cc, cap, fx, int(ids[j]), P, W, F, X, j, ("mixed batch", count, j))
                        runs.append((P, W, F, X))
                    live = runs[1][2] != -2
                    assert np.array_equal(runs[0][2][:3], runs[1][2])
                    for a, b in zip(runs[0], runs[1]):
                        assert np.array_equal(a[:3][live], b[live])
            finally:
                dk.close()


# ---- 5. whole searches off the default path ---------------------------------------------------------------------------------
def _search_ref(oracle, kind, n, cap_nodes):
    p, w, cap = K.search_model(kind, n)
    ref = oracle.knapsack_solve(oracle.Problem(oracle.MAX, p, w.reshape(1, -1), [oracle.LE], [cap]), max_nodes=cap_nodes)
    fin = bool(np.isfinite(ref.best_z))
    return [ref.nodes_popped, ref.relaxations, ref.nodes_expanded, ref.max_heap, float(ref.best_z) if fin else None,
            ref.best_x.tolist() if fin else None]


def test_searches_with_negative_and_zero_coefficients(gpu, oracle):
    """BranchAndBoundKnapsack.Solve with one negative coefficient in its row runs every relaxation through the scan kernel
    and the host's one-relaxation-per-job path; zero coefficients keep the default path.  Popped, relaxations, expanded,
    largest heap, z and x equal the oracle's."""
    Pm, C_, S, R = gpu.LPProblem, gpu.Constraint, gpu.Sense, gpu.Rel
    for kind in ("mixed", "zero"):
        for n, cap_nodes in K.SEARCH_SIZES:
            p, w, cap = K.search_model(kind, n)
            want = _search_ref(oracle, kind, n, cap_nodes)
            for width in WIDTHS:
                r = gpu.BranchAndBoundKnapsack(max_nodes=cap_nodes, concurrent_nodes=width).Solve(Pm(S.Max, p.tolist(), [C_(w.tolist(), R.LE, cap)]))
                fin = bool(np.isfinite(r.OptimalValue))
                got = [int(r.Nodes), int(r.Aux[0]), int(r.Aux[2]), int(r.Aux[3]), float(r.OptimalValue) if fin else None,
                       r.Extra.astype(int).tolist() if fin else None]
                assert got == want, (kind, n, width)


def test_searches_under_the_switches(oracle, scan_child):
    """The same searches in child processes: LPX_KNAP_DEPTH2=0 (one relaxation per job, lists shipped), LPX_KNAP_SCAN=1 (the
    root through the scan kernel) and both (every relaxation through it)."""
    runs = {"depth2 off": _child(LPX_KNAP_DEPTH2="0")["search"], "scan": scan_child["search"],
            "scan, depth2 off": scan_child["search_depth2_off"]}
    for name, got in runs.items():
        kinds = ("nonneg",) if name == "scan" else ("nonneg", "zero")
        assert len(got) == len(kinds) * len(K.SEARCH_SIZES) * len(WIDTHS)
        for kind in kinds:
            for n, cap_nodes in K.SEARCH_SIZES:
                want = _search_ref(oracle, kind, n, cap_nodes)
                for width in WIDTHS:
                    assert got["%s/%d/%d" % (kind, n, width)] == want, (name, kind, n, width)


# ---- 6. data that is not integral ---------------------------------------------------------------------------------------------
def test_dyadic_data_stays_bit_exact_in_the_store_kernels(gpu, oracle, monkeypatch):
    """Sums of multiples of 1/64 are exact: the relax kernels are covered by the dyadic case of the prefix test above, here a
    random chain through both store kernels."""
    for wide in ("1", "0"):
        monkeypatch.setenv("LPX_KNAP_WIDE", wide)
        for n in (65, 600):
            p, w, cap = K.instance("dyadic", n)
            cc = K.ChainCase(n, p, w, K.ratio_order(p, w), 0, {}, [cap], [])
            dk = gpu.DeviceKnapsack(p, w, cap)
            try:
                parent, fx = -1, {}
                for g, (item, val) in enumerate(K.real_chain(n)):
                    ids, P, W, F, X = dk.expand_batch([parent], [item], [val])
                    fx[item] = val; parent = int(ids[0])
                    _check_job(dk, oracle, cc, cap, fx, parent, P, W, F, X, 0, (wide, n, g))
            finally:
                dk.close()


@pytest.mark.parametrize("path", ["relax_batch", "relax_batch2", "expand_batch"])
@pytest.mark.parametrize("n", K.REAL_SIZES)
def test_real_data_within_1e9_of_the_exact_answer(gpu, n, path):
    """The header of lpx_knapsack.hip promises 1e-9 relative for data whose sums round.  relax_batch, relax_batch2 and a random
    expand_batch chain on real-valued data against the exact rationals: `frac` equal, profit, weight and fraction within 1e-9
    relative.  A node is left out of the comparison only if its exact margin is below 1e-10 * cap (a rounded sum of 5000 terms
    moves by about 1e-12 * cap), at most one per n; the reference alone leaves out none (smallest margin 3.1e-6 * cap).

    Largest relative deviation measured on an MI355X: relax_batch / relax_batch2 profit 2.9e-16, weight 2.2e-16, fraction
    2.5e-11; expand_batch chains profit 2.8e-15, weight 1.4e-15, fraction 2.1e-10.  Before knap_relax_prefix closed with
    error-free sums, `allfit` nodes that leave almost nothing undecided missed the bound: the undecided sum is PW[n] minus the
    fixed weight, two numbers of the size of the instance total (n = 4097: weight 2.3e-9 relative, 4.9e-9 instead of an exact 0)."""
    worst = {"profit": 0.0, "weight": 0.0, "fraction": 0.0}
    misses = []
    left_out = []
    c = K.case("real", n)

    def close(got, nd, where):
        """True when the slot was compared and may be branched on."""
        r = K.relax(c.profit, c.weight, c.cap, c.order, nd, c.exact)
        if got[2] != r.frac:
            assert r.margin < Fraction(1, 10 ** 10) * Fraction(c.cap), (where, got, r)
            left_out.append(where)
            return False
        for name, g, want in (("profit", got[0], r.profit), ("weight", got[1], r.weight), ("fraction", got[3], r.fracval)):
            dev = abs(Fraction(g) - want)
            if want != 0:
                worst[name] = max(worst[name], float(dev / abs(want)))
            if dev > Fraction(1, 10 ** 9) * abs(want):
                misses.append((where, r.category, name, g, float(want), float(dev)))
        return True

    def three(P, W, F, X, j, nd, where):
        if not close(_slot(P, W, F, X, j, 0), nd, (where, 0)):
            return
        if F[j, 0] < 0:
            assert F[j, 1] == -2 and F[j, 2] == -2, where
            return
        item = int(c.order[F[j, 0]])
        for v in (0, 1):
            nd2 = dict(nd); nd2[item] = v
            close(_slot(P, W, F, X, j, 1 + v), nd2, (where, 1 + v))

    dk = gpu.DeviceKnapsack(c.profit, c.weight, c.cap)
    try:
        if path == "relax_batch":
            got = dk.relax_batch(c.nodes)
            for j, nd in enumerate(c.nodes):
                close(_slot(*got, j), nd, j)
        elif path == "relax_batch2":
            P, W, F, X = dk.relax_batch2(c.nodes)
            for j, nd in enumerate(c.nodes):
                three(P, W, F, X, j, nd, j)
        else:
            parent, fx = -1, {}
            for g, (item, val) in enumerate(K.real_chain(n)):
                ids, P, W, F, X = dk.expand_batch([parent], [item], [val])
                fx[item] = val; parent = int(ids[0])
                assert dk.node_list(parent) == fx
                three(P, W, F, X, 0, fx, g)
    finally:
        dk.close()
    print("n = %d, %s: largest relative deviation from the exact answer: " % (n, path) + ", ".join("%s %.3g" % kv for kv in worst.items()))
    for m in misses:
        print("outside 1e-9 relative:", m)
    assert len(left_out) <= 1, left_out
    assert not misses, (len(misses), misses[:8])


# ---- 7. argument checks that need a device ------------------------------------------------------------------------------------
def test_argument_checks_leave_the_handle_usable(gpu):
    lib = gpu._lib.lib(); EINVAL = gpu._lib.EINVAL
    dp = gpu._lib.dp
    short = np.ones(4)
    h = C.c_void_p()
    for n in (0, -1, 1200001):                         # the count is checked before anything is read
        assert lib.lpx_knapsack_create(short.ctypes.data_as(dp), short.ctypes.data_as(dp), n, 1.0, C.byref(h)) == EINVAL and not h
    p, w, cap = K.instance("nonneg", 65)
    dk = gpu.DeviceKnapsack(p, w, cap)
    try:
        probe = [{}, {3: 1, 7: 0}]
        base = dk.relax_batch(probe)
        base2 = dk.relax_batch2(probe)

        def usable():
            return (all(np.array_equal(a, b) for a, b in zip(base, dk.relax_batch(probe)))
                    and all(np.array_equal(a, b) for a, b in zip(base2, dk.relax_batch2(probe))))

        for bad in ({65: 1}, {-1: 0}, {2: 1, 1 << 20: 0}):                       # a fixed index outside [0, n)
            assert _einval(gpu, lambda: dk.relax_batch([{}, bad])) and usable()
            assert _einval(gpu, lambda: dk.relax_batch2([bad])) and usable()
        assert _einval(gpu, lambda: dk.expand_batch([0], [1], [0])) and usable()           # a parent id never returned
        assert _einval(gpu, lambda: dk.expand_batch([-2], [1], [0])) and usable()
        assert _einval(gpu, lambda: dk.expand_batch([-1], [1], [2])) and usable()          # val of 2
        assert _einval(gpu, lambda: dk.expand_batch([-1], [65], [0])) and usable()         # an item outside [0, n)
        assert _einval(gpu, lambda: dk.node_list(0))
        assert lib.lpx_knapsack_expand_finish(dk._h, None, None, None, None) == 0 and usable()   # nothing in flight: a no-op
        # nothing was stored by the refused calls: the first accepted job gets id 0, its children 1 and 2
        ids, P, W, F, X = dk.expand_batch([-1, -1], [3, 7], [1, 0])
        assert ids.tolist() == [0, 3] and dk.node_list(0) == {3: 1} and dk.node_list(3) == {7: 0}
        assert _einval(gpu, lambda: dk.expand_batch([6], [1], [0])) and usable()           # one past the last id
        ids2, P2, W2, F2, X2 = dk.expand_batch([0], [7], [0])
        assert ids2.tolist() == [6] and dk.node_list(6) == {3: 1, 7: 0}
        assert _slot(P2, W2, F2, X2, 0, 0) == _slot(*base, 1)
    finally:
        dk.close()
