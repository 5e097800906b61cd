"""The exact restatement of the knapsack bound (tests/_knap_ref.py) against the CPU oracle, on every instance and node
family that tests/test_gpu_knapsack_edges.py runs on the device, and the coverage conditions of that file from the
restatement alone: a seed that stops reaching a branch fails here, before any GPU time is spent.  CPU only."""
from fractions import Fraction

import numpy as np
import pytest

import _knap_ref as K


def _assigned(n, nd):
    a = -np.ones(n, np.int32)
    for i, v in nd.items():
        a[i] = v
    return a


def _oracle(oracle, c, cap, nd):
    """(profit, weight, frac, fracval) of the oracle."""
    rp, rw, rf, rx = oracle.knapsack_relax(c.profit, c.weight, cap, c.order, _assigned(c.n, nd), want_vector=True)
    return rp, rw, rf, (float(rx[c.order[rf]]) if rf >= 0 else 0.0)


@pytest.mark.parametrize("family", K.FAMILIES)
def test_ratio_order_is_the_oracles(oracle, family):
    for n in K.SIZES + (600,):
        p, w, _ = K.instance(family, n)
        assert K.ratio_order(p, w).tolist() == oracle.knapsack_order(p, w).tolist(), (family, n)
    # the ties family really ties: equal ratio with different profit, exact duplicates, several items of ratio +inf
    p, w, _ = K.instance("ties", 65)
    order = K.ratio_order(p, w)
    ratio = np.where(w > 0, p / np.where(w > 0, w, 1.0), np.inf)[order]
    same = ratio[1:] == ratio[:-1]
    assert (same & (p[order][1:] < p[order][:-1])).sum() >= 16 and (same & (p[order][1:] == p[order][:-1])).sum() >= 16
    assert np.isinf(ratio).sum() >= 3 and len(set(p[order][np.isinf(ratio)])) == 3


@pytest.mark.parametrize("family", [f for f in K.FAMILIES if f != "real"])
def test_restatement_is_the_oracle_bit_for_bit_on_integer_and_dyadic_data(oracle, family):
    for n in K.SIZES:
        c = K.case(family, n)
        for cap, ex, nodes in c.handles():
            for j, nd in enumerate(nodes):
                r = K.relax(c.profit, c.weight, cap, c.order, nd, ex)
                assert K.doubles(r, c.profit, c.weight, cap, c.order) == _oracle(oracle, c, cap, nd), (family, n, cap, j)
                if r.category == "frac":
                    assert c.weight[c.order[r.frac]] > 0                     # no fractional item ever has zero weight


def test_restatement_agrees_with_the_oracle_on_real_data(oracle):
    """Profit and weight to 1e-12 relative: the oracle's sums are rounded, the restatement's are not (largest seen: 3.8e-15).
    The fraction is remain / w_i with remain = cap - w a difference of two numbers of the size of cap, so a relative bound on it
    says nothing about the sums; it is held to the same 1e-12 * cap in weight units, |fr - fr_exact| * w_i (largest seen:
    1.8e-15 * cap; relative to the fraction itself the oracle is 2.8e-10 off at n = 4097, where remain is 3.6e-6 * cap)."""
    worst = 0.0; worst_fr = 0.0; worst_rel = 0.0
    for n in K.SIZES:
        c = K.case("real", n)
        for j, nd in enumerate(c.nodes):
            r = K.relax(c.profit, c.weight, c.cap, c.order, nd, c.exact)
            rp, rw, rf, rv = _oracle(oracle, c, c.cap, nd)
            assert rf == r.frac, (n, j)
            for got, want in ((rp, r.profit), (rw, r.weight)):
                dev = abs(Fraction(got) - want) / max(abs(want), Fraction(1, 10 ** 300))
                worst = max(worst, float(dev))
                assert dev <= Fraction(1, 10 ** 12), (n, j, float(dev))
            if rf >= 0:
                dev = abs(Fraction(rv) - r.fracval) * Fraction(float(c.weight[c.order[rf]])) / Fraction(c.cap)
                worst_fr = max(worst_fr, float(dev))
                worst_rel = max(worst_rel, float(abs(Fraction(rv) - r.fracval) / r.fracval))
                assert dev <= Fraction(1, 10 ** 12), (n, j, float(dev))
    print("largest deviation oracle / exact: profit, weight %.3g relative; fraction %.3g * cap (%.3g relative)" % (worst, worst_fr, worst_rel))


def test_every_category_is_built_at_every_size():
    zero = 0
    for family in K.FAMILIES:
        for n in K.SIZES:
            z = K.check_coverage(K.case(family, n))
            if family in K.ZERO_FAMILIES:
                zero += z
    assert zero >= 4
    # every family holds what its name says
    assert all((K.instance("mixed", n)[1] < 0).any() for n in K.SIZES if n >= 63)
    for family in K.PREFIX_FAMILIES:
        assert all((K.instance(family, n)[1] >= 0).all() for n in K.SIZES)
        assert all((K.instance(family, n)[1] == 0).any() for n in K.SIZES if n >= 63)
    assert K.instance("fraccap", 65)[2] % 1 == 0.5 and (K.instance("dyadic", 65)[1] % 1 != 0).any()


def test_real_nodes_keep_their_distance_from_every_threshold():
    """The device may decide a comparison differently only within what a rounded sum can move, about n * 2^-53 relative; the
    GPU test leaves a node out of its `frac` comparison below 1e-10 * cap.  From the reference alone it leaves out none."""
    smallest = 1.0
    for n in K.REAL_SIZES:
        c = K.case("real", n)
        for nd in c.nodes + K.real_chain_nodes(n):
            r = K.relax(c.profit, c.weight, c.cap, c.order, nd, c.exact)
            smallest = min(smallest, float(r.margin) / c.cap)
    print("smallest margin / cap: %.3g" % smallest)
    assert smallest >= 1e-10


@pytest.mark.parametrize("wide", ["1", "0"])
def test_chains_meet_every_list_case(wide):
    met = K.chain_coverage(wide)
    assert met["x2<x1"] >= 10 and met["x2>x1"] >= 10, met
    for cat in ("over", "allfit", "tie", "frac"):
        assert met[cat] >= 1, met
    # parents of every length at which a kernel changes its step: KW_PER, the wave, 64 * KP_CACHE, KW_CAP (and one around)
    assert {0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513} <= met["parents"]
    assert met["front"] >= 500 and met["end"] >= 500                      # before == 0 with a list to shift / appended


def test_search_models_leave_the_default_path_and_stay_small(oracle):
    for kind in ("mixed", "zero", "nonneg"):
        for n, cap_nodes in K.SEARCH_SIZES:
            p, w, cap = K.search_model(kind, n)
            ref = oracle.knapsack_solve(oracle.Problem(oracle.MAX, p, w.reshape(1, -1), [oracle.LE], [cap]), max_nodes=cap_nodes)
            assert ref.rc == 0 and ref.nodes_popped <= 3000, (kind, n)
            if n >= 18:
                assert (w < 0).any() == (kind == "mixed") and (w == 0).any() == (kind != "nonneg")
    assert sum((K.search_model("mixed", n)[1] < 0).any() for n, _ in K.SEARCH_SIZES) >= 4
