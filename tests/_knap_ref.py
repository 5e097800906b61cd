"""Exact restatement of ComputeRelaxation (Models/BranchAndBoundKnapsack.cs:431-491) and of the ratio order (:19, :75-79),
plus the instance, node and chain builders that tests/test_knapsack_reference.py (CPU) and tests/test_gpu_knapsack_edges.py
(GPU) share.  Test infrastructure only.

Every double is a dyadic rational, so the restatement works in Python integers over one power-of-two denominator: exact
rationals over the doubles as given, with the reference's three tests `W1 > cap + 1e-9`, `w + w_i <= cap + 1e-9` and
`remain > 1e-9 and w_i > 1e-9` decided without rounding.  For integer and dyadic data the running sums of the reference are
exact too, so `doubles()` -- the exact sums closed with the reference's three double operations -- is the oracle bit for bit;
for real data the exact answer is what the device's "1e-9 relative" is measured against."""
from dataclasses import dataclass
from fractions import Fraction
from functools import lru_cache

import numpy as np

KEPS = 1e-9                                  # :56
SIZES = (1, 2, 3, 63, 64, 65, 511, 512, 513, 1025, 4097)
FAMILIES = ("mixed", "nonneg", "ties", "dyadic", "fraccap", "real")
PREFIX_FAMILIES = ("nonneg", "ties", "dyadic", "fraccap")           # non-negative weights, sums exact in doubles
ZERO_FAMILIES = ("mixed", "nonneg", "ties", "dyadic", "fraccap")    # families that hold zero-weight items
CATEGORIES = ("over", "allfit", "frac", "tie")


def ratio_order(profit, weight):
    """Descending ratio (w > 0 ? p / w : +inf, the double quotient), then descending profit, then index."""
    p = np.asarray(profit, np.float64); w = np.asarray(weight, np.float64)
    ratio = np.full(len(p), np.inf)
    pos = w > 0
    ratio[pos] = p[pos] / w[pos]
    return np.lexsort((np.arange(len(p)), -p, -ratio)).astype(np.int32)


class Exact:
    """profit, weight, cap and 1e-9 as integers over one power-of-two denominator."""

    def __init__(self, profit, weight, cap):
        vals = [float(v) for v in profit] + [float(v) for v in weight] + [float(cap), KEPS]
        rat = [v.as_integer_ratio() for v in vals]
        self.den = max(d for _, d in rat)
        ints = [a * (self.den // d) for a, d in rat]
        n = len(profit)
        self.p, self.w, self.cap, self.eps = ints[:n], ints[n:2 * n], ints[2 * n], ints[2 * n + 1]

    def frac(self, v):
        return Fraction(v, self.den)


@dataclass
class Relax:
    category: str            # over / allfit / frac / tie (tie: a break item without a fraction)
    brk: int                 # ratio rank of the first undecided item that does not fit, -1 without one
    frac: int                # what the kernels report: brk for `frac`, else -1
    profit: Fraction         # exact
    weight: Fraction
    fracval: Fraction
    before_profit: Fraction  # totals in front of the break item (the totals themselves without one)
    before_weight: Fraction
    margin: Fraction         # smallest |threshold - value| over every comparison made


def relax(profit, weight, cap, order, fixed, exact=None):
    ex = exact if exact is not None else Exact(profit, weight, cap)
    thr = ex.cap + ex.eps
    W = 0; P = 0
    for i in sorted(fixed):                                           # :442-452
        if fixed[i] == 1:
            W += ex.w[i]; P += ex.p[i]
    margin = abs(thr - W)
    F = ex.frac
    if W > thr:                                                       # :455-456
        return Relax("over", -1, -1, F(P), F(W), Fraction(0), F(P), F(W), F(margin))
    for s, i in enumerate(order.tolist() if hasattr(order, "tolist") else order):   # :459-488
        if i in fixed:
            continue
        wi = ex.w[i]
        t = W + wi
        margin = min(margin, abs(thr - t))
        if t <= thr:
            W = t; P += ex.p[i]
            continue
        remain = ex.cap - W
        margin = min(margin, abs(remain - ex.eps))
        if remain > ex.eps:
            margin = min(margin, abs(wi - ex.eps))
            if wi > ex.eps:
                fv = Fraction(remain, wi)
                return Relax("frac", s, s, F(P) + F(ex.p[i]) * fv, F(W) + F(wi) * fv, fv, F(P), F(W), F(margin))
        return Relax("tie", s, -1, F(P), F(W), Fraction(0), F(P), F(W), F(margin))
    return Relax("allfit", -1, -1, F(P), F(W), Fraction(0), F(P), F(W), F(margin))


def doubles(r, profit, weight, cap, order):
    """(profit, weight, frac, fracval) as the reference's doubles, provided its running sums were exact (integer and dyadic
    data): the sums are taken from the exact restatement, the closing `remain / w_i`, `p += p_i * fr`, `w += w_i * fr`
    (:476-484) are the same three double operations."""
    p, w = float(r.before_profit), float(r.before_weight)
    assert Fraction(p) == r.before_profit and Fraction(w) == r.before_weight, "sums not representable: real data has no bit-exact form"
    if r.category != "frac":
        return p, w, -1, 0.0
    j = int(order[r.brk])
    fv = (float(cap) - w) / float(weight[j])
    return p + float(profit[j]) * fv, w + float(weight[j]) * fv, r.brk, fv


# ---- instances ------------------------------------------------------------------------------------------------------
def _family_seed(family):
    return FAMILIES.index(family) + 1


@lru_cache(maxsize=None)
def instance(family, n):
    """(profit, weight, cap) of one family at one size; the arrays are shared and must not be written to."""
    g = np.random.default_rng([_family_seed(family), n])
    if family == "mixed":
        w = g.integers(-50, 1001, size=n).astype(float)
        w[g.random(n) < 0.1] = 0.0
        p = np.abs(w) + g.integers(0, 101, size=n)
        cap = float(np.floor(0.5 * w[w > 0].sum()))
    elif family in ("nonneg", "dyadic", "fraccap"):
        w = g.integers(0, 1001, size=n).astype(float)
        w[g.random(n) < 0.1] = 0.0
        p = np.abs(w) + g.integers(0, 101, size=n)
        cap = float(np.floor(0.5 * w.sum()))
        if family == "dyadic":
            w, p, cap = w / 64.0, p / 64.0, cap / 64.0
        elif family == "fraccap":
            cap += 0.5
    elif family == "ties":
        # groups (p, w), (2p, 2w), (p, w): equal ratio with different profit and an exact duplicate; after every group one
        # zero-weight item, the first three of different profit (ratio +inf, ordered by profit)
        ws, ps = [], []
        k = 0
        while len(ws) < n:
            bw = float(g.integers(1, 1001)); bp = bw + float(g.integers(0, 101))
            ws += [bw, 2 * bw, bw, 0.0]; ps += [bp, 2 * bp, bp, float(7 + 5 * (k % 3))]
            k += 1
        w = np.array(ws[:n]); p = np.array(ps[:n])
        cap = float(np.floor(0.5 * w.sum()))
    elif family == "real":
        w = g.uniform(0.5, 1000.0, size=n)
        p = w * g.uniform(1.0, 1.1, size=n)
        cap = float(0.5 * w.sum())
    else:
        raise KeyError(family)
    p.setflags(write=False); w.setflags(write=False)
    return p, w, cap


@dataclass
class Case:
    """One instance with its nodes: `nodes` on the handle of capacity `cap`, `tie_nodes` on a second handle of capacity
    `tie_cap` (None when the instance has no item of positive weight)."""
    family: str
    n: int
    profit: np.ndarray
    weight: np.ndarray
    cap: float
    order: np.ndarray
    exact: Exact
    nodes: list
    tie_cap: float
    tie_exact: Exact
    tie_nodes: list

    def handles(self):
        """[(cap, exact, nodes)] of the one or two handles."""
        out = [(self.cap, self.exact, self.nodes)]
        if self.tie_cap is not None:
            out.append((self.tie_cap, self.tie_exact, self.tie_nodes))
        return out


def random_nodes(g, n, count=40, depth=300):
    """Random fixed sets of up to min(n, depth) decisions, as tests/test_gpu_models.py builds them."""
    out = []
    for _ in range(count):
        k = int(g.integers(0, min(n, depth)))
        idx = g.choice(n, size=k, replace=False)
        out.append({int(i): int(g.integers(0, 2)) for i in idx})
    return out


def over_nodes(g, weight, cap, count=6):
    """The heaviest items fixed to 1 until the cap is passed, plus a few more decisions that cannot bring the weight back."""
    n = len(weight)
    heavy = np.argsort(-weight, kind="stable")
    base = {}; tot = 0.0
    for i in heavy:
        if weight[i] <= 0 or tot > cap + 1.0:
            break
        base[int(i)] = 1; tot += float(weight[i])
    if not tot > cap + 1e-6:
        return []
    out = []
    for t in range(count):
        nd = dict(base)
        rest = [i for i in range(n) if i not in nd]
        for i in g.permutation(rest)[: min(len(rest), 3 * t)]:
            nd[int(i)] = int(g.integers(0, 2)) if weight[i] >= 0 else 0
        out.append(nd)
    return out


def allfit_nodes(g, weight, cap, count=6):
    """All but a few light items fixed to 0; the few are chosen so that they fit together."""
    n = len(weight)
    light = np.argsort(weight, kind="stable")[: min(n, 8)]
    out = []
    for t in range(count):
        keep = []; tot = 0.0
        for i in g.permutation(light)[: min(len(light), t)]:
            if tot + max(float(weight[i]), 0.0) <= cap:
                keep.append(int(i)); tot += max(float(weight[i]), 0.0)
        out.append({i: 0 for i in range(n) if i not in keep})
    return out


def tie_setup(g, weight, order, count=8):
    """(cap, nodes): cap = PW[k], the running sum of the weights in ratio order in front of rank k, with k the first rank
    >= n // 2 of positive weight (the last such rank when there is none behind the middle).  A node fixes to 1 a random subset
    of the ranks below k -- every item of negative weight among them, or the fixed weight alone overflows -- and to 0 a random
    subset of the ranks above k: everything in front of k fits exactly, item k does not, and nothing remains for a fraction."""
    n = len(weight)
    ws = weight[order]
    posr = [s for s in range(n) if ws[s] > 0]
    if not posr:
        return None, []
    behind = [s for s in posr if s >= n // 2]
    k = behind[0] if behind else posr[-1]
    PW = 0.0
    for s in range(k):
        PW += float(ws[s])
    nodes = []
    for _ in range(count):
        nd = {}
        for s in range(k):
            if ws[s] < 0 or g.random() < 0.3:
                nd[int(order[s])] = 1
        for s in range(k + 1, n):
            if g.random() < 0.3:
                nd[int(order[s])] = 0
        nodes.append(nd)
    return PW, nodes


@lru_cache(maxsize=None)
def case(family, n):
    p, w, cap = instance(family, n)
    order = ratio_order(p, w)
    g = np.random.default_rng([_family_seed(family), n, 17])
    nodes = [{}] + random_nodes(g, n) + over_nodes(g, w, cap) + allfit_nodes(g, w, cap)
    if family == "real":                    # a built tie sits 1e-9 from its threshold by construction: no margin to speak of
        tcap, tnodes = None, []
    else:
        tcap, tnodes = tie_setup(g, w, order)
    return Case(family, n, p, w, cap, order, Exact(p, w, cap), nodes, tcap,
                Exact(p, w, tcap) if tcap is not None else None, tnodes)


def categories(c):
    """Category counts of a case over both handles, and the number of nodes that would break on a zero-weight item if a
    kernel mis-ranked one: an undecided zero-weight item exists and the node is not `allfit`."""
    cnt = dict.fromkeys(CATEGORIES, 0)
    zero = 0
    zeros = [i for i in range(c.n) if c.weight[i] == 0]
    for cap, ex, nodes in c.handles():
        for nd in nodes:
            r = relax(c.profit, c.weight, cap, c.order, nd, ex)
            cnt[r.category] += 1
            if r.category != "allfit" and any(i not in nd for i in zeros):
                zero += 1
    return cnt, zero


def possible_categories(c):
    """The categories that can exist at all.  n <= 3: every one of the 3^n nodes on both handles is classified; above that
    every family reaches all four (the real family has no tie handle, see case())."""
    if c.n > 3:
        return set(CATEGORIES) - ({"tie"} if c.tie_cap is None else set())
    seen = set()
    for cap, ex, _ in c.handles():
        for code in range(3 ** c.n):
            nd = {}
            for i in range(c.n):
                v = (code // 3 ** i) % 3
                if v < 2:
                    nd[i] = v
            seen.add(relax(c.profit, c.weight, cap, c.order, nd, ex).category)
    return seen


def check_coverage(c, least=4):
    """The coverage condition of one case; returns its zero-weight count for the sum over the zero-weight families."""
    cnt, zero = categories(c)
    for cat in possible_categories(c):
        assert cnt[cat] >= least, (c.family, c.n, cat, cnt)
    return zero


# ---- chains for the node-store kernels ----------------------------------------------------------------------------------
PATTERNS = ("ascending", "descending", "alternating", "random")


def chain_ranks(pattern, n, length, g):
    """Ratio ranks in the order a chain fixes them: ascending = every decision appended to the stored list, descending =
    every decision inserted at its front, alternating = the two ends in turn, random."""
    if pattern == "ascending":
        return list(range(length))
    if pattern == "descending":
        return list(range(n - 1, n - 1 - length, -1))
    if pattern == "alternating":
        out = []
        for t in range(length):
            out.append(t // 2 if t % 2 == 0 else n - 1 - t // 2)
        return out
    return [int(s) for s in g.permutation(n)[:length]]


def chain_value(t):
    """Values are 0 except every seventh decision."""
    return 1 if t % 7 == 6 else 0


@dataclass
class ChainCase:
    n: int
    profit: np.ndarray
    weight: np.ndarray
    order: np.ndarray
    length: int
    chains: dict             # pattern -> [(item, value)] of `length` decisions
    caps: list               # the capacities of the two handles
    exacts: list


@lru_cache(maxsize=None)
def chain_case(n):
    """The non-negative family at size n with the four chains of min(n - 1, 520) decisions, on two handles: the family's own
    capacity (deep chains end `allfit`), and a small one set from the random chain so that its node half way down is a `tie`
    and the decisions fixed to 1 further down make it `over`."""
    p, w, cap = instance("nonneg", n)
    order = ratio_order(p, w)
    length = min(n - 1, 520)
    g = np.random.default_rng([n, 29])
    chains = {}
    for pat in PATTERNS:
        chains[pat] = [(int(order[s]), chain_value(t)) for t, s in enumerate(chain_ranks(pat, n, length, g))]
    half = dict(chains["random"][: (length + 1) // 2])
    small = sum(float(w[i]) for i, v in sorted(half.items()) if v == 1)
    taken = 0
    for s in range(n):                                     # the first two undecided items of positive weight fit exactly
        i = int(order[s])
        if i not in half and w[i] > 0 and taken < 2:
            small += float(w[i]); taken += 1
    caps = [cap, small]
    return ChainCase(n, p, w, order, length, chains, caps, [Exact(p, w, c) for c in caps])


# ---- whole searches -------------------------------------------------------------------------------------------------------
SEARCH_SIZES = ((1, 0), (2, 0), (3, 0), (18, 0), (60, 0), (400, 3000))    # (n, max_nodes; 0 = to exhaustion)


@lru_cache(maxsize=None)
def search_model(kind, n):
    """Models for BranchAndBoundKnapsack.Solve: `mixed` has negative and zero coefficients in its row (every relaxation goes
    through the scan kernel), `zero` zero coefficients only, `nonneg` neither."""
    g = np.random.default_rng([("mixed", "zero", "nonneg").index(kind) + 41, n])
    lo = -8 if kind == "mixed" else 1
    w = g.integers(lo, 60, size=n).astype(float)
    if kind != "nonneg":
        w[g.random(n) < 0.1] = 0.0
    p = np.abs(w) + g.integers(0, 12, size=n)
    cap = float(np.floor(0.5 * w[w > 0].sum()))
    p.setflags(write=False); w.setflags(write=False)
    return p, w, cap


CHAIN_SIZES = (2, 3, 65, 600)


@lru_cache(maxsize=None)
def chain_coverage(wide):
    """What the chain set meets in the kernel that LPX_KNAP_WIDE = `wide` is about -- "1": knap_expand_w (parents of at most
    512 entries), "0": knap_expand (every parent) -- from the restatement alone: slot-0 categories, the two q1 / q2
    placements, insertions at the front and at the end of a non-empty list, and the parent lengths."""
    met = dict.fromkeys(CATEGORIES + ("x2<x1", "x2>x1", "front", "end"), 0)
    met["parents"] = set()
    for n in CHAIN_SIZES:
        cc = chain_case(n)
        pos = {int(i): s for s, i in enumerate(cc.order)}
        for cap, ex in zip(cc.caps, cc.exacts):
            for pat in PATTERNS:
                fixed = {}; ranks = []
                for g, (item, val) in enumerate(cc.chains[pat]):
                    x1 = pos[item]
                    mine = wide == "0" or g <= 512
                    fixed[item] = val
                    met["parents"].add(g)
                    if mine:
                        if ranks and x1 < min(ranks):
                            met["front"] += 1
                        if ranks and x1 > max(ranks):
                            met["end"] += 1
                        r = relax(cc.profit, cc.weight, cap, cc.order, fixed, ex)
                        met[r.category] += 1
                        if r.frac >= 0:
                            met["x2<x1" if r.frac < x1 else "x2>x1"] += 1
                    ranks.append(x1)
    return met


# ---- real data ------------------------------------------------------------------------------------------------------------
REAL_SIZES = (65, 600, 4097)


@lru_cache(maxsize=None)
def real_chain(n):
    """A random chain of min(n - 1, 100) decisions on the real family, a quarter of them 1."""
    g = np.random.default_rng([n, 53])
    items = g.permutation(n)[: min(n - 1, 100)]
    return [(int(i), int(g.integers(0, 4) == 0)) for i in items]


def real_chain_nodes(n):
    out = []; fixed = {}
    for item, val in real_chain(n):
        fixed[item] = val
        out.append(dict(fixed))
    return out
