"""Instances for the revised-path shape tests (tests/test_revised_ref.py, tests/test_gpu_revised_shapes.py).

Every builder returns (A[m, n], c[n], b[m]) of the standardised MINIMISATION that DeviceRevised and
oracle.revised_ref.RevisedRef take (c = -C of a Max model), with b >= 0.  The seeds of the crafted instances are
pinned: the tests assert from the reference's records that each still produces the event it was built for.
"""
import numpy as np

from linear_programming_solver_lpr381_amd import synth

SEG = 1024          # rows per segment of rv_select2's hysteresis scan (64 lanes x 16 ratios)


def dense(m, n, seed):
    """synth.dense_lp (A ~ U(0,1), Max) in minimisation form."""
    c, A, b = synth.dense_lp(m, n, seed=seed)
    return A, -c, b


def mixed(m, n, seed, dups=(), neg=None):
    """Mixed-sign A ~ U(-0.4, 1): columns enter, leave and re-enter, and slacks come back.  `dups` = [(x, y), ...]
    makes column y an exact copy of column x (cost included).  `neg`: only that many columns (the first ones) get a
    negative cost, the rest a positive one, so the run ends optimal after few pivots."""
    g = np.random.default_rng(seed)
    A = g.uniform(-0.4, 1.0, size=(m, n))
    b = g.uniform(1.0, 2.0, size=m)
    c = -g.uniform(0.5, 1.5, size=n)
    if neg is not None:
        c[neg:] = g.uniform(0.5, 1.5, size=n - neg)
        A[:, neg:] = np.abs(A[:, neg:])
    for x, y in dups:
        A[:, y] = A[:, x]
        c[y] = c[x]
    return A, c, b


def ratio_chain(m, ratios, n=6, seed=0):
    """First iteration with B = I: column 0 enters (cost -10, the others -1 .. 0), d = a_0 and x_B = b, so the ratio
    of row i is exactly b_i / a_0[i].  `ratios` = {row: theta} get a_0 = 1 and b = theta; every other row gets a
    ratio >= 2, or a_0 <= 0 (not eligible)."""
    g = np.random.default_rng(seed)
    A = g.uniform(0.0, 1.0, size=(m, n))
    a0 = np.where(g.random(m) < 0.8, 1.0, -g.uniform(0, 1, size=m))
    a0[g.random(m) < 0.05] = 0.0
    b = np.where(a0 > 0, 2.0 + g.uniform(0, 1, size=m), g.uniform(0, 1, size=m))
    for i, t in ratios.items():
        a0[i] = 1.0
        b[i] = t
    A[:, 0] = a0
    c = -g.uniform(0.0, 1.0, size=n)
    c[0] = -10.0
    return A, c, b


# ---- the hysteresis chains of rv_select2 (first iteration, forced entering column) --------------------------------
def _desc_chain(rows, start=1.0):
    """Descending ratios whose steps alternate outside (2e-12: taken) and inside (0.5e-12: not taken) the band."""
    out, v = {}, start
    for k, r in enumerate(rows):
        if k:
            v -= 2e-12 if k % 2 else 0.5e-12
        out[r] = v
    return out


CHAINS = {
    # ratio 1 + 5e-13 then 1 (in band): the earlier row keeps it, across each segment boundary and in the last partial segment
    "keep_1023_1024": (4500, {1023: 1.0 + 5e-13, 1024: 1.0}),
    "keep_2047_2048": (4500, {2047: 1.0 + 5e-13, 2048: 1.0}),
    "keep_4095_4096": (4500, {4095: 1.0 + 5e-13, 4096: 1.0}),
    "keep_last_partial": (4500, {4200: 1.0 + 5e-13, 4499: 1.0}),
    # descending chains across 1023/1024, 2047/2048, 4095/4096 into the last partial segment
    "desc_all": (4500, _desc_chain([1000, 1023, 1024, 2047, 2048, 4095, 4096, 4300])),
    "desc_last_in_band": (4500, _desc_chain([1023, 1024, 2047, 2048, 4095, 4096, 4300])),
    # exact zero-ratio ties (b_i = 0): the first row wins
    "zero_ties": (4500, {1023: 0.0, 1024: 0.0, 2048: 0.0, 4096: 0.0, 4499: 0.0}),
    "zero_ties_late": (4500, {2047: 0.0, 2048: 0.0, 4095: 0.0, 4096: 0.0}),
    # a segment that is not clean: two in-band ratios in one lane (rows r and r + 64 of one segment)
    "unclean_lane": (4500, {1100: 1.0 + 3e-13, 1164: 1.0, 3000: 1.0 + 2e-12}),
    "unclean_after_best": (4500, {500: 1.0 - 5e-12, 1100: 1.0 + 3e-13, 1164: 1.0}),
    # single segment (m <= 1024): the wave scan
    "keep_small": (1000, {10: 1.0 + 5e-13, 11: 1.0, 700: 1.0 + 2e-13}),
}
BOUNDARIES = (1024, 2048, 4096)


def chain(name):
    m, ratios = CHAINS[name]
    return ratio_chain(m, ratios, seed=len(name))


def embedded(m, n, core, rows, cols, seed=0):
    """A small LP `core` = (A, c, b) placed at rows `rows` and columns `cols` of an m x n instance.  The padding rows
    never bind (entries U(0, 0.01), b ~ 1e3) and the padding columns never price out (cost 50 .. 100), so the run
    follows the core's pivots, with the core's slacks and columns at the chosen indices."""
    Ac, cc, bc = core
    g = np.random.default_rng(seed)
    A = g.uniform(0.0, 0.01, size=(m, n))
    b = 1e3 * g.uniform(1.0, 2.0, size=m)
    c = g.uniform(50.0, 100.0, size=n)
    rows, cols = np.asarray(rows), np.asarray(cols)
    A[np.ix_(rows, cols)] = Ac
    b[rows] = bc
    c[cols] = cc
    return A, c, b


# ---- pinned cores (seeds found with the reference; the tests assert the event each was picked for) ---------------------
def reentry_core():
    """10 x 12: four slacks re-enter within 9 pivots to optimal."""
    return mixed(10, 12, 0)


def tie_core():
    """40 x 60, column j + 30 a copy of column j: twins tie exactly, and after a twin has entered and left, the copy with
    the larger column index holds the smaller order key and wins the tie."""
    return mixed(40, 60, 0, dups=[(j, j + 30) for j in range(30)])


def optimal_core():
    """30 x 40: optimal after 21 pivots, with slack re-entries."""
    return mixed(30, 40, 2)


def unbounded_core():
    """20 x 30: column 29 (all entries negative, cost -0.6) enters at the sixth iteration with d <= 0: unbounded."""
    A, c, b = mixed(20, 30, 351)
    A[:, 29] = -np.random.default_rng(358).uniform(0.1, 1.0, 20)
    c[29] = -0.6
    return A, c, b


def spread(k, m, lo=0):
    """k distinct row (or column) indices spread over [lo, m), first and last included."""
    return np.unique(np.linspace(lo, m - 1, k).round().astype(int))


def unbounded_embedded(m, n, seed=0):
    """unbounded_core() at rows spread(20, m) and columns spread(30, n), with zero padding entries in the core's columns:
    the run is the core's exactly, 5 pivots and then its crafted column (index spread(30, n)[29]) with no positive d."""
    rows, cols = spread(20, m), spread(30, n)
    A, c, b = embedded(m, n, unbounded_core(), rows, cols, seed)
    pad = np.setdiff1d(np.arange(m), rows)
    A[np.ix_(pad, cols)] = 0.0
    return A, c, b
