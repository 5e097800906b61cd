"""Two pieces of arithmetic of the select-only pair (lpx_pivot_ratio, lpx_pivot_select in lpx_pivot_fused.hip) restated in NumPy.

1. The entering column under any partition of the columns.  The row launch's workgroups own shares of the handle's CAPACITY, not
of the live columns (their early loads are issued before the live shape is known).  The entering column is the argmin of mi_pick
(strict minimum, lowest index on equal values) over per-lane results of rule_feed (strict `<` in ascending order): the same
column whatever the partition, empty shares included.

2. The scan record of the column launch in ONE exchange among the waves, against the ballot count the kernel uses.  A workgroup
reduces its SELC_ROWS = 256 ratios (four waves of 64; rows that are not live constraint rows count as +inf and take no part) to a
record: the least ratio v, its first row, and whether that row is ALONE in the band, i.e. whether exactly one live row x has
fl(x - tol) <= v.  The kernel counts those rows with a ballot per wave, behind a first exchange that gives every wave v, and sums
the counts in a second exchange.  The one-exchange form publishes three values per wave -- its least ratio, that ratio's first
row, its second least ratio -- and counts over the eight published values.  x -> fl(x - tol) is monotone, so the rows inside the
band are the least ones, and the least two rows of the workgroup are among the published values: the two counts are 0 together,
1 together and >= 2 together.  A record of +inf has every live row in its band, and there the lanes past the live rows (+inf as
well) would be counted too: the count is then the number of live rows.  This form was built into the kernel and measured in r17;
it did not lower the launch's time and the kernel keeps the ballots.  The equivalence is kept here, checked, for
whoever takes it up again."""
import numpy as np
import pytest

ROWS, WAVE = 256, 64
INF = np.inf
TOL = 1e-9


def record_by_ballot(x, nlive, tol):
    """The record as the kernel (two exchanges, a ballot per wave) computes it.  x: 256 ratios, rows >= nlive are not live."""
    x = np.asarray(x, dtype=np.float64)
    rt = np.where(np.arange(ROWS) < nlive, x, INF)
    v = rt.min()
    first = int(np.flatnonzero(rt == v)[0])
    inband = int(np.count_nonzero((np.arange(ROWS) < nlive) & ((rt - np.float64(tol)) <= v)))
    return v, first, inband == 1


def mi_pick(a, b):
    return b if (b[0] < a[0] or (b[0] == a[0] and b[1] < a[1])) else a


def record_by_exchange(x, nlive, tol):
    """The record from the least ratio, its first row and the second least ratio of every wave."""
    x = np.asarray(x, dtype=np.float64)
    rt = np.where(np.arange(ROWS) < nlive, x, INF)
    pub = []
    for w in range(ROWS // WAVE):
        seg = rt[w * WAVE:(w + 1) * WAVE]
        v1 = seg.min()
        i1 = int(np.flatnonzero(seg == v1)[0])
        v2 = np.delete(seg, i1).min()
        pub.append((v1, w * WAVE + i1, v2))
    best = (pub[0][0], pub[0][1])
    for v1, i1, _ in pub[1:]:
        best = mi_pick(best, (v1, i1))
    v = best[0]
    inband = sum(int((v1 - np.float64(tol)) <= v) + int((v2 - np.float64(tol)) <= v) for v1, _, v2 in pub)
    if not v < INF:
        inband = min(nlive, ROWS)
    return v, best[1], inband == 1


def _agree(x, nlive=ROWS, tol=TOL):
    a, b = record_by_ballot(x, nlive, tol), record_by_exchange(x, nlive, tol)
    assert a == b, (a, b, nlive, tol)
    return a


def test_random_vectors():
    g = np.random.default_rng(11)
    for k in range(300):
        x = g.uniform(0.0, 10.0, ROWS)
        x[g.random(ROWS) < g.choice([0.0, 0.3, 0.9, 0.99])] = INF         # ineligible rows
        _agree(x, nlive=int(g.choice([ROWS, ROWS - 1, 200, 65, 64, 63, 2, 1, 0])))
    # near-ties: many values within a few tol of each other
    for k in range(300):
        x = 1.0 + g.integers(0, 6, ROWS) * (TOL / 2)
        _agree(x, nlive=int(g.choice([ROWS, 130, 64])))


def test_inf_rows_and_ineligible_blocks():
    x = np.full(ROWS, INF)
    for nlive in (ROWS, 65, 64, 2, 1, 0):
        v, first, alone = _agree(x, nlive)
        assert v == INF and first == 0 and alone == (nlive == 1)
    # one eligible row in any wave, first or last lane
    for row in (0, 63, 64, 127, 128, 200, 255):
        x = np.full(ROWS, INF); x[row] = 3.0
        assert _agree(x) == (3.0, row, True)
        assert _agree(x, nlive=row + 1) == (3.0, row, True)
        v, first, alone = _agree(x, nlive=row)
        assert v == INF and alone == (row == 1)
    # a whole wave ineligible beside the minimum's
    x = np.linspace(1.0, 2.0, ROWS); x[64:128] = INF
    assert _agree(x) == (1.0, 0, True)


@pytest.mark.parametrize("a,b", [(10, 11), (0, 63), (5, 70), (63, 64), (20, 250), (128, 255)])
def test_exact_duplicates_within_and_across_waves(a, b):
    g = np.random.default_rng(a * 256 + b)
    x = g.uniform(2.0, 9.0, ROWS)
    x[a] = x[b] = 1.0
    assert _agree(x) == (1.0, a, False)
    assert _agree(x, nlive=b) == (1.0, a, True)          # the copy is not a live row
    x[g.integers(0, ROWS)] = 1.0                         # maybe a third
    assert _agree(x)[2] is False
    # duplicates that are not the minimum do not matter
    x = g.uniform(2.0, 9.0, ROWS); x[a] = x[b] = 1.5; x[(a + 7) % ROWS if (a + 7) % ROWS != b else (a + 9) % ROWS] = 1.0
    assert _agree(x)[2] is True


@pytest.mark.parametrize("tol", [1e-9, 1e-6, 0.0, 0.25])
@pytest.mark.parametrize("where", [(3, 4), (3, 100), (200, 7), (64, 127)])
def test_values_on_the_band_edge(tol, where):
    """A second value x with fl(x - tol) equal to, just below and just above the minimum, in the minimum's wave or another."""
    lo, other = where
    vmin = np.float64(1.0)
    x0 = vmin + np.float64(tol)
    cands = [x0]
    for _ in range(3):
        cands.append(np.nextafter(cands[-1], INF))
    c = x0
    for _ in range(3):
        c = np.nextafter(c, -INF)
        if c > vmin:
            cands.append(c)
    seen = set()
    for x2 in cands:
        x = np.full(ROWS, 5.0); x[lo] = vmin; x[other] = x2
        v, first, alone = _agree(x, tol=tol)
        assert v == vmin and alone == (not (x2 - np.float64(tol)) <= vmin)
        if x2 == vmin:
            assert first == min(lo, other)
        else:
            assert first == lo
        seen.add(alone)
    if tol > 0.0:
        assert seen == {True, False}                     # both sides of the edge were met


def test_a_third_value_in_the_band_of_a_wave_is_not_needed():
    """Three rows of one wave inside the band: only two of them are published, the record is "not alone" all the same; and with
    the second of a wave outside the band, no third of that wave can be inside."""
    x = np.full(ROWS, 5.0); x[[70, 80, 90]] = [1.0, 1.0 + TOL / 4, 1.0 + TOL / 2]
    assert _agree(x) == (1.0, 70, False)
    x[[80, 90]] = [1.0 + 2 * TOL, 1.0 + 3 * TOL]
    assert _agree(x) == (1.0, 70, True)


# ---------------------------------------------------------------------------------------------------------------------------
# the entering column under any partition of the columns
# ---------------------------------------------------------------------------------------------------------------------------
IMAX = 2 ** 31 - 1


def _feed(best, j, u, C):
    """rule_feed (lpx_scan.h), the rule that is not forced: ChooseEntering."""
    if j < C - 1 and u < best[0]:
        return (u, j)
    return best


def _sequential(row, eps):
    best = (-eps, IMAX)
    for j, u in enumerate(row):
        best = _feed(best, j, u, len(row))
    return best


def _partitioned(row, eps, g):
    C = len(row)
    # contiguous shares of a capacity >= C (shares past C are empty), each walked by `nt` lanes in strides; the lanes' results,
    # the waves' and the workgroups' are combined by mi_pick in a shuffled order
    cap = C + int(g.integers(0, 3 * C))
    nsel = int(g.integers(1, 33))
    per = (cap + nsel - 1) // nsel
    nt = int(g.choice([1, 2, 7, 64]))
    parts = []
    for b in range(nsel):
        j0, j1 = b * per, min(min(cap, (b + 1) * per), C)
        lanes = []
        for t in range(nt):
            best = (-eps, IMAX)
            for j in range(j0 + t, j1, nt):
                best = _feed(best, j, row[j], C)
            lanes.append(best)
        g.shuffle(lanes)
        acc = lanes[0]
        for y in lanes[1:]:
            acc = mi_pick(acc, y)
        parts.append(acc)
    order = g.permutation(nsel)
    acc = parts[order[0]]
    for k in order[1:]:
        acc = mi_pick(acc, parts[k])
    return acc


def test_entering_column_is_partition_independent():
    g = np.random.default_rng(5)
    eps = 1e-9
    for k in range(200):
        C = int(g.integers(2, 90))
        row = g.integers(-3, 3, C).astype(np.float64)                        # many repeated values, the minimum among them
        if k % 5 == 0:
            row = np.abs(row)                                                # nothing below -eps: no entering column
        if k % 7 == 0:
            row[C - 1] = -100.0                                              # the RHS column never enters
        want = _sequential(row, eps)
        assert _partitioned(row, eps, g) == want, (row, want)
        if want[1] != IMAX:
            assert want[1] == int(np.flatnonzero(row[:C - 1] == row[:C - 1].min())[0])
