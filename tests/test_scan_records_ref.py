"""The leaving-row scan from segment records (lpx_pivot_ratio's SelcRec, replayed by lpx_pivot_select), restated in NumPy.

The reference's ratio test is a sequential hysteresis chain: `if ratio < best - tol: best, row = ratio, i`.  The select-only pair
cuts the rows into segments (one per workgroup of the column launch), keeps per segment only

    v   the least ratio of the segment (+inf: no eligible row)
    i   the first row of that minimum, or -1 unless exactly one row of the segment has ratio - tol <= v

and replays the chain over those records (after a short cut: the least record alone in its band among the records); a segment
that the chain would enter and whose record says -1 hands over to the sequential rule from that segment's first row on, best and row carried.  This file checks that the three are the same function:
the sequential rule, the record + replay, for segment lengths 64, 256 (SELC_ROWS) and 1024 (64 x WH_PER), on random vectors
and on the vectors that can tell them apart -- exact ties and near-ties within tol inside a segment and across a segment
edge, +inf runs that fill whole segments, all-+inf vectors, and lengths on every side of a segment edge.  No GPU."""
import numpy as np
import pytest

TOL = 1e-9
SEGS = (64, 256, 1024)
INF = np.inf


def sequential(x, tol=TOL, start=0, best=INF, row=-1):
    """Models/PrimalSimplex.cs:229-241 over ratios that are +inf where the row is not eligible."""
    for i in range(start, len(x)):
        if x[i] < best - tol:
            best, row = x[i], i
    return row


def records(x, seg, tol=TOL):
    """One (v, i) per segment, with block_hysteresis_segments' expressions."""
    out = []
    for a in range(0, len(x), seg):
        s = x[a:a + seg]
        v = s.min()
        first = a + int(np.argmin(s))                   # first position of the minimum
        alone = int(np.count_nonzero((s - tol) <= v)) == 1
        out.append((v, first if alone else -1))
    return out


def replay(x, seg, tol=TOL):
    """The chain over the records; returns (row, segment where the exact scan took over or -1)."""
    best, row = INF, -1
    for k, (v, i) in enumerate(records(x, seg, tol)):
        if not (v < best - tol):
            continue
        if i < 0:
            return sequential(x, tol, k * seg, best, row), k
        best, row = v, i
    return row, -1


def replay_short_cut(x, seg, tol=TOL):
    """The row launch's form: when the least record is alone in its band among the records and its row alone in its segment,
    that row; else the chain above."""
    rec = records(x, seg, tol)
    v = np.array([r[0] for r in rec])
    g = v.min()
    k = int(np.argmin(v))
    if g < INF and np.count_nonzero((v - tol) <= g) == 1 and rec[k][1] >= 0:
        return rec[k][1], -2
    return replay(x, seg, tol)


def _lengths(seg):
    return (1, seg - 1, seg, seg + 1, 2 * seg, 4 * seg + 1)


def _vectors(seg, L, g):
    """Named vectors of length L for segment length seg."""
    base = g.uniform(1.0, 100.0, L)
    yield "random", base
    x = base.copy(); x[g.random(L) < 0.7] = INF
    yield "sparse", x
    yield "all-inf", np.full(L, INF)
    x = np.sort(base)[::-1].copy()                      # every row accepted in turn
    yield "descending", x
    yield "descending-within-tol", 5.0 - np.arange(L) * (TOL / 4)
    for d in (1, seg - 1, seg, seg + 1):
        if L <= d:
            continue
        for where in (0, max(0, seg - 2), max(0, L - d - 1)):
            if where + d >= L:
                continue
            for gap in (0.0, TOL / 2, TOL, 2 * TOL, -TOL / 2, -TOL, -2 * TOL):
                x = base.copy()
                x[where] = 0.5
                x[where + d] = 0.5 + gap               # a tie or near-tie at distance d: inside a segment or across its edge
                yield f"pair-d{d}-at{where}-gap{gap:g}", x
    if L > seg:                                         # whole segments of +inf in front of, between and behind the live ones
        x = base.copy(); x[:seg] = INF
        yield "inf-head", x
        x = base.copy(); x[seg:] = INF
        yield "inf-tail", x
        x = np.full(L, INF); x[-1] = 3.0
        yield "only-last", x
    if L > 2 * seg:
        x = base.copy(); x[seg:2 * seg] = INF; x[0] = 0.25; x[2 * seg] = 0.25
        yield "inf-middle-tie-across", x
    # zero-ratio degeneracy: many rows tied at 0, some inside the band above it
    x = base.copy()
    z = g.choice(L, size=max(1, L // 7), replace=False)
    x[z] = 0.0
    x[z[: len(z) // 3]] = g.choice([3e-10, 6e-10, 9e-10, 1.1e-9], size=len(z) // 3)
    yield "zeros", x
    # a clean early segment, then a later one whose minimum is lower by less than, exactly, and more than tol
    if L > seg:
        for gap in (TOL / 2, TOL, 2 * TOL):
            x = base.copy(); x[3 % seg] = 0.75; x[seg + (5 % (L - seg))] = 0.75 - gap
            yield f"later-lower-{gap:g}", x


@pytest.mark.parametrize("seg", SEGS)
def test_replay_equals_the_sequential_rule(seg):
    g = np.random.default_rng(seg)
    seen_tie = seen_clean = seen_short = 0
    for L in _lengths(seg):
        for name, x in _vectors(seg, L, g):
            want = sequential(x)
            got, tie = replay(x, seg)
            assert got == want, (seg, L, name, got, want, tie)
            got2, how = replay_short_cut(x, seg)
            assert got2 == want, (seg, L, name, got2, want, how)
            seen_tie += tie >= 0
            seen_clean += tie < 0
            seen_short += how == -2
    assert seen_tie > 20 and seen_clean > 20 and seen_short > 20       # every path ran


@pytest.mark.parametrize("seg", SEGS)
def test_records(seg):
    """What a record holds: +inf for a segment without eligible rows, -1 for a tied or near-tied minimum, the first row of a
    minimum that is alone in its band; the last segment may be short."""
    x = np.full(3 * seg + 1, INF)
    x[1] = 2.0; x[seg - 1] = 2.0 + 2 * TOL              # alone: the other one is outside the band
    x[2 * seg] = 1.0; x[2 * seg + 1] = 1.0              # exact tie
    x[3 * seg] = 7.0                                    # a segment of one row
    rec = records(x, seg)
    assert rec[0] == (2.0, 1) and rec[1][0] == INF and rec[2] == (1.0, -1) and rec[3] == (7.0, 3 * seg)
    x[seg - 1] = 2.0 + TOL / 2                          # inside the band
    assert records(x, seg)[0] == (2.0, -1)
    assert replay(np.full(5, INF), seg) == (-1, -1)     # nothing eligible: unbounded


def test_a_record_of_one_length_serves_any_other():
    """The chain is exact for every segment length, so three lengths agree with each other on shared inputs."""
    g = np.random.default_rng(7)
    for _ in range(200):
        L = int(g.integers(1, 3000))
        x = np.round(g.uniform(0, 3, L), int(g.integers(0, 3)))        # coarse values: many exact ties
        x[g.random(L) < 0.3] = INF
        x += g.choice([0.0, 3e-10, 1e-9], size=L)
        want = sequential(x)
        assert {replay(x, s)[0] for s in SEGS} | {replay_short_cut(x, s)[0] for s in SEGS} == {want}
