"""CPU pin of tests/_packed_ref.py, the restatement the GPU tests of lpx_solve_packed compare against: one 2 x 3 Min model with a
non-zero lower bound, a zero cost and one infinite upper bound, every number worked out by hand (all of them are exact in binary).

  Min -2 x1 + 0 x2 - 3 x3;  x1 + x2 + x3 <= 10,  x1 + 2 x3 <= 8;  l = (1, 0, 0.5), u = (inf, 2, 2).
  Preparation: c' = (2, -0, 3), objective row (-2, +0, -3 | 0);  b' = (10 - 1 - 0.5, 8 - 1 - 1) = (8.5, 6);  u' = (inf, 2, 1.5);
  c.l = -2 + -1.5 = -3.5.
  Event 1: q = 2 (-3), ratios (8.5, 3), u'_3 = 1.5 <= 3: flip.  RHS (7, 3 | 4.5), column 2 (-1, -2 | 3).
  Event 2: q = 0 (-2), ratios (7, 3): pivot (1, 0), kind 0.  Row 0 (0 1 1 1 -1 | 4), objective (0 0 -1 0 2 | 10.5).
  Event 3: q = 2 (-1), ratio row 0: 4, row 1 has a = -2 and an unbounded basic variable; u'_3 = 1.5 <= 4: flip back.
           RHS (2.5, 6 | 12), objective (0 0 1 0 2): optimal.
  x' = (6, 0, 0), x = (7, 0, 0.5), z = 12, value = -12 + -3.5 = -15.5, basis (3, 0), nothing at its upper bound."""
import numpy as np

import _packed_ref as P


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64).tolist()


def test_preparation_of_the_hand_model():
    c, A, b, lower, upper = P.hand_model()
    p = P.prepare(c, A, b, lower, upper, P.MIN)
    assert p.status == 0 and p.shifted and p.constant == -3.5
    want = np.array([[1.0, 1.0, 1.0, 1.0, 0.0, 8.5], [1.0, 0.0, 2.0, 0.0, 1.0, 6.0], [-2.0, 0.0, -3.0, 0.0, 0.0, 0.0]])
    assert _u64(p.T) == _u64(want)                      # bit for bit: the zero cost of a Min model is +0.0 in the objective row
    assert p.basis.tolist() == [3, 4] and _u64(p.ub) == _u64([np.inf, 2.0, 1.5, np.inf, np.inf])
    q = P.prepare(c, A, b, lower, upper, P.MAX)         # the same costs maximised: the zero cost is -0.0
    assert _u64(q.T[2]) == _u64([2.0, -0.0, 3.0, 0.0, 0.0, 0.0]) and q.constant == -3.5


def test_solution_of_the_hand_model():
    c, A, b, lower, upper = P.hand_model()
    s = P.solve(c, A, b, lower, upper, P.MIN)
    assert s.status == 0 and s.events == 3 and s.counts == (1, 0, 2)
    assert _u64(s.x) == _u64([7.0, 0.0, 0.5]) and s.value == -15.5 and s.z == 12.0
    assert s.basis.tolist() == [3, 0] and s.at_upper.tolist() == [0, 0, 0]
    for limit, events in ((0, 0), (1, 1), (2, 2), (3, 3)):          # the limit is tested first: 3 is still the limit
        t = P.solve(c, A, b, lower, upper, P.MIN, max_iter=limit)
        assert t.status == 3 and t.events == events
    t = P.solve(c, A, b, lower, upper, P.MIN, max_iter=1)           # stopped behind the flip: x3 sits at its upper bound
    assert _u64(t.x) == _u64([1.0, 0.0, 2.0]) and t.at_upper.tolist() == [0, 0, 1] and t.value == -4.5 + -3.5
    assert P.solve(c, A, b, lower, upper, P.MIN, max_iter=4).status == 0


def test_refusals_in_the_order_of_the_host_path():
    c, A, b, lower, upper = P.hand_model()
    for lo, up in ((np.array([1.0, -np.inf, 0.5]), upper), (np.array([1.0, np.nan, 0.5]), upper), (lower, np.array([np.inf, 2.0, 0.25])),
                   (lower, np.array([np.inf, np.nan, 2.0]))):
        s = P.solve(c, A, b, lo, up, P.MIN)
        assert s.status == P.EINVAL and not s.x.any() and s.value == 0.0 and s.counts == (0, 0, 0)
    s = P.solve(c, A, b, np.array([9.0, 0.0, 0.5]), upper, P.MIN)   # b'_2 = 8 - 9 - 1 = -2
    assert s.status == P.E_NEG_RHS and not s.x.any()
    s = P.solve(c, A, b, np.array([9.0, 0.0, 5.0]), upper, P.MIN)   # both defects: the bounds come first
    assert s.status == P.EINVAL
    s = P.solve(c, A, b, None, None, P.MIN)                         # no bounds: x3 enters first, then x1: x = (8, 0, 0), value -16
    assert s.status == 0 and _u64(s.x) == _u64([8.0, 0.0, 0.0]) and s.value == -16.0 and s.counts == (2, 0, 0)


def test_solve_all_reads_shared_and_batched_arrays_alike():
    c, A, b, lower, upper = P.hand_model()
    bs = np.stack([b, b + 1.0, b - 6.5])
    got = P.solve_all(c, A, bs, lower, upper, P.MIN)
    tiled = P.solve_all(np.tile(c, (3, 1)), np.tile(A, (3, 1, 1)), bs, np.tile(lower, (3, 1)), np.tile(upper, (3, 1)), P.MIN)
    assert len(got) == 3 and [g.status for g in got] == [0, 0, P.E_NEG_RHS]
    for g, t in zip(got, tiled):
        assert g.status == t.status and _u64(g.x) == _u64(t.x) and g.value == t.value and g.counts == t.counts
