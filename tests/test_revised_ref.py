"""oracle/revised_ref.py (the basis-only longdouble reference of the revised iteration) against oracle.revised_solve (the
faithful restatement that re-inverts the basis every iteration): the same status, trace, Bidx and Nidx exactly, x_B and z to
1e-12 relative, on small shapes and on the crafted tie instances.  This is what justifies comparing the GPU with the reference
at sizes the oracle cannot reach (tests/test_gpu_revised_shapes.py).  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _revised_cases as RC                     # noqa: E402
from oracle import revised_ref as R             # noqa: E402

REL = 1e-12


def _oracle_run(oracle, A, c, b, cap):
    """oracle.revised_solve takes a Max model: C = -c."""
    m = len(b)
    return oracle.revised_solve(oracle.Problem(oracle.MAX, -c, A, np.zeros(m, np.int32), b), max_iter=cap)


CASES = {
    "dense_1x3": lambda: RC.dense(1, 3, 1),
    "dense_2x5": lambda: RC.dense(2, 5, 2),
    "dense_12x20": lambda: RC.dense(12, 20, 3),
    "dense_64x40": lambda: RC.dense(64, 40, 4),
    "dense_257x300": lambda: RC.dense(257, 300, 5),
    "dense_300x120": lambda: RC.dense(300, 120, 6),
    "mixed_50x70": lambda: RC.mixed(50, 70, 7),
    "mixed_200x33": lambda: RC.mixed(200, 33, 8),
    "reentry_core": RC.reentry_core,
    "tie_core": RC.tie_core,
    "optimal_core": RC.optimal_core,
    "unbounded_core": RC.unbounded_core,
    "keep_small": lambda: RC.chain("keep_small"),
    "zero_ties_300": lambda: RC.ratio_chain(300, {17: 0.0, 18: 0.0, 250: 0.0}),
    "unclean_300": lambda: RC.ratio_chain(300, {100: 1.0 + 3e-13, 164: 1.0}),
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("cap", [3, 10000])
def test_reference_matches_the_oracle(oracle, name, cap):
    A, c, b = CASES[name]()
    ref = _oracle_run(oracle, A, c, b, cap)
    rr = R.RevisedRef(A, c, b)
    status = rr.run(cap)
    assert status == ref.status
    assert rr.trace == ref.trace.tolist()
    assert rr.Bidx == ref.Bidx.tolist() and rr.Nidx == ref.Nidx.tolist()
    scale = max(1.0, np.abs(ref.xB).max())
    assert np.abs(rr.xB - ref.xB).max() <= REL * scale
    assert abs(rr.z - ref.z_internal) <= REL * max(1.0, abs(ref.z_internal))


def test_crafted_instances_produce_their_events():
    """The records the GPU module relies on: key-order ties (winner with the larger column index), slack re-entries, an
    unbounded end on the crafted column, chains on both sides of every named segment boundary."""
    rr = R.RevisedRef(*RC.tie_core()); rr.run(10000)
    ev = rr.key_order_ties()
    assert any(t["winner_larger"] for t in ev) and any(not t["winner_larger"] for t in ev)
    rr = R.RevisedRef(*RC.reentry_core()); rr.run(10000)
    assert rr.status == R.OPTIMAL and len(rr.slack_reentries()) >= 2
    rr = R.RevisedRef(*RC.unbounded_core()); rr.run(10000)
    assert rr.status == R.UNBOUNDED and rr.steps[-1].q == 29 and len(rr.trace) >= 3 and rr.steps[-1].d.max() <= 1e-9
    rr = R.RevisedRef(*RC.optimal_core()); rr.run(10000)
    assert rr.status == R.OPTIMAL and 15 < len(rr.trace) <= 40
    band = []
    for name in RC.CHAINS:
        rr = R.RevisedRef(*RC.chain(name)); rr.run(1)
        band.append((rr.trace[0][0], rr.steps[0].ratio_band))
    for B in RC.BOUNDARIES:
        assert any(min([r] + bd) < B <= max([r] + bd) for r, bd in band if bd), B


def test_reference_binv_is_the_inverse():
    A, c, b = RC.mixed(50, 70, 7)
    rr = R.RevisedRef(A, c, b); rr.run(20)
    full = np.hstack([A, np.eye(50)])
    Binv = rr.binv()
    assert np.abs(Binv @ full[:, rr.Bidx] - np.eye(50)).max() <= 1e-12
    assert np.array_equal(rr.binv_rows(10, 30), Binv[10:30])
