"""The NumPy restatement of reduced-cost bound tightening (tests/_bnb_tighten_ref.py) against independent answers: the optimum of
the search by divers without it and of scipy.optimize.milp on binary_ip(16, 4), (24, 6) and (32, 8) under every flag set and
W = 1 and 4; strictly fewer nodes at W = 1 without flags; the general-integer instances, which reach t >= 1 and flipped columns
with a non-zero lower shift; and the defining property on every tightened node -- a twin handle that takes the reported triples as
an edit makes no event and no flip and ends with equal bounds.  CPU only; the GPU tests compare the device against this
restatement bit for bit."""
import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bnb_divers_ref as DV
import _bnb_tighten_ref as R
import _bounded_long_ref as L
from test_bnb_bounded_reference import milp

REL = 1e-9
INF = np.inf


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("flags", L.FLAG_SETS)
@pytest.mark.parametrize("n,m", R.IP_MODELS)
def test_same_optimum_as_the_search_without_tightening_and_as_milp(oracle, n, m, flags, W):
    c, A, b, up = R.ip_model(n, m)
    on = R.ip_search(n, m, W, flags)
    off = DV.solve_divers(c, A, b, up, W, search_flags=flags)
    st, want = milp(c, A, np.zeros(m), b, up)
    print("nodes", off["nodes"], "->", on["nodes"], "events", off["events"], "->", on["events"], "tightened", on["tightened_cols"],
          "on", on["tightened_nodes"], "nodes, optimum", on["value"], off["value"], want)
    assert on["rc"] == 0 and off["rc"] == 0 and on["status"] == off["status"] == st == L.OPTIMAL
    assert abs(on["value"] - off["value"]) <= REL * max(1.0, abs(off["value"]))
    assert abs(on["value"] - want) <= REL * max(1.0, abs(want))
    x = on["x"]
    assert np.array_equal(x, np.rint(x)) and (x >= 0).all() and (x <= 1).all() and (A @ x <= b + 1e-9).all()
    assert on["tightened_nodes"] >= 1 and on["tightened_cols"] >= on["tightened_nodes"] and on["max_per_node"] >= 1


@pytest.mark.parametrize("n,m", R.IP_MODELS)
def test_strictly_fewer_nodes_with_one_diver_and_no_flags(oracle, n, m):
    c, A, b, up = R.ip_model(n, m)
    on = R.ip_search(n, m, 1, 0)
    off = DV.solve_divers(c, A, b, up, 1)
    print("nodes", off["nodes"], "->", on["nodes"], "events", off["events"], "->", on["events"])
    assert on["nodes"] < off["nodes"]


def test_tightening_off_is_the_search_by_divers(oracle):
    c, A, b, up = R.ip_model(24, 6)
    for W in (1, 4):
        off = R.solve_tighten(c, A, b, up, W, tighten_on=False)
        want = DV.solve_divers(c, A, b, up, W)
        assert off["log"].tobytes() == want["log"].tobytes() and off["round"].tolist() == want["round"].tolist()
        assert off["tightened_nodes"] == 0 and _u64(off["x"]).tolist() == _u64(want["x"]).tolist()


@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("name", ["general", "lowers", "min"])
def test_general_integer_models_reach_the_optimum(oracle, name, W):
    c, A, rel, b, upper, lower, is_int, sense = N.small_models()[name]
    seen = {"t": 0.0, "flipped_lo": 0}

    def on_done(index, d, h, rec):
        fc, fl, fu = rec["fixed"]
        for j, l, u in zip(fc, fl, fu):
            seen["t"] = max(seen["t"], u - l)
            if h.flip[j] and l != 0.0:
                seen["flipped_lo"] += 1

    on = R.solve_tighten(c, A, b, upper, W, lower=lower, is_int=is_int, sense=sense, rel=rel, on_done=on_done)
    off = DV.solve_divers(c, A, b, upper, W, lower=lower, is_int=is_int, sense=sense, rel=rel)
    st, want = milp(c, A, rel, b, upper, lower, is_int, sense)
    print(name, "nodes", off["nodes"], "->", on["nodes"], "largest t", seen["t"], "flipped with a lower shift", seen["flipped_lo"])
    assert on["rc"] == 0 and on["status"] == st == L.OPTIMAL
    assert abs(on["value"] - off["value"]) <= REL * max(1.0, abs(off["value"]))
    assert abs(on["value"] - want) <= REL * max(1.0, abs(want))
    assert on["tightened_cols"] >= 1
    if W == 1:
        assert seen["t"] >= 1.0, "no column was tightened to a range of one or more"
        assert seen["flipped_lo"] >= 1, "no flipped column got a non-zero lower shift"


@pytest.mark.parametrize("case", [(16, 4, 1, 0), (24, 6, 4, 0), (32, 8, 1, L.LONG_STEP | L.CUTOFF_FLAG), "general", "lowers"])
def test_a_twin_that_takes_the_triples_as_an_edit_makes_no_event(oracle, case):
    """The defining property, on every tightened node of a whole search."""
    if isinstance(case, str):
        c, A, rel, b, upper, lower, is_int, sense = N.small_models()[case]
        kw = dict(lower=lower, is_int=is_int, sense=sense, rel=rel)
        W, flags, n = 1, 0, len(c)
    else:
        n, m, W, flags = case
        c, A, b, upper = R.ip_model(n, m)
        kw = {}
    twins, checked = {}, [0]

    def on_node(index, d, h, cols, lo, up, cutoff, fix_bound):
        twins[index] = (h.clone(), cols.copy(), lo.copy(), up.copy(), cutoff)

    def on_done(index, d, h, rec):
        twin, cols, lo, up, cutoff = twins.pop(index)
        fc, fl, fu = rec["fixed"]
        if not len(fc):
            return
        first = twin.node4(cols, lo, up, n, None, R.EPS, R.SKIP_FIXED | flags, cutoff)
        assert first["status"] == rec["status"] == L.OPTIMAL and _u64(first["z"]) == _u64(rec["z"])
        assert fc.tolist() == sorted(set(fc.tolist()))
        second = twin.node4(fc, fl, fu, n, None, R.EPS, R.SKIP_FIXED | flags, cutoff)
        assert (second["status"], second["events"], second["flips"]) == (L.OPTIMAL, 0, 0), second
        assert np.array_equal(_u64(twin.ub), _u64(h.ub)) and np.array_equal(_u64(twin.lo), _u64(h.lo))
        assert np.array_equal(_u64(twin.T), _u64(h.T)) and twin.basis.tolist() == h.basis.tolist()
        assert twin.flip.tolist() == h.flip.tolist()
        checked[0] += 1

    out = R.solve_tighten(c, A, b, upper, W, search_flags=flags, on_node=on_node, on_done=on_done, **kw)
    assert out["rc"] == 0 and checked[0] == out["tightened_nodes"] >= 1


def test_the_rule_leaves_basic_masked_and_cheap_columns_alone(oracle):
    c, A, b, up = R.ip_model(16, 4)
    root = R.ip_search(16, 4, 1, 0)["root"]
    h = R.Handle(root[0], root[1], root[2], root[3])
    z = float(h.T[-1, -1])
    m = h.T.shape[0] - 1
    d = h.T[m, :16]
    basic = np.isin(np.arange(16), h.basis)
    mask = np.ones(16, dtype=np.uint8)
    order = np.argsort(np.where(basic, -INF, d))
    big, second = int(order[-1]), int(order[-2])
    assert not basic[big] and not basic[second] and d[big] > d[second] > 1e-9 and h.ub[big] == 1.0
    gap = 0.5 * (d[big] + d[second])                          # only the largest reduced cost leaves less than one step
    mask[big] = 0
    ub0, lo0 = h.ub.copy(), h.lo.copy()
    fc, fl, fu = R.tighten(h, 16, mask, z, z - gap)
    assert len(fc) == 0 and np.array_equal(h.ub, ub0) and np.array_equal(h.lo, lo0)
    fc, fl, fu = R.tighten(h, 16, None, z, z - gap)
    assert fc.tolist() == [big] and h.ub[big] == 0.0 and fu[0] - fl[0] == 0.0
    for bound in (z, z + 1.0, -INF):                          # z <= fix_bound, and off
        g = R.Handle(root[0], root[1], root[2], root[3])
        assert len(R.tighten(g, 16, None, z, bound)[0]) == 0 and np.array_equal(g.ub, ub0)
