"""CPU checks of the restatement of strong branching by probes (tests/_bnb_probe_ref.py, the rule of lpx_solve_bnb_bounded6):
without the rule it is the search by divers log for log, with it every model reaches the optimum of scipy.optimize.milp, it
visits fewer nodes than the plain rule, a probe leaves its handle alone, and the counters add up."""
import functools

import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bnb_divers_ref as V
import _bnb_probe_ref as P
import _bounded_dual_ref as D
import _bounded_long_ref as L
from test_bnb_bounded_reference import milp

REL = 1e-9      # README "Parity bar": objectives reached by different pivot sequences agree within 1e-9 relative
LONG, CUT = L.LONG_STEP, L.CUTOFF_FLAG
BINARY = [(16, 8, 1), (24, 8, 1), (40, 10, 1)]


@functools.lru_cache(maxsize=None)
def _strong(n, m, seed, W=1, flags=0, cand_max=4, probe_iter=None, branching=1):
    c, A, b = N.binary_model(n, m, seed)
    return P.solve_strong(c, A, b, np.ones(n), W, search_flags=flags, branching=branching, cand_max=cand_max, probe_iter=probe_iter)


@functools.lru_cache(maxsize=None)
def _plain(n, m, seed, W=1, flags=0):
    c, A, b = N.binary_model(n, m, seed)
    return V.solve_divers(c, A, b, np.ones(n), W, search_flags=flags)


@pytest.mark.parametrize("W,flags", [(1, 0), (3, LONG | CUT)])
def test_without_the_rule_it_is_the_search_by_divers(W, flags):
    got, want = _strong(16, 8, 1, W, flags, branching=0), _plain(16, 8, 1, W, flags)
    assert got["log"].tobytes() == want["log"].tobytes() and len(got["log"]) > 50
    assert got["round"].tolist() == want["round"].tolist() and got["diver"].tolist() == want["diver"].tolist()
    for k in ("rc", "status", "nodes", "events", "flips", "incumbents", "pruned_bound", "pruned_infeasible", "max_K", "rounds", "steals"):
        assert got[k] == want[k], k
    assert np.float64(got["value"]).view(np.uint64) == np.float64(want["value"]).view(np.uint64)
    assert all(got[k] == 0 for k in P.SINFO_KEYS)


@pytest.mark.parametrize("n,m,seed", BINARY)
def test_strong_optimum_of_binary_programs_matches_milp(oracle, n, m, seed):
    c, A0, b0 = N.binary_model(n, m, seed)
    out = _strong(n, m, seed)
    st, want = milp(c, A0, np.zeros(m), b0, np.ones(n))
    print("optimum", out["value"], "milp", want, "nodes", out["nodes"], "plain", _plain(n, m, seed)["nodes"])
    assert out["rc"] == 0 and out["status"] == st == L.OPTIMAL
    assert abs(out["value"] - want) <= REL * max(1.0, abs(want))
    x = out["x"]
    assert np.array_equal(x, np.rint(x)) and (A0 @ x <= b0 + 1e-9).all()


@pytest.mark.parametrize("W,flags,cand_max,probe_iter", [(1, 0, 4, None), (3, LONG | CUT, 1, 4), (1, LONG | CUT, 4, 4)])
@pytest.mark.parametrize("name", ["general", "lowers", "min", "mixed", "infeasible"])
def test_strong_optimum_of_small_models_matches_milp(oracle, name, W, flags, cand_max, probe_iter):
    c, A, rel, b, upper, lower, is_int, sense = N.small_models()[name]
    out = P.solve_strong(c, A, b, upper, W, lower=lower, is_int=is_int, sense=sense, rel=rel, search_flags=flags, cand_max=cand_max,
                         probe_iter=probe_iter)
    st, want = milp(c, A, rel, b, upper, lower, is_int, sense)
    assert out["rc"] == 0 and out["status"] == st
    if st == L.OPTIMAL:
        assert abs(out["value"] - want) <= REL * max(1.0, abs(want))
    assert out["probe_launches"] == out["rounds"] and out["nodes"] == len(out["log"])


@pytest.mark.parametrize("n,m,seed", [(24, 8, 1), (40, 10, 1)])
def test_strong_visits_fewer_nodes_than_plain(n, m, seed):
    strong, plain = _strong(n, m, seed), _plain(n, m, seed)
    print("nodes", plain["nodes"], "->", strong["nodes"], "probes", strong["probes"], "pruned by probe", strong["pruned_by_probe"],
          "changed picks", strong["changed_picks"])
    assert strong["rc"] == plain["rc"] == 0
    assert strong["nodes"] < plain["nodes"]
    assert abs(strong["value"] - plain["value"]) <= REL * max(1.0, abs(plain["value"]))
    assert strong["changed_picks"] > 0 and strong["pruned_by_probe"] > 0
    assert strong["probes"] % 2 == 0 and 0 < strong["probes"] <= 8 * strong["nodes"]


def test_two_runs_give_identical_logs():
    c, A, b = N.binary_model(16, 8, 1)
    a = P.solve_strong(c, A, b, np.ones(16), 3, search_flags=LONG | CUT)
    again = P.solve_strong(c, A, b, np.ones(16), 3, search_flags=LONG | CUT)
    assert a["log"].tobytes() == again["log"].tobytes() and all(a[k] == again[k] for k in P.SINFO_KEYS)


def _root(n, m, seed):
    _, _, ub, _, Ts, bs, flip = D.root(n, m, seed)
    return L.Handle(Ts, bs, ub, flip), n


def test_probe_reads_its_handle_and_orders_its_candidates():
    h, n = _root(16, 8, 1)
    before = (h.T.tobytes(), h.basis.tobytes(), h.ub.tobytes(), h.lo.tobytes(), h.flip.tobytes())
    pr = P.probe(h, n, 32, 10000)
    assert before == (h.T.tobytes(), h.basis.tobytes(), h.ub.tobytes(), h.lo.tobytes(), h.flip.tobytes())
    want = N.pick(h.T, h.basis, h.flip, h.ub, h.lo, n)
    assert pr["candidates"] == want["candidates"] == pr["count"] >= 2 and len(pr["records"]) == 2 * pr["count"]
    assert pr["records"][0]["var"] == want["var"] and pr["records"][0]["x_var"] == want["x_var"]
    keys = []
    for c in range(pr["count"]):
        fl, ce = pr["records"][2 * c], pr["records"][2 * c + 1]
        assert (fl["var"], fl["dir"], ce["dir"]) == (ce["var"], 0, 1)
        assert (fl["lower"], fl["upper"], ce["lower"], ce["upper"]) == (0.0, 0.0, 1.0, 1.0)
        f = fl["x_var"] - np.floor(fl["x_var"])
        keys.append((abs(f - 0.5), fl["var"]))
        assert fl["z"] <= pr["z"] and ce["z"] <= pr["z"]                 # a child's bound is no better than its node's
    assert keys == sorted(keys)
    # a candidate's records do not depend on how many others are probed; the event limit is the child's
    one = P.probe(h, n, 1, 10000)
    assert one["count"] == 1 and one["candidates"] == pr["candidates"] and one["records"] == pr["records"][:2]
    none = P.probe(h, n, 4, 0)
    assert all(r["status"] == L.ITER_LIMIT and r["events"] == 0 for r in none["records"])
    # nothing to probe: pruned at z exactly (not one ulp below), or a handle whose last node did not end optimal
    assert P.probe(h, n, 4, 100, prune=pr["z"])["count"] == 0
    assert P.probe(h, n, 4, 100, prune=np.nextafter(pr["z"], -np.inf))["count"] == min(4, pr["candidates"])
    assert P.probe(h, n, 4, 100, last_status=L.INFEASIBLE) == {"count": 0, "candidates": 0, "z": pr["z"], "records": []}


def test_gain_score_and_dead_children():
    z = 10.0
    rec = lambda st, zz: {"status": st, "z": zz}
    assert P.gain(rec(L.INFEASIBLE, 0.0), z) == P.gain(rec(L.CUTOFF, 9.0), z) == 1e12
    assert P.gain(rec(None, 0.0), z) == 1e-6 and P.gain(rec(L.OPTIMAL, 10.0), z) == 1e-6
    assert P.gain(rec(L.ITER_LIMIT, 7.5), z) == 2.5 and P.gain(rec(L.OPTIMAL, -1e13), z) == 1e12
    pr = {"count": 3, "records": [rec(L.OPTIMAL, 9.0), rec(L.OPTIMAL, 8.0),        # 1 * 2
                                  rec(L.OPTIMAL, 8.0), rec(L.OPTIMAL, 8.0),        # 2 * 2: the first maximum
                                  rec(L.OPTIMAL, 6.0), rec(L.OPTIMAL, 9.0)]}       # 4 * 1
    assert P.choose(pr, z) == 1
    assert P.dead(rec(L.INFEASIBLE, 0.0), -np.inf) and P.dead(rec(L.CUTOFF, 0.0), -np.inf)
    assert P.dead(rec(L.OPTIMAL, 5.0 + 1e-6), 5.0) and not P.dead(rec(L.OPTIMAL, 5.1), 5.0)
    assert not P.dead(rec(L.ITER_LIMIT, 0.0), 5.0) and not P.dead(rec(None, 0.0), 5.0)
