"""The NumPy restatement of the packed branch and bound from a dual start (tests/_packed_bnb_dual_ref.py) against independent
answers: scipy.optimize.milp on every instance at the REL of test_bnb_bounded_reference.py, its root against
_packed_dual_ref.solve, record for record against a driver that carries a path per node, and every stop code and both INFEASIBLE
forms once.  CPU only; tests/test_gpu_packed_bnb_dual.py compares the device against this restatement."""
import numpy as np
import pytest

import _bnb_bounded_ref as N
import _bounded_long_ref as L
import _packed_bnb_dual_ref as R
import _packed_dual_ref as PD
from test_bnb_bounded_reference import REL

ALL = list(R.INSTANCES) + list(R.EDGES)
LAST = "edge 9x130 s1"          # it ends NODES by design


def milp(c, A, rel, b, upper, lower=None, is_int=None, sense=R.MAX):
    """(status, optimum in the user's sense) of scipy.optimize.milp over rows of both senses."""
    from scipy.optimize import Bounds, LinearConstraint, milp as _milp
    n = len(c)
    ge = np.asarray(rel) == R.GE
    res = _milp(c if sense == R.MIN else -np.asarray(c), constraints=LinearConstraint(A, np.where(ge, b, -np.inf), np.where(ge, np.inf, b)),
                integrality=np.ones(n) if is_int is None else np.asarray(is_int, dtype=float),
                bounds=Bounds(np.zeros(n) if lower is None else lower, upper))
    if res.status == 2:
        return R.INFEASIBLE, None
    assert res.status == 0, res.message
    return R.OPTIMAL, (res.fun if sense == R.MIN else -res.fun)


def solve_paths(c, A, rel, b, upper, lower=None, is_int=None, sense=R.MAX, search_flags=0, max_iter=10000):
    """The second driver: _bounded_long_ref.solve2's loop, a path per node, behind the root of _bounded_long_ref.solve_bounded_dual."""
    n = len(c)
    mask = None if is_int is None else np.asarray(is_int, dtype=np.uint8)
    root = L.solve_bounded_dual(c, A, rel, b, upper, lower, sense, flags=search_flags & L.LONG_STEP, max_iter=max_iter)
    out = {"status": root["status"], "x": None, "value": 0.0, "nodes": 0, "events": 0, "flips": 0, "incumbents": 0,
           "pruned_bound": 0, "pruned_infeasible": 0, "max_K": 0, "constant": root["constant"], "log": np.zeros(0, dtype=N.LOG_DTYPE)}
    if root["status"] != R.OPTIMAL:
        return out
    h = L.Handle(root["T"], root["basis"], root["ub"], root["flip"])
    root_lo, root_ub = np.zeros(n), root["ub"][:n].copy()
    cur_lo, cur_ub = root_lo.copy(), root_ub.copy()
    best, best_x = -np.inf, None
    stack = [(0, [])]
    log = []
    while stack:
        depth, path = stack.pop()
        out["nodes"] += 1
        nb_lo, nb_ub = root_lo.copy(), root_ub.copy()
        for var, l, u in path:
            nb_lo[var], nb_ub[var] = l, u
        cols = np.flatnonzero((nb_lo != cur_lo) | (nb_ub != cur_ub)).astype(np.int32)
        cutoff = best + L.EPS if search_flags & L.CUTOFF_FLAG else -np.inf
        rec = h.node2(cols, nb_lo[cols], nb_ub[cols], n, mask, L.EPS, L.SKIP_FIXED | search_flags, cutoff, max_iter=max_iter)
        assert rec["status"] not in (None, R.ITER_LIMIT)
        cur_lo, cur_ub = nb_lo, nb_ub
        out["events"] += rec["events"]; out["flips"] += rec["flips"]; out["max_K"] = max(out["max_K"], len(cols))
        log.append((depth, len(cols), rec["status"], rec["events"], rec["flips"], rec["var"], rec["z"]))
        if rec["status"] == R.INFEASIBLE:
            out["pruned_infeasible"] += 1
        elif rec["status"] == R.CUTOFF or rec["z"] <= best + L.EPS:
            out["pruned_bound"] += 1
        elif rec["var"] < 0:
            x = N.values(h.T, h.basis, h.flip, h.ub, h.lo, n).copy()
            ints = np.ones(n, dtype=bool) if mask is None else mask != 0
            x[ints] = np.rint(x[ints])
            best, best_x = rec["z"], x
            out["incumbents"] += 1
        else:
            v, xv = rec["var"], rec["x_var"]
            stack.append((depth + 1, path + [(v, nb_lo[v], np.floor(xv))]))
            stack.append((depth + 1, path + [(v, np.ceil(xv), nb_ub[v])]))
    out["log"] = np.array(log, dtype=N.LOG_DTYPE)
    if best_x is None:
        out["status"] = R.INFEASIBLE
        return out
    x = best_x + lower if lower is not None else best_x
    value = -best if sense == R.MIN else best
    if lower is not None and np.any(np.asarray(lower) != 0.0):
        value = value + root["constant"]
    out.update(status=R.OPTIMAL, x=x, value=float(value))
    return out


def _instance(name):
    return (R.INSTANCES.get(name) or R.EDGES[name])[0]


@pytest.mark.parametrize("name", ALL)
def test_every_instance_agrees_with_milp(oracle, name):
    c, A, rel, b, upper, lower, is_int, sense = _instance(name)
    st, want = milp(c, A, rel, b, upper, lower, is_int, sense)
    for flags in L.FLAG_SETS:
        out = R.ref(name, flags)
        print(name, flags, "status", out["status"], "stop", out["stop"], "nodes", out["nodes"], "deepest", out["deepest"],
              "infeasible nodes", out["pruned_infeasible"], "value", out["value"], "milp", want)
        if name == LAST:
            assert (out["status"], out["stop"], out["nodes"]) == (R.ITER_LIMIT, R.NODES, 200) and st == R.OPTIMAL
            # the incumbent so far is a point of the model, no better than the optimum (Min)
            assert out["incumbents"] > 0 and (A @ out["x"] >= b - 1e-9).all() and out["value"] >= want - REL * abs(want)
            continue
        assert out["stop"] == (R.ROOT if out["nodes"] == 0 else R.DONE) and out["status"] == st
        if st == R.OPTIMAL:
            assert abs(out["value"] - want) <= REL * max(1.0, abs(want))
            x = out["x"]
            ints = np.ones(len(c), dtype=bool) if is_int is None else np.asarray(is_int) != 0
            assert np.array_equal(x[ints], np.rint(x[ints]))
            assert out["nodes"] > 1 or name == "sweep f=1"      # that root is integral: one node
        else:
            assert not out["x"].any() and out["value"] == 0.0 and out["incumbents"] == 0 and out["best"] == -np.inf


def test_the_instances_take_every_path(oracle):
    """What the issue names for orientation, asserted as presence, not as numbers: infeasible nodes in every mixed_rows model,
    in eq_pair and in the sweep's middle, none at its ends; root dualize flips in mixed_rows; both INFEASIBLE forms."""
    for s in (1, 2, 3):
        out = R.ref("mixed_rows s%d" % s, 0)
        assert out["pruned_infeasible"] > 0 and out["root_flips"] > 0 and out["nodes"] > 1
        assert R.ref("mixed_general s%d" % s, 0)["nodes"] > 1
    eq = R.ref("eq_pair", 0)
    assert (eq["status"], eq["stop"], eq["incumbents"]) == (R.INFEASIBLE, R.DONE, 0) and eq["nodes"] > 1
    assert eq["pruned_infeasible"] > 0 and eq["pruned_infeasible"] + eq["pruned_bound"] < eq["nodes"]
    ri = R.ref("root_infeasible", 0)
    assert (ri["status"], ri["stop"], ri["nodes"], ri["logged"]) == (R.INFEASIBLE, R.ROOT, 0, 0) and ri["root_events"] > 0
    inf = [R.ref("sweep f=%g" % f, 0)["pruned_infeasible"] for f in R.SWEEP_F]
    assert inf[0] == 0 and inf[4] == 0 and all(1 <= k <= 10 for k in inf[1:4])
    assert R.ref("sweep f=1.05", 0)["stop"] == R.ROOT
    assert R.ref("edge 1x1 s1", 0)["pruned_infeasible"] == 1 and R.ref("edge 1x1 s1", 0)["nodes"] == 3
    assert R.ref("edge 3x65 s2", 0)["deepest"] > 20


@pytest.mark.parametrize("name", ["cover 6x12 s1", "mixed_rows s2", "mixed_general s3", "eq_pair", "root_infeasible",
                                  "sweep f=1.05", "edge 65x5 s1"])
def test_the_root_is_the_packed_dual_call(oracle, name):
    c, A, rel, b, upper, lower, is_int, sense = _instance(name)
    for flags in L.FLAG_SETS:
        out = R.ref(name, flags)
        want = PD.solve(c, A, b, rel, lower, upper, sense, long_step=bool(flags & L.LONG_STEP))
        assert out["root_status"] == want.status and out["root_events"] == want.events and out["root_flips"] == want.dualize_flips
        assert np.float64(out["root_z"]).tobytes() == np.float64(want.z).tobytes()


@pytest.mark.parametrize("flags", L.FLAG_SETS)
@pytest.mark.parametrize("name", [k for k in ALL if k != LAST])
def test_one_path_array_is_a_path_per_node(oracle, name, flags):
    c, A, rel, b, upper, lower, is_int, sense = _instance(name)
    out = R.ref(name, flags)
    want = solve_paths(c, A, rel, b, upper, lower, is_int, sense, flags)
    assert out["status"] == want["status"]
    for k in R.COUNTERS:
        assert out[k] == want[k], k
    assert out["log"].tobytes() == want["log"].tobytes() and out["constant"] == want["constant"]
    if want["status"] == R.OPTIMAL:
        assert out["x"].tobytes() == want["x"].tobytes() and out["value"] == want["value"]


def test_refusals_in_their_order(oracle):
    c, A, rel, b, upper, lower, is_int, sense = R.cover(4, 8, 1)
    cont = np.zeros(8, dtype=np.uint8)
    bad_rel = rel.copy(); bad_rel[2] = R.EQ
    cases = ((dict(upper=np.full(8, -1.0), is_int=cont), "bound"), (dict(lower=np.full(8, np.nan)), "bound"),
             (dict(upper=np.full(8, 1.5)), "integer"), (dict(upper=np.full(8, np.inf)), "integer"),
             (dict(lower=np.full(8, 0.5), upper=np.full(8, 1.5)), "integer"), (dict(rel=bad_rel), "rel"),
             # a bad bound in front of a bad integer bound in front of a bad rel
             (dict(upper=np.r_[-1.0, np.full(7, 1.5)], rel=bad_rel), "bound"), (dict(upper=np.full(8, 1.5), rel=bad_rel), "integer"))
    for kw, why in cases:
        args = dict(rel=rel, upper=upper, lower=None, is_int=None); args.update(kw)
        out = R.solve(c, A, b, sense=sense, **args)
        assert (out["status"], out["stop"], out["nodes"], out["why"]) == (R.EINVAL, R.ROOT, 0, why), (kw, out["why"])
        assert not out["x"].any() and out["best"] == -np.inf and out["root_events"] == 0
    # the precheck can only name a continuous variable: Max with a positive cost, no upper bound, the variable continuous
    mask = np.ones(8, dtype=np.uint8); mask[3] = 0
    up = upper.copy(); up[3] = np.inf
    out = R.solve(c, A, b, rel, up, None, mask, R.MAX)
    assert (out["status"], out["stop"], out["why"]) == (R.EINVAL, R.ROOT, "precheck")
    assert R.solve(c, A, b, bad_rel, up, None, mask, R.MAX)["why"] == "rel"             # rel in front of the precheck
    assert R.solve(c, A, b, rel, up, None, mask, R.MIN)["status"] == R.OPTIMAL          # Min: the column does not improve


def test_every_stop_code_once(oracle):
    c, A, rel, b, upper, lower, is_int, sense = R.mixed_rows(2)
    full = R.solve(c, A, b, rel, upper, sense=sense)
    n_nodes, n_events, deepest = full["nodes"], full["events"], full["deepest"]
    assert (full["status"], full["stop"]) == (R.OPTIMAL, R.DONE) and n_nodes > 50 and full["logged"] == n_nodes

    one = R.solve(c, A, b, rel, upper, sense=sense, max_nodes=1)
    assert (one["status"], one["stop"], one["nodes"], one["incumbents"], one["logged"]) == (R.ITER_LIMIT, R.NODES, 1, 0, 1)
    assert one["value"] == 0.0 and not one["x"].any() and one["log"].tobytes() == full["log"][:1].tobytes()
    short = R.solve(c, A, b, rel, upper, sense=sense, max_nodes=n_nodes - 1)
    assert (short["status"], short["stop"], short["nodes"]) == (R.ITER_LIMIT, R.NODES, n_nodes - 1) and short["incumbents"] > 0
    assert short["log"].tobytes() == full["log"][:n_nodes - 1].tobytes() and short["x"].any()

    done = np.cumsum(full["log"]["events"])
    half = int(n_events // 2)
    ev = R.solve(c, A, b, rel, upper, sense=sense, max_events=half)
    k = int(np.searchsorted(done, half)) + 1
    assert (ev["status"], ev["stop"], ev["nodes"], ev["events"]) == (R.ITER_LIMIT, R.EVENTS, k, int(done[k - 1])) and k < n_nodes
    assert ev["log"].tobytes() == full["log"][:k].tobytes()

    assert R.solve(c, A, b, rel, upper, sense=sense, max_depth=deepest)["log"].tobytes() == full["log"].tobytes()
    shallow = R.solve(c, A, b, rel, upper, sense=sense, max_depth=deepest - 1)
    first = int(np.flatnonzero((full["log"]["depth"] == deepest - 1) & (full["log"]["var"] >= 0))[0])
    assert (shallow["status"], shallow["stop"], shallow["nodes"]) == (R.ITER_LIMIT, R.DEPTH, first + 1)
    assert shallow["log"].tobytes() == full["log"][:first + 1].tobytes()

    # a node's own iteration limit: the busiest node makes more events than the root, so the root passes; the search stops at the
    # first node that would make busiest - 1 events or more
    busiest = int(full["log"]["events"].max())
    node = int(np.flatnonzero(full["log"]["events"] >= busiest - 1)[0])
    assert busiest > full["root_events"]
    lim = R.solve(c, A, b, rel, upper, sense=sense, max_iter=busiest - 1)
    assert (lim["status"], lim["stop"], lim["nodes"]) == (R.ITER_LIMIT, R.NODE_ITER, node + 1)
    assert lim["log"]["status"][-1] == R.ITER_LIMIT and lim["log"]["events"][-1] == busiest - 1
    assert lim["log"][:node].tobytes() == full["log"][:node].tobytes()
    # the root's: x and value as the packed dual call extracts them
    root = R.solve(c, A, b, rel, upper, sense=sense, max_iter=1)
    want = PD.solve(c, A, b, rel, None, upper, sense, long_step=False, max_iter=1)
    assert (root["status"], root["stop"], root["root_events"], root["nodes"]) == (R.ITER_LIMIT, R.ROOT, 1, 0)
    assert want.status == R.ITER_LIMIT and root["x"].tobytes() == want.x.tobytes() and root["value"] == want.value

    capped = R.solve(c, A, b, rel, upper, sense=sense, log_cap=10)
    assert capped["logged"] == 10 and capped["nodes"] == n_nodes and capped["log"].tobytes() == full["log"][:10].tobytes()

    # every stop code a search can produce.  REFUSED is not among them: a child's bounds lie inside its parent's, so no edit of a
    # search gives a flipped column the upper bound +inf, and every integer column has a finite one for the flips
    stops = {R.ref(k, 0)["stop"] for k in ALL} | {one["stop"], ev["stop"], shallow["stop"], lim["stop"]}
    assert stops == {R.DONE, R.ROOT, R.NODES, R.NODE_ITER, R.EVENTS, R.DEPTH}


def test_solve_all_shares_what_has_no_batch_axis(oracle):
    insts = R.sweep()
    c, A, rel = insts[0][0], insts[0][1], insts[0][2]
    bs = np.stack([i[3] for i in insts])
    outs = R.solve_all(c, A, bs, rel, 1.0, sense=R.MIN)
    assert len(outs) == len(R.SWEEP_F)
    for o, f in zip(outs, R.SWEEP_F):
        w = R.ref("sweep f=%g" % f, 0)
        assert o["log"].tobytes() == w["log"].tobytes() and o["value"] == w["value"] and o["status"] == w["status"]
