"""Every host path a group of LPs can take through lpx_multi_run and lpx_multi_run_some -- the resident group kernel, the fused
group step, the two-launch kernels (captured and eager) and the per-node loops -- on one small mixed group of four primal and
three dual LPs: each form ends in the oracle's tableaux, bases, statuses and pivot counts, bit for bit.  The switches that pick a
form are read once per process, hence one child process per form (this file, run as a script)."""
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (m, n, seed, rows turned into repaired >= rows): the shapes of test_multi_run_batched_mixed_group -- one and several 64-lane
# waves, one and several select workgroups.  The 20 x 30 LP has seed 3 instead of that test's 2: with 2 it takes 8 pivots, as
# many as the 8 x 12 one, and the seven runs are to differ in length (30, 57, 8, 13, 67, 31, 27 pivots).
SPECS = [(40, 60, 2, 0), (64, 100, 3, 0), (8, 12, 1, 0), (20, 30, 3, 5), (100, 160, 5, 30), (30, 45, 21, 0), (40, 64, 3, 10)]
BATCH = 8               # pivots per poll of the rolling run: a member with more than this many pivots can be suspended

FORMS = {
    "resident": {},
    "fused group": {"LPX_RESIDENT_GROUP": "0"},
    "two-launch": {"LPX_RESIDENT_GROUP": "0", "LPX_GROUP_FUSED": "0"},
    "two-launch eager": {"LPX_RESIDENT_GROUP": "0", "LPX_GROUP_FUSED": "0", "LPX_GRAPH": "0"},
    "per node": {"LPX_RESIDENT_GROUP": "0", "LPX_BATCHED": "0"},
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _group(O):
    """The seven LPs and their oracle runs: [(T, basis, dual)], [(status, trace, T_final, basis_final)]."""
    from linear_programming_solver_lpr381_amd import synth
    lps, refs = [], []
    for (m, n, seed, n_ge) in SPECS:
        c, A, b = synth.dense_lp(m, n, seed=seed)
        T, basis = synth.primal_tableau_from(c, A, b)
        if n_ge:
            g = np.random.Generator(np.random.PCG64(seed + 99))
            for i in g.choice(m, size=n_ge, replace=False):
                T[i, :n] *= -1.0
                T[i, -1] = -0.02 * T[i, -1]
        Tr, br = T.copy(), basis.copy()
        if n_ge:
            st, tr, _ = O.dual_tableau(Tr, br, fdf_guard=10000, cleanup=1)
        else:
            st, tr = O.primal_tableau(Tr, br)
        lps.append((T, basis, bool(n_ge)))
        refs.append((st, tr, Tr, br))
    return lps, refs


def _digest(results):
    """sha256 over (status, pivots, tableau, basis) of every member, in order."""
    h = hashlib.sha256()
    for status, pivots, T, basis in results:
        h.update(np.array([status, pivots], dtype=np.int64).view(np.uint8))
        h.update(np.ascontiguousarray(T, dtype=np.float64).view(np.uint8))
        h.update(np.ascontiguousarray(basis, dtype=np.int32).view(np.uint8))
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def _reference():
    from oracle import oracle as O
    O.build()
    O.lib()
    lps, refs = _group(O)
    return lps, refs, _digest([(st, len(tr), Tr, br) for st, tr, Tr, br in refs])


def _child():
    """Part 1: lpx_multi_run on the mixed group.  Part 2: the same seven through lpx_multi_run_some as a rolling batch."""
    import ctypes as C
    import linear_programming_solver_lpr381_amd as L
    lib = L._lib.lib()
    L._lib.check(lib.lpx_init(0))
    lps, refs, _ = _reference()
    dual = [d for _, _, d in lps]

    tabs = [L.DeviceTableau.from_host(T, basis) for T, basis, _ in lps]
    statuses, stats = L.multi_run(tabs, dual, dual_opts=L.default_opts(True, fdf_guard=10000, cleanup=1))
    one = []
    for i, (t, (st, tr, Tr, br)) in enumerate(zip(tabs, refs)):
        Tg, bg = t.download()
        assert statuses[i] == st and stats[i]["pivots"] == len(tr), (i, statuses[i], st, stats[i]["pivots"], len(tr))
        assert t.trace().tolist() == tr.tolist(), i
        assert np.array_equal(_bits(Tg), _bits(Tr)) and bg.tolist() == br.tolist(), i
        one.append((statuses[i], stats[i]["pivots"], Tg, bg))
        t.close()

    tabs = [L.DeviceTableau.from_host(T, basis) for T, basis, _ in lps]
    po = L._lib.default_opts(False, resident=-1, batch=BATCH)
    do = L._lib.default_opts(True, resident=-1, batch=BATCH, fdf_guard=10000, cleanup=1)
    waiting, inflight, done, calls, suspended_seen = list(range(len(tabs))), [], {}, 0, 0
    while waiting or inflight:
        while waiting and len(inflight) < 4:
            inflight.append(waiting.pop(0))
        k = len(inflight)
        hs = (C.c_void_p * k)(*[tabs[i]._h for i in inflight]); dl = (C.c_int * k)(*[int(dual[i]) for i in inflight])
        st = (C.c_int * k)(); ss = (L._lib.Stats * k)()
        L._lib.check(lib.lpx_multi_run_some(hs, dl, k, C.byref(po), C.byref(do), st, ss, 2 if waiting else 0))
        calls += 1
        keep = []
        for j, i in enumerate(inflight):
            if st[j] == 4:
                keep.append(i); suspended_seen += 1
            else:
                done[i] = (st[j], ss[j].pivots)
        inflight = keep
        assert calls < 200
    assert suspended_seen > 0                                           # the suspension path did run
    two = []
    for i, (t, (st, tr, Tr, br)) in enumerate(zip(tabs, refs)):
        Tg, bg = t.download()
        assert done[i] == (st, len(tr)), (i, done[i], st, len(tr))      # pivot counts are cumulative over the suspensions
        assert np.array_equal(_bits(Tg), _bits(Tr)) and bg.tolist() == br.tolist(), i
        two.append((done[i][0], done[i][1], Tg, bg))
        t.close()
    print("DIGEST", _digest(one), _digest(two), suspended_seen)


def test_oracle_runs_can_be_suspended():
    """What part 2 relies on, from the oracle alone: the seven runs differ in length, and at least one primal and one dual run
    is longer than one poll of BATCH pivots -- so a rolling batch with min_active > 0 has something to suspend."""
    lps, refs, _ = _reference()
    pivots = [len(tr) for _, tr, _, _ in refs]
    assert len(set(pivots)) == len(pivots), pivots
    assert max(p for p, (_, _, d) in zip(pivots, lps) if not d) > BATCH, pivots
    assert max(p for p, (_, _, d) in zip(pivots, lps) if d) > BATCH, pivots
    assert sum(1 for _, _, d in lps if d) == 3 and len(lps) == 7


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_group_paths_agree_with_the_oracle_bit_for_bit(oracle, form):
    """One child per form: lpx_multi_run on the mixed group (status, pivot count, trace, tableau, basis of every member against its
    own oracle run), then lpx_multi_run_some with at most 4 in flight, batch 8 and min_active 2 while any wait (suspensions
    asserted, pivot counts cumulative).  Both digests equal the oracle's, hence all forms print the same."""
    want = _reference()[2]
    env = dict(os.environ, PYTHONPATH=ROOT, **FORMS[form])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "DIGEST" in r.stdout, form + ": " + r.stdout + r.stderr
    got = r.stdout.split("DIGEST", 1)[1].split()
    assert got[0] == want and got[1] == want, (form, got, want)
    assert int(got[2]) > 0, (form, got)


if __name__ == "__main__":
    _child()
