"""The fused group step (lpx_group_fused / lpx_group_fused_c, lpx_group_fused.hip) against the CPU oracle, bit for bit, in every
cache-policy form and at its edges: live rows R mod 3 (the tile has 3 rows), pivot rows in the last partial tile, leading dimensions
that are no multiple of 128, R on both sides of the select loops' 256-thread stride, live shapes below the handle's capacity, every
end state among members that go on running, more live nodes than one 64-slot chunk of the device-side compaction, the two halves
lpx_multi_run_begin / _end (rolling batches over two slots, runs carried over windows, both tableau buffers as final homes, handle
reuse, runs crossing between the halves and lpx_multi_run_some, the argument contract), profile mode, and one long single dual run.

What a bitwise comparison can and cannot see: the forms differ in the CACHE POLICY of their loads and stores, which leaves every
value the same, so no test here can tell a wrong policy from the right one.  What the forms do have apart is code -- the plain tile
and the per-row path in two instantiations, the row-block test of the mixed form -- and what that code can get wrong shows in the
bits: a row or column block skipped or written twice, the pivot row mishandled in a partial tile, a node dropped from or duplicated
in the device's live list, a record read at the wrong parity.

The switches that pick a form are read once per process, hence one child process per form (this file, run as a script).  Every child
proves that the fused path ran: lpx_multi_run_begin on the very handles returns 0 (it returns 1 exactly when the fused path is not
available and the two-launch kernels would have taken the group), and the single run's launch count is that of one launch per step.
No comparison has a tolerance.  Every property of the oracle's runs that a GPU part relies on is asserted from the oracle alone by
the tests that are not marked gpu."""
import functools
import hashlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT, RUNNING = 0, 1, 2, 3, 4
ASYNC_SLOTS = 4                                 # LPX_ASYNC_SLOTS of include/lpx.h
TILE_ROWS = 3                                   # UPDS_ROWS of lpx_tile.h

# Part A: (m, n, seed, rows turned into repaired >= rows), made as test_gpu_group_paths._group makes them
A_SPECS = [(2, 3, 1, 0), (3, 5, 2, 1), (4, 6, 3, 2), (17, 30, 12, 4), (18, 30, 13, 0), (19, 30, 14, 5), (40, 70, 4, 0),
           (40, 87, 5, 8), (40, 88, 6, 0), (85, 170, 7, 20), (86, 170, 8, 0), (255, 20, 9, 0), (256, 20, 10, 30), (257, 20, 11, 0)]
GUARDS = [(10000, 1), (3, 0), (0, 1)]           # (fdf_guard, cleanup) of the dual members, one pass over the group each
# Part B: these members of A in handles of capacity B_CAP, beside exact-capacity handles of the others
B_CAP = (200, 330)
B_SMALL = [(40, 70, 4, 0), (19, 30, 14, 5), (85, 170, 7, 20)]
B_EXACT = [(18, 30, 13, 0), (40, 88, 6, 0), (4, 6, 3, 2), (256, 20, 10, 30)]
# Part C: six members of A beside the hand-made end states and six members of part D's generator
C_FROM_A = [(4, 6, 3, 2), (17, 30, 12, 4), (18, 30, 13, 0), (40, 87, 5, 8), (86, 170, 8, 0), (257, 20, 11, 0)]
C_FROM_D = [0, 1, 2, 3, 4, 5]
C_CAPS = [10000, 12]
# Part D
D_COUNT = 130
D_PREFIXES = [64, 65, 128, 129]
D_SOME = (100, 40, 4)                           # lpx_multi_run_some: at most in flight, min_active while any wait, batch
# Part E
E_FROM_D = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
E_WIDTH, E_STEPS = 8, 5                         # an odd step count: lpx_multi_run_begin rounds it up to 6
# Part G
G_SPEC, G_GUARD, G_BATCH = (256, 20, 10, 30), (0, 1), 8

FORMS = {
    "cached": {"LPX_UPDATE_POLICY": "0"},
    "all-nt": {"LPX_UPDATE_POLICY": "1"},
    "mixed-1": {"LPX_UPDATE_POLICY": "2", "LPX_UPDATE_MIXMOD": "1"},
    "mixed-2": {"LPX_UPDATE_POLICY": "2", "LPX_UPDATE_MIXMOD": "2"},
    "mixed-5": {"LPX_UPDATE_POLICY": "2", "LPX_UPDATE_MIXMOD": "5"},
}
PROFILED = ("cached", "mixed-1")                # the forms whose child also runs part F
TWO_LAUNCH = {"LPX_GROUP_FUSED": "0"}           # the extra child of part E
FUZZ_ARGS = ("2", "3")                          # tests/fuzz_groups.py seed and trials: see test_fuzz_arguments_draw_a_large_group


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _ld(C_):
    return (C_ + 15) // 16 * 16                 # lpx_tableau_create


def _lp(m, n, seed, n_ge):
    """(T, basis, dual) as test_gpu_group_paths._group makes it."""
    from linear_programming_solver_lpr381_amd import synth
    c, A, b = synth.dense_lp(m, n, seed=seed)
    T, basis = synth.primal_tableau_from(c, A, b)
    if n_ge:
        g = np.random.Generator(np.random.PCG64(seed + 99))
        for i in g.choice(m, size=n_ge, replace=False):
            T[i, :n] *= -1.0
            T[i, -1] = -0.02 * T[i, -1]
    return T, basis, bool(n_ge)


def _d_lp(k):
    """Member k of part D."""
    from linear_programming_solver_lpr381_amd import synth
    m, n = 6 + k % 13, 8 + k % 17
    c, A, b = synth.dense_lp(m, n, seed=2000 + k)
    T, basis = synth.primal_tableau_from(c, A, b)
    if k % 2:
        g = np.random.Generator(np.random.PCG64(k))
        for i in g.choice(m, size=1 + k % 3, replace=False):
            T[i, :n] *= -1.0
            T[i, -1] = -0.02 * T[i, -1]
    return T, basis, bool(k % 2)


def _hand_made():
    """The infeasible dual tableau of test_gpu_dual.test_dual_infeasible, the "unbounded" and "ties" LPs of
    test_gpu_configs._small_lps, and the unbounded one once more as a dual member: ForceDualFeasibility gives up on its column, the
    dual loop has nothing to do and the clean-up finds it unbounded -- all three hops of the state machine in one launch."""
    from linear_programming_solver_lpr381_amd import synth
    out = [(np.array([[1.0, 1, 0, 1], [-1.0, 0, 1, -2], [-1.0, 0, 0, 0]]), np.array([1, 2], dtype=np.int32), True)]
    c = np.array([1.0, 1.0]); A = np.array([[1.0, -1.0], [-1.0, 0.5]]); b = np.array([1.0, 2.0])
    T, basis = synth.primal_tableau_from(c, A, b)
    out += [(T, basis, False), (T.copy(), basis.copy(), True)]
    c = np.array([3.0, 2.0, 1.0]); A = np.array([[1.0, 1.0, 0.0], [1.0, 0.0, 1.0], [1.0, 1.0, 1.0], [2.0, 1.0, 0.0]])
    b = np.array([4.0, 4.0, 4.0, 8.0])
    T, basis = synth.primal_tableau_from(c, A, b)
    out.append((T, basis, False))
    return out


def _oracle_run(O, lp, guard=GUARDS[0], max_iter=10000):
    """(status, trace, FDF pivots, clean-up pivots, final tableau, final basis) of the oracle."""
    T, basis, dual = lp
    Tr, br = T.copy(), basis.copy()
    if not dual:
        st, tr = O.primal_tableau(Tr, br, max_iter=max_iter)
        return st, tr, 0, 0, Tr, br
    st, tr, nf = O.dual_tableau(Tr, br, fdf_guard=guard[0], cleanup=guard[1], max_iter=max_iter)
    cl = 0
    if guard[1]:                                # the clean-up's pivots: what the same run without it does not make
        _, tr0, _ = O.dual_tableau(T.copy(), basis.copy(), fdf_guard=guard[0], cleanup=0, max_iter=max_iter)
        cl = len(tr) - len(tr0)
    return st, tr, nf, cl, Tr, br


def _digest(items):
    """sha256 over (status, pivots, FDF pivots, clean-up pivots, trace, tableau, basis) of every member, in order."""
    h = hashlib.sha256()
    for st, tr, nf, cl, T, basis in items:
        h.update(np.array([st, len(tr), nf, cl], dtype=np.int64).view(np.uint8))
        h.update(np.ascontiguousarray(tr, dtype=np.int32).view(np.uint8))
        h.update(np.ascontiguousarray(T, dtype=np.float64).view(np.uint8))
        h.update(np.ascontiguousarray(basis, dtype=np.int32).view(np.uint8))
    return h.hexdigest()


def _windows(pivots, steps):
    """Launches a run of `pivots` pivots needs, in windows of `steps`: launch l chooses pivot l + 1 and applies pivot l, so the run
    ends in launch `pivots`, the pivots + 1st."""
    return (pivots + 1 + steps - 1) // steps


def _roll(count, width, begin, end):
    """The two-slot rolling batch of host/bnb.cpp: begin(slot, members) starts a window, end(slot, members) returns their statuses.
    Returns (windows every member took part in, number of begin calls)."""
    waiting, sets, running, seen, begins = list(range(count)), [[], []], [False, False], [0] * count, 0

    def launch(s):
        nonlocal begins
        while waiting and len(sets[s]) < width:
            sets[s].append(waiting.pop(0))
        if sets[s]:
            begin(s, list(sets[s])); running[s] = True; begins += 1

    def land(s):
        st = end(s, list(sets[s])); running[s] = False
        for i in sets[s]:
            seen[i] += 1
        sets[s] = [i for i, x in zip(sets[s], st) if x == RUNNING]

    launch(0); launch(1)
    while any(running):
        for s in (0, 1):
            if running[s]:
                land(s); launch(s)
        assert begins < 10000
    return seen, begins


def _roll_expected(pivots, steps):
    """_roll as the oracle's pivot counts say it goes."""
    left = [_windows(p, steps) for p in pivots]

    def end(s, members):
        for i in members:
            left[i] -= 1
        return [RUNNING if left[i] > 0 else OPTIMAL for i in members]
    return _roll(len(pivots), E_WIDTH, lambda s, members: None, end)


@functools.lru_cache(maxsize=None)
def _reference():
    """Every LP of the file with its oracle runs, the digests the children must print and the counters that go with them."""
    from oracle import oracle as O
    O.build()
    O.lib()
    R = {"digest": {}, "count": {}}
    a_lps = {s: _lp(*s) for s in A_SPECS}
    a_refs = {}
    for g, guard in enumerate(GUARDS):
        for s in A_SPECS:
            a_refs[s, g] = a_refs[s, 0] if g and not a_lps[s][2] else _oracle_run(O, a_lps[s], guard)
        R["digest"]["A%d" % g] = _digest([a_refs[s, g] for s in A_SPECS])
    R["A"] = ([a_lps[s] for s in A_SPECS], [[a_refs[s, g] for s in A_SPECS] for g in range(len(GUARDS))])
    R["digest"]["F"] = R["digest"]["A0"]
    R["count"]["F.launches"] = max(len(a_refs[s, 0][1]) for s in A_SPECS)

    R["B"] = ([a_lps[s] for s in B_SMALL + B_EXACT], [a_refs[s, 0] for s in B_SMALL + B_EXACT])
    R["digest"]["B"] = _digest(R["B"][1])

    d_lps = [_d_lp(k) for k in range(D_COUNT)]
    d_refs = [_oracle_run(O, lp) for lp in d_lps]
    d_refs12 = [_oracle_run(O, lp, max_iter=12) for lp in d_lps]
    R["D"] = (d_lps, d_refs, d_refs12)
    for name in ("D.b4", "D.b64", "D.some"):
        R["digest"][name] = _digest(d_refs)
    R["digest"]["D.cap12"] = _digest(d_refs12)
    for n in D_PREFIXES:
        R["digest"]["D.%d" % n] = _digest(d_refs[:n])

    c_lps = _hand_made() + [a_lps[s] for s in C_FROM_A] + [d_lps[k] for k in C_FROM_D]
    R["C"] = (c_lps, {cap: [_oracle_run(O, lp, max_iter=cap) for lp in c_lps] for cap in C_CAPS})
    for cap in C_CAPS:
        R["digest"]["C%d" % cap] = _digest(R["C"][1][cap])

    e_lps = [a_lps[s] for s in A_SPECS] + [d_lps[k] for k in E_FROM_D]
    e_refs = [a_refs[s, 0] for s in A_SPECS] + [d_refs[k] for k in E_FROM_D]
    R["E"] = (e_lps, e_refs)
    R["digest"]["E.roll"] = _digest(e_refs)
    seen, begins = _roll_expected([len(r[1]) for r in e_refs], E_STEPS + 1)
    R["count"]["E.begins"] = begins
    R["count"]["E.carried"] = max(seen) - 1
    # handle reuse: the member of A with the longest run of an odd number of pivots (its final tableau is in the second buffer, the
    # buffers have traded places) takes another LP of its shape
    at = max(range(len(A_SPECS)), key=lambda i: len(e_refs[i][1]) if len(e_refs[i][1]) % 2 else -1)
    m, n, seed, n_ge = A_SPECS[at]
    lp = _lp(m, n, seed + 500, n_ge)
    R["E.reuse_at"] = at
    R["E.reuse"] = (lp, _oracle_run(O, lp))
    R["digest"]["E.reuse"] = _digest([R["E.reuse"][1]])
    # crossing paths: the three longest primal runs of A (one for _end -> _some, two for _some -> _begin / _end)
    longest = sorted((s for s in A_SPECS if not a_lps[s][2]), key=lambda s: -len(a_refs[s, 0][1]))[:3]
    R["E.cross"] = ([a_lps[s] for s in longest], [a_refs[s, 0] for s in longest])
    R["digest"]["E.cross1"] = _digest(R["E.cross"][1][:1])
    R["digest"]["E.cross2"] = _digest(R["E.cross"][1][1:])
    R["digest"]["T.some"] = R["digest"]["E.cross2"]
    # contract: three short members of D land although a second _begin was refused meanwhile; three more run after a refused
    # profile-mode _begin
    R["E.contract"] = ([d_lps[k] for k in (10, 11, 12, 13, 14, 15)], [d_refs[k] for k in (10, 11, 12, 13, 14, 15)])
    R["digest"]["E.contract"] = _digest(R["E.contract"][1])

    g_lp = a_lps[G_SPEC]
    R["G"] = (g_lp, a_refs[G_SPEC, GUARDS.index(G_GUARD)])
    R["digest"]["G"] = _digest([R["G"][1]])
    return R


def _expected_keys(form):
    R = _reference()
    if form == "two-launch":
        return ["T.some"]
    return [k for k in R["digest"] if k != "T.some" and (k != "F" or form in PROFILED)]


# ---------------------------------------------------------------------------------------------------------------------------
# the child: one process per form
# ---------------------------------------------------------------------------------------------------------------------------
class _Child:
    def __init__(self):
        import ctypes as C
        import linear_programming_solver_lpr381_amd as L
        self.C, self.L, self.lib = C, L, L._lib.lib()
        L._lib.check(self.lib.lpx_init(0))
        self.R = _reference()
        self.t0 = time.time()

    def opts(self, guard=GUARDS[0], **kw):
        """Both option records with resident = -1: no resident kernel whatever the environment says."""
        d = self.L._lib.default_opts
        return d(False, resident=-1, **kw), d(True, resident=-1, fdf_guard=guard[0], cleanup=guard[1], **kw)

    def handles(self, lps, cap=None):
        T = self.L.DeviceTableau
        return [T.with_capacity(lp[0], lp[1], *cap) if cap else T.from_host(lp[0], lp[1]) for lp in lps]

    def arrays(self, tabs, lps):
        C, k = self.C, len(tabs)
        return (C.c_void_p * k)(*[t._h for t in tabs]), (C.c_int * k)(*[int(lp[2]) for lp in lps]), (C.c_int * k)(), (self.L._lib.Stats * k)()

    def multi_run(self, tabs, lps, po, do):
        hs, dl, st, ss = self.arrays(tabs, lps)
        self.L._lib.check(self.lib.lpx_multi_run(hs, dl, len(tabs), self.C.byref(po), self.C.byref(do), st, ss))
        return list(st), ss

    def some(self, tabs, lps, po, do, min_active):
        hs, dl, st, ss = self.arrays(tabs, lps)
        self.L._lib.check(self.lib.lpx_multi_run_some(hs, dl, len(tabs), self.C.byref(po), self.C.byref(do), st, ss, min_active))
        return list(st), ss

    def begin(self, slot, tabs, lps, po, do, steps):
        hs, dl, _, _ = self.arrays(tabs, lps)
        return self.lib.lpx_multi_run_begin(slot, hs, dl, len(tabs), self.C.byref(po), self.C.byref(do), steps)

    def end(self, slot, count):
        st, ss = (self.C.c_int * count)(), (self.L._lib.Stats * count)()
        rc = self.lib.lpx_multi_run_end(slot, st, ss)
        return rc, list(st), ss

    def prove_fused(self, tabs, lps):
        """Proof of path for a group that has run: lpx_multi_run_begin takes these very handles (it goes through the same
        fused_prepare as the run did and returns 1 exactly when the fused path is not available)."""
        po, do = self.opts()
        assert self.begin(ASYNC_SLOTS - 1, tabs, lps, po, do, 2) == 0, "the fused path was not available for this group"
        rc, _, _ = self.end(ASYNC_SLOTS - 1, len(tabs))
        assert rc == 0

    def check(self, name, tabs, statuses, stats, refs):
        """Every member against its own oracle run; returns the digest of what the device left."""
        got = []
        for i, (t, (st, tr, nf, cl, Tr, br)) in enumerate(zip(tabs, refs)):
            Tg, bg = t.download()
            s = stats[i]
            have = (statuses[i], s.pivots, s.fdf_pivots, s.cleanup_pivots)
            assert have == (st, len(tr), nf, cl), (name, i, have, (st, len(tr), nf, cl))
            trg = t.trace()
            assert trg.tolist() == tr.tolist(), (name, i, "trace")
            assert bg.tolist() == br.tolist(), (name, i, "basis")
            assert np.array_equal(_bits(Tg), _bits(Tr)), (name, i, "tableau", int(np.sum(_bits(Tg) != _bits(Tr))))
            got.append((statuses[i], trg, s.fdf_pivots, s.cleanup_pivots, Tg, bg))
        print("DIGEST", name, _digest(got), "%.2f s" % (time.time() - self.t0), flush=True)

    def close(self, tabs):
        for t in tabs:
            t.close()

    # ---- parts ----
    def part_a(self, profile=False):
        lps, refs = self.R["A"]
        for g, guard in enumerate(GUARDS[:1] if profile else GUARDS):
            tabs = self.handles(lps)
            for t, lp in zip(tabs, lps):
                assert t.ld == _ld(lp[0].shape[1])
            po, do = self.opts(guard, batch=16, profile=1 if profile else 0)
            st, ss = self.multi_run(tabs, lps, po, do)
            self.check("F" if profile else "A%d" % g, tabs, st, ss, refs[g])
            if profile:
                assert ss[0].update_ms_sum > 0.0, ss[0].update_ms_sum
                print("COUNT F.launches", ss[0].update_launches, flush=True)
            self.prove_fused(tabs, lps)
            self.close(tabs)

    def part_b(self):
        lps, refs = self.R["B"]
        tabs = self.handles(lps[:len(B_SMALL)], cap=B_CAP) + self.handles(lps[len(B_SMALL):])
        for t in tabs[:len(B_SMALL)]:
            assert t.ld == _ld(B_CAP[1])
        po, do = self.opts()
        st, ss = self.multi_run(tabs, lps, po, do)
        self.check("B", tabs, st, ss, refs)
        self.prove_fused(tabs, lps)
        self.close(tabs)

    def part_c(self):
        lps, refs = self.R["C"]
        for cap in C_CAPS:
            tabs = self.handles(lps)
            po, do = self.opts(max_iter=cap)
            st, ss = self.multi_run(tabs, lps, po, do)
            self.check("C%d" % cap, tabs, st, ss, refs[cap])
            self.prove_fused(tabs, lps)
            self.close(tabs)

    def part_d(self):
        lps, refs, refs12 = self.R["D"]
        tabs = self.handles(lps)

        def fresh(n):
            for t, lp in zip(tabs[:n], lps[:n]):
                t.upload(lp[0], lp[1])

        for name, n, kw, want in ([("D.b4", D_COUNT, {"batch": 4}, refs), ("D.b64", D_COUNT, {"batch": 64}, refs),
                                   ("D.cap12", D_COUNT, {"batch": 64, "max_iter": 12}, refs12)]
                                  + [("D.%d" % n, n, {"batch": 64}, refs[:n]) for n in D_PREFIXES]):
            fresh(n)
            po, do = self.opts(**kw)
            st, ss = self.multi_run(tabs[:n], lps[:n], po, do)
            self.check(name, tabs[:n], st, ss, want)
            self.prove_fused(tabs[:n], lps[:n])
        # rolling batch through lpx_multi_run_some
        fresh(D_COUNT)
        width, min_active, batch = D_SOME
        po, do = self.opts(batch=batch)
        waiting, inflight, done, calls, suspended = list(range(D_COUNT)), [], {}, 0, 0
        while waiting or inflight:
            while waiting and len(inflight) < width:
                inflight.append(waiting.pop(0))
            st, ss = self.some([tabs[i] for i in inflight], [lps[i] for i in inflight], po, do, min_active if waiting else 0)
            calls += 1
            keep = []
            for j, i in enumerate(inflight):
                if st[j] == RUNNING:
                    keep.append(i); suspended += 1
                else:
                    done[i] = (st[j], self.copy_stats(ss[j]))
            inflight = keep
            assert calls < 400
        assert suspended > 0
        self.check("D.some", tabs, [done[i][0] for i in range(D_COUNT)], [done[i][1] for i in range(D_COUNT)], refs)
        self.prove_fused(tabs, lps)
        self.close(tabs)

    def copy_stats(self, s):
        c = self.L._lib.Stats()
        self.C.memmove(self.C.byref(c), self.C.byref(s), self.C.sizeof(c))
        return c

    def run_halves(self, slot, tabs, lps, po, do, steps, done):
        """Windows through _begin / _end in one slot until every member has ended; done[i] = (status, stats)."""
        live = [i for i in range(len(tabs)) if i not in done]
        n = 0
        while live:
            assert self.begin(slot, [tabs[i] for i in live], [lps[i] for i in live], po, do, steps) == 0
            rc, st, ss = self.end(slot, len(live))
            assert rc == 0
            for j, i in enumerate(live):
                if st[j] != RUNNING:
                    done[i] = (st[j], self.copy_stats(ss[j]))
            live = [i for j, i in enumerate(live) if st[j] == RUNNING]
            n += 1
            assert n < 400
        return n

    def part_e(self):
        lps, refs = self.R["E"]
        po, do = self.opts()
        # rolling batch over slots 0 and 1
        tabs = self.handles(lps)
        done = {}

        def begin(s, members):
            assert self.begin(s, [tabs[i] for i in members], [lps[i] for i in members], po, do, E_STEPS) == 0, (s, members)

        def end(s, members):
            rc, st, ss = self.end(s, len(members))
            assert rc == 0
            for j, i in enumerate(members):
                if st[j] != RUNNING:
                    done[i] = (st[j], self.copy_stats(ss[j]))
                else:           # the window ended where it started, rounded up to an even count: cumulative pivots
                    assert ss[j].pivots % (E_STEPS + 1) == 0 and ss[j].pivots > 0, (i, ss[j].pivots)
            return st

        seen, begins = _roll(len(lps), E_WIDTH, begin, end)
        self.check("E.roll", tabs, [done[i][0] for i in range(len(lps))], [done[i][1] for i in range(len(lps))], refs)
        assert seen == [_windows(len(r[1]), E_STEPS + 1) for r in refs], seen
        print("COUNT E.begins", begins, flush=True)
        print("COUNT E.carried", max(seen) - 1, flush=True)
        # handle reuse: a handle whose buffers have traded places takes another LP of the same shape
        at = self.R["E.reuse_at"]
        lp, ref = self.R["E.reuse"]
        tabs[at].upload(lp[0], lp[1])
        d = {}
        self.run_halves(0, [tabs[at]], [lp], po, do, E_STEPS, d)
        self.check("E.reuse", [tabs[at]], [d[0][0]], [d[0][1]], [ref])
        self.close(tabs)

        # crossing paths
        lps, refs = self.R["E.cross"]
        tabs = self.handles(lps)
        po4, do4 = self.opts(batch=4)
        assert self.begin(0, tabs[:1], lps[:1], po, do, E_STEPS) == 0
        rc, st, _ = self.end(0, 1)
        assert rc == 0 and st == [RUNNING], st                      # left unfinished by _end ...
        st, ss = self.some(tabs[:1], lps[:1], po4, do4, 0)           # ... it ends through lpx_multi_run_some
        self.check("E.cross1", tabs[:1], st, ss, refs[:1])
        st, ss = self.some(tabs[1:], lps[1:], po4, do4, 1)           # left unfinished by lpx_multi_run_some ...
        assert RUNNING in st, st
        d = {j: (st[j], self.copy_stats(ss[j])) for j in range(2) if st[j] != RUNNING}
        self.run_halves(1, tabs[1:], lps[1:], po, do, E_STEPS, d)    # ... it ends through _begin / _end
        self.check("E.cross2", tabs[1:], [d[j][0] for j in range(2)], [d[j][1] for j in range(2)], refs[1:])
        self.close(tabs)

        # contract
        lps, refs = self.R["E.contract"]
        tabs = self.handles(lps)
        first, second = slice(0, 3), slice(3, 6)
        assert self.begin(0, tabs[first], lps[first], po, do, 64) == 0
        assert self.begin(0, tabs[second], lps[second], po, do, 64) < 0          # the slot has a window in flight
        for slot in (-1, ASYNC_SLOTS):
            assert self.begin(slot, tabs[second], lps[second], po, do, 64) < 0
            assert self.end(slot, 3)[0] < 0
        assert self.end(1, 3)[0] < 0                                             # idle slot
        rc, st_a, ss_a = self.end(0, 3)                                          # the window still lands
        assert rc == 0
        assert self.end(0, 3)[0] < 0                                             # and the slot is idle again
        pp, dp = self.opts(profile=1)
        assert self.begin(0, tabs[second], lps[second], pp, dp, 64) == 1         # profile mode: not on this path
        for t, lp in zip(tabs[second], lps[second]):
            Tg, bg = t.download()
            assert np.array_equal(_bits(Tg), _bits(lp[0])) and bg.tolist() == lp[1].tolist()
        assert self.end(0, 3)[0] < 0                                             # nothing was started
        d = {}
        self.run_halves(0, tabs[second], lps[second], po, do, 64, d)
        self.check("E.contract", tabs, st_a + [d[j][0] for j in range(3)], [ss_a[j] for j in range(3)] + [d[j][1] for j in range(3)], refs)
        self.close(tabs)

    def part_g(self):
        lp, ref = self.R["G"]
        (t,) = self.handles([lp])
        _, do = self.opts(G_GUARD, batch=G_BATCH)
        s = self.L._lib.Stats()
        st = self.L._lib.check(self.lib.lpx_dual_run(t._h, self.C.byref(do), self.L._lib.NULL_CB, None, self.C.byref(s)))
        self.check("G", [t], [st], [s], [ref])
        # one launch per step (the fused path reports steps + 1; the two-launch kernels at least two launches per pivot)
        assert s.pivots >= 3 * G_BATCH and s.launches <= s.pivots + G_BATCH + 1, (s.pivots, s.launches)
        print("COUNT G.launches", s.launches, flush=True)
        self.close([t])

    def two_launch(self):
        """LPX_GROUP_FUSED=0: the halves are not available, and a run the two-launch kernels left unfinished is refused by them."""
        lps, refs = self.R["E.cross"]
        lps, refs = lps[1:], refs[1:]
        tabs = self.handles(lps)
        po, do = self.opts(batch=4)
        assert self.begin(0, tabs, lps, po, do, E_STEPS) == 1
        assert self.end(0, 2)[0] < 0
        st, ss = self.some(tabs, lps, po, do, 1)
        left = [j for j in range(2) if st[j] == RUNNING]
        assert left, st
        assert self.begin(0, [tabs[j] for j in left], [lps[j] for j in left], po, do, E_STEPS) < 0
        assert "suspended on the two-launch kernels" in self.L._lib.last_error(), self.L._lib.last_error()
        d = {j: (st[j], self.copy_stats(ss[j])) for j in range(2) if st[j] != RUNNING}
        n = 0
        while left:
            st, ss = self.some([tabs[j] for j in left], [lps[j] for j in left], po, do, 0)
            for k, j in enumerate(left):
                if st[k] != RUNNING:
                    d[j] = (st[k], self.copy_stats(ss[k]))
            left = [j for k, j in enumerate(left) if st[k] == RUNNING]
            n += 1
            assert n < 10
        self.check("T.some", tabs, [d[j][0] for j in range(2)], [d[j][1] for j in range(2)], refs)
        self.close(tabs)


def _child(form):
    c = _Child()
    if form == "two-launch":
        c.two_launch()
        return
    c.part_a()
    c.part_b()
    c.part_c()
    c.part_d()
    c.part_e()
    if form in PROFILED:
        c.part_a(profile=True)
    c.part_g()


# ---------------------------------------------------------------------------------------------------------------------------
# what the GPU parts rely on, from the oracle alone
# ---------------------------------------------------------------------------------------------------------------------------
def test_oracle_group_a_covers_the_tile_and_stride_edges():
    lps, refs = _reference()["A"]
    shapes = [lp[0].shape for lp in lps]
    assert {R % TILE_ROWS for R, _ in shapes} == {0, 1, 2}, shapes
    # a pivot row in the last, partial tile.  Only R = 3k + 2 can have one: with R = 3k + 1 the partial tile is the objective row
    # alone, which every update takes through the per-row path and which is never a pivot row.
    in_partial = [R for (R, _), ref in zip(shapes, refs[0]) if R % TILE_ROWS == 2 and (ref[1][:, 0] >= R - R % TILE_ROWS).any()]
    assert {5, 41, 86} <= set(in_partial), in_partial
    assert any(R % TILE_ROWS == 1 and len(ref[1]) > 0 for (R, _), ref in zip(shapes, refs[0]))
    assert {256, 257, 258} <= {R for R, _ in shapes}
    assert {256, 257} <= {C_ for _, C_ in shapes}                               # columns on both sides of the stride as well
    assert {_ld(C_) for _, C_ in shapes} == {16, 48, 64, 112, 128, 144, 256, 272, 288}
    assert sum(1 for _, C_ in shapes if _ld(C_) % 128) >= 4
    pivots = [len(ref[1]) for g in range(len(GUARDS)) for ref in refs[g]]
    assert min(pivots) == 1 and max(pivots) == 140, pivots
    # the three passes differ where they should: guard 3 stops ForceDualFeasibility after 3 pivots, guard 0 allows none
    dual = [i for i, lp in enumerate(lps) if lp[2]]
    assert len(dual) == 7
    cut = [i for i in dual if refs[0][i][2] > 3]
    assert len(cut) >= 4 and all(refs[1][i][2] == 3 == len(refs[1][i][1]) for i in cut)
    assert all(refs[1][i][2] == refs[0][i][2] for i in dual if i not in cut)
    assert all(refs[2][i][2] == 0 for i in dual) and any(refs[0][i][2] > 0 for i in dual)
    assert any(refs[0][i][3] > 0 or refs[2][i][3] > 0 for i in dual)            # some clean-up pivots
    # part B: the live shapes fit the capacity, with another leading dimension than their own
    lps_b, _ = _reference()["B"]
    for lp in lps_b[:len(B_SMALL)]:
        assert lp[0].shape[0] < B_CAP[0] and lp[0].shape[1] < B_CAP[1] and _ld(lp[0].shape[1]) != _ld(B_CAP[1])
    # part G: long enough for the launch count to tell one launch per step from two
    g = _reference()["G"][1]
    assert len(g[1]) == 46 and g[2] == 0 and len(g[1]) >= 3 * G_BATCH


def test_oracle_group_c_covers_every_end_state():
    lps, refs = _reference()["C"]
    assert len(lps) >= 12
    full, capped = refs[10000], refs[12]
    assert {r[0] for r in full} == {OPTIMAL, UNBOUNDED, INFEASIBLE}, [r[0] for r in full]
    assert [r[0] for r in full[:4]] == [INFEASIBLE, UNBOUNDED, UNBOUNDED, OPTIMAL]
    at_cap = [i for i, r in enumerate(capped) if r[0] == ITER_LIMIT]
    assert len(at_cap) >= 2 and len(at_cap) < len(lps) - 4, at_cap
    assert {r[0] for r in capped} == {OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT}
    # ends before the cap are the same ends
    for a, b in zip(full, capped):
        if b[0] != ITER_LIMIT:
            assert a[0] == b[0] and len(a[1]) == len(b[1])


def test_oracle_group_d_spreads_over_windows_and_chunks():
    lps, refs, refs12 = _reference()["D"]
    pivots = [len(r[1]) for r in refs]
    assert all(r[0] == OPTIMAL for r in refs)
    assert min(pivots) == 2 and max(pivots) == 18 and len(set(pivots)) == 16, sorted(set(pivots))
    assert {_windows(p, 4) for p in pivots} == {1, 2, 3, 4, 5}
    assert max(pivots[:64]) != max(pivots[64:])
    d = np.diff(pivots)
    assert (d > 0).any() and (d < 0).any()                                      # not monotone in k
    assert max(pivots) + 1 <= 64                                                # batch 64: everything ends inside one window
    # the launch in which the shortest run beyond slot 63 ends leaves runs going in both chunks of the compaction
    first_out = min(pivots[64:])
    assert any(p > first_out for p in pivots[:64]) and any(p > first_out for p in pivots[64:])
    assert sum(1 for r in refs12 if r[0] == ITER_LIMIT) == 11
    # the rolling run has something to suspend: when at most min_active of the first batch still run, some do
    width, min_active, batch = D_SOME
    w = 1
    while sum(1 for p in pivots[:width] if _windows(p, batch) > w) > min_active:
        w += 1
    assert sum(1 for p in pivots[:width] if _windows(p, batch) > w) > 0


def test_oracle_group_e_carries_runs_and_ends_in_both_buffers():
    R = _reference()
    lps, refs = R["E"]
    assert len(lps) == 24
    pivots = [len(r[1]) for r in refs]
    assert {p % 2 for p in pivots} == {0, 1}                                    # both buffers are final homes
    assert R["count"]["E.carried"] >= 2
    assert R["count"]["E.begins"] > 2 * ((len(lps) + E_WIDTH - 1) // E_WIDTH)   # fresh members join beside carried ones
    at = R["E.reuse_at"]
    assert 0 <= at < len(A_SPECS) and pivots[at] % 2 == 1
    lp, ref = R["E.reuse"]
    assert lp[0].shape == lps[at][0].shape and not np.array_equal(lp[0], lps[at][0]) and len(ref[1]) > 0
    # crossing paths: primal runs longer than two windows, of different lengths
    clps, crefs = R["E.cross"]
    cp = [len(r[1]) for r in crefs]
    assert all(not lp[2] for lp in clps) and min(cp) > 2 * (E_STEPS + 1) and cp[1] != cp[2], cp
    # contract: short enough to end inside one window of 64
    assert all(len(r[1]) + 1 <= 64 for r in R["E.contract"][1])


def _fuzz_counts(seed, trials):
    """The group sizes tests/fuzz_groups.py draws, by its own sequence of draws (no device needed)."""
    rng = np.random.default_rng(seed)
    out = []
    for trial in range(trials):
        count = int(rng.choice([1, 2, 3, 17, 64, 255, 256, 257, 400]))
        big, made = trial % 4 == 3, 0
        for k in range(count):
            m = int(rng.integers(200, 420)) if big else int(rng.integers(1, 40))
            rng.integers(300, 900) if big else rng.integers(1, 60)
            rng.integers(1, 1 << 30)
            if m > 1 and int(rng.integers(0, 2)):
                rng.integers(0, m)
            made += 1
            if big and k >= 40:
                break
        out.append(made)
    return out


def test_fuzz_arguments_draw_a_large_group():
    counts = _fuzz_counts(int(FUZZ_ARGS[0]), int(FUZZ_ARGS[1]))
    assert max(counts) >= 255, counts
    assert int(FUZZ_ARGS[1]) <= 3                                               # no trial of large shapes (every fourth)


# ---------------------------------------------------------------------------------------------------------------------------
# the parent side
# ---------------------------------------------------------------------------------------------------------------------------
def _run_child(form, env):
    R = _reference()
    env = dict(os.environ, PYTHONPATH=ROOT, LPX_RESIDENT_GROUP="0", **env)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), form], env=env, capture_output=True, text=True, timeout=120)
    print("%s: child took %.1f s" % (form, time.time() - t0))
    assert r.returncode == 0, form + ": " + r.stdout[-3000:] + r.stderr[-3000:]
    digests, counts = {}, {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[:1] == ["DIGEST"]:
            assert w[1] not in digests, line
            digests[w[1]] = w[2]
        elif w[:1] == ["COUNT"]:
            counts[w[1]] = int(w[2])
    want = _expected_keys(form)
    assert sorted(digests) == sorted(want), (form, sorted(digests))
    for k in want:
        assert digests[k] == R["digest"][k], (form, k)
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_fused_group_step_agrees_with_the_oracle_bit_for_bit(oracle, form):
    """One child per cache-policy form (LPX_RESIDENT_GROUP=0, resident = -1): parts A to E and G, part F in the cached and mixed-1
    children; every member of every group against its own oracle run in the child, the digests and counters again here."""
    R = _reference()
    counts = _run_child(form, FORMS[form])
    assert counts["E.begins"] == R["count"]["E.begins"] and counts["E.carried"] == R["count"]["E.carried"], counts
    assert counts["E.carried"] >= 2
    pivots = len(R["G"][1][1])
    assert pivots + 1 <= counts["G.launches"] <= pivots + G_BATCH + 1, counts
    if form in PROFILED:
        # launch l applies pivot l and the first applies none: the launches that updated are as many as the longest run has pivots
        assert counts["F.launches"] == R["count"]["F.launches"], counts


@pytest.mark.gpu
def test_halves_are_refused_where_the_two_launch_kernels_run(oracle):
    """LPX_GROUP_FUSED=0: lpx_multi_run_begin returns 1 on fresh handles, refuses a run that lpx_multi_run_some left unfinished on
    the two-launch kernels (the error of the suspended2 check), and that run ends through lpx_multi_run_some in the oracle's bits."""
    _run_child("two-launch", TWO_LAUNCH)


@pytest.mark.gpu
def test_randomized_group_sweep_on_the_fused_group_step(oracle):
    """tests/fuzz_groups.py with the resident group kernel off and the mixed store policy forced: its groups, one of them of 255
    or more members, go through lpx_group_fused."""
    env = dict(os.environ, PYTHONPATH=ROOT, LPX_RESIDENT_GROUP="0", LPX_UPDATE_POLICY="2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuzz_groups.py"), *FUZZ_ARGS], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "0 mismatches" in r.stdout
    assert r.stdout.count(": ok") == int(FUZZ_ARGS[1])


if __name__ == "__main__":
    _child(sys.argv[1])
