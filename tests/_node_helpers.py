"""Helpers shared by the GPU tests of the branch-and-bound node (test_gpu_bounded_node_onchip.py, test_gpu_node_batch.py,
test_gpu_bounded_node_edges.py, and the pick tableaux of test_gpu_bnb_bounded.py): the bitwise views, what is read back from a
device handle, the comparison of a node record and of a handle with the NumPy restatement (tests/_bounded_long_ref.py), the
covering instances and the synthetic solved tableaux of the pick.  A plain module, no fixtures."""
import numpy as np

import _bounded_dual_ref as D
import _bounded_long_ref as L

INF = np.inf
SKIP, LONG, CUT = L.SKIP_FIXED, L.LONG_STEP, L.CUTOFF_FLAG
REC_KEYS = ("status", "events", "kind0", "kind1", "flips", "unrepairable", "var", "candidates")


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def bits(x):
    return np.float64(x).view(np.uint64)


def state(dt):
    Tg, bg = dt.download()
    lo, ub, flip = dt.bound_state()
    return (u64(Tg).tolist(), bg.tolist(), flip.tolist(), u64(ub).tolist(), u64(lo).tolist())


def reads(dt, n):
    """Everything the contract lets a caller read from a handle after a node."""
    x, z, up = dt.bounded_solution(n)
    return state(dt) + (dt.trace().tolist(), dt.bounded_counts(), u64(x).tolist(), int(bits(z)), np.asarray(up).tolist())


def same_record(got, want):
    assert {k: got[k] for k in REC_KEYS} == {k: want[k] for k in REC_KEYS}, (got, want)
    assert bits(got["x_var"]) == bits(want["x_var"]) and bits(got["z"]) == bits(want["z"]), (got, want)


def same_state(dt, h, what=""):
    """Tableau, basis, flip, ub and lo of the device handle against the restatement's handle, bit for bit."""
    Tg, bg = dt.download()
    glo, gub, gflip = dt.bound_state()
    assert np.array_equal(u64(Tg), u64(h.T)), "tableau bits differ from the restatement " + what
    assert bg.tolist() == h.basis.tolist(), what
    assert gflip.tolist() == h.flip.tolist(), what
    assert np.array_equal(u64(gub), u64(h.ub)) and np.array_equal(u64(glo), u64(h.lo)), what


def covering_fixed(n, seed):
    """Which structural columns covering_with_fixed fixes at 0: about a fifth of them."""
    return np.random.default_rng(seed).random(n) < 0.2


def covering_with_fixed(m, n, seed):
    T, basis, ub, _ = D.covering(m, n, seed)
    ub[:n][covering_fixed(n, seed)] = 0.0               # fixed columns: they do not enter
    return T, basis, ub


def fresh(lpx, T, basis, ub):
    dt = lpx.DeviceTableau.from_host(T, basis)
    dt.set_bounds(ub)
    return dt


def slack_handle(T, basis, ub):
    return L.Handle(T, basis, ub, np.zeros(len(ub), dtype=np.uint8))


def node(cols=(), lower=(), upper=()):
    return (np.asarray(cols, dtype=np.int32), np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64))


def ref_node(h, nd, n, flags=0, cutoff=None, **kw):
    return h.node2(*nd, n, flags=SKIP | flags | (0 if cutoff is None else CUT), cutoff=-INF if cutoff is None else cutoff, **kw)


def node3(dt, h, cols, lower, upper, n, flags=0, cutoff=None, form="onchip", other=None, is_int=None, **kw):
    """One node on the device in `form` and in the restatement: everything bit for bit.  other: a second device handle in the
    same state, which runs the node on the launches form and must end in the same state, counts included."""
    cols = np.atleast_1d(np.asarray(cols, dtype=np.int32))
    lower = np.broadcast_to(np.asarray(lower, dtype=np.float64), cols.shape)
    upper = np.broadcast_to(np.asarray(upper, dtype=np.float64), cols.shape)
    ref_kw = {k: v for k, v in kw.items() if k in ("eps", "max_iter")}
    want = h.node2(cols, lower, upper, n, is_int=is_int, flags=SKIP | flags | (0 if cutoff is None else CUT),
                   cutoff=-INF if cutoff is None else cutoff, **ref_kw)
    got = dt.bounded_node(cols, lower, upper, n, is_int=is_int, long_step=bool(flags & LONG), cutoff=cutoff, form=form, **kw)
    same_record(got, want)
    assert dt.trace().tolist() == h.trace.tolist()
    same_state(dt, h, "after the node")
    passes = want["events"] - want["kind0"] - want["kind1"]
    assert dt.bounded_counts() == (want["kind0"], want["kind1"], passes)
    if other is not None:
        ref = other.bounded_node(cols, lower, upper, n, is_int=is_int, long_step=bool(flags & LONG), cutoff=cutoff, form="launches", **kw)
        same_record(got, ref)
        assert dt.trace().tolist() == other.trace().tolist() and state(dt) == state(other)
        assert dt.bounded_counts() == other.bounded_counts()
    return got, want


FRACTIONS = np.array([0.0, 0.0, 0.0, 0.25, 0.75, 0.5, 0.125, 0.875, 1e-6, 1.0 - 1e-6, 2e-6, 0.4999, 0.3, 0.7])


def pick_tableau(nint, m, seed, extra=3):
    """A synthetic solved tableau: permutation basis, chosen RHS values, zero columns otherwise (bound edits and dual-feasibility
    flips then move the RHS of the objective row only).  Returns (T, basis, ub)."""
    g = np.random.default_rng(seed)
    Cm = nint + extra
    m = min(m, Cm)
    T = np.zeros((m + 1, Cm + 1))
    basis = g.permutation(Cm)[:m].astype(np.int32)
    T[np.arange(m), basis] = 1.0
    T[:m, Cm] = g.integers(0, 3, size=m) + g.choice(FRACTIONS, size=m)
    T[m, Cm] = 17.25
    ub = g.choice(np.array([1.0, 2.0, 3.0, INF]), size=Cm)
    return T, basis, ub


def exact(nint, entries, m_extra=0):
    """A tableau whose only non-integral values are `entries`: {column: value}."""
    cols = sorted(entries)
    m = len(cols) + m_extra
    Cm = nint + 1 + m_extra
    T = np.zeros((m + 1, Cm + 1))
    basis = np.array(cols + list(range(nint + 1, nint + 1 + m_extra)), dtype=np.int32)
    T[np.arange(m), basis] = 1.0
    T[:len(cols), Cm] = [entries[j] for j in cols]
    T[len(cols):m, Cm] = 2.0
    T[m, Cm] = -3.5
    return T, basis, np.full(Cm, INF)


class Pool:
    """Handles that are closed together."""

    def __init__(self):
        self.h = []

    def add(self, dt):
        self.h.append(dt)
        return dt

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for dt in self.h:
            dt.close()
