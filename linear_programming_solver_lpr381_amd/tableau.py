"""Device-resident simplex tableau: thin Python face of the lpx_tableau_* C ABI (include/lpx.h)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import RunOpts, Stats, check, default_opts, dp, ip, lib

PivotCallback = Callable[[int, int, int], None]


def _wrap_cb(cb: Optional[PivotCallback]):
    if cb is None:
        return _lib.NULL_CB
    return _lib.PIVOT_CB(lambda _user, it, r, q: cb(it, r, q))


@dataclass
class TableauRanging:
    """lpx_tableau_ranging of a device tableau (include/lpx.h): the column ratio test along the RHS column for every
    column j < C-1 (col_*), the row ratio test along the objective row over the nonbasic columns for every row r < m
    (row_*), and the two scalars that tell whether the basis is primal / dual feasible.  *_at: -1 where the set is empty."""
    col_inc: np.ndarray
    col_inc_at: np.ndarray
    col_dec: np.ndarray
    col_dec_at: np.ndarray
    row_inc: np.ndarray
    row_inc_at: np.ndarray
    row_dec: np.ndarray
    row_dec_at: np.ndarray
    min_rhs: float
    min_dj: float


class DeviceTableau:
    """A simplex tableau living in HBM (row-major, padded leading dimension).

    Layout follows Models/PrimalSimplex.cs:179-203: R = m+1 rows, objective row last;
    C = n+m+1 columns, RHS last; basis[i] = column basic in row i.
    """

    def __init__(self, R: int, C_: int):
        self._h = C.c_void_p()
        check(lib().lpx_tableau_create(int(R), int(C_), C.byref(self._h)))
        self.R, self.C = int(R), int(C_)

    @classmethod
    def from_host(cls, T: np.ndarray, basis: Optional[np.ndarray] = None) -> "DeviceTableau":
        T = np.ascontiguousarray(T, dtype=np.float64)
        t = cls(T.shape[0], T.shape[1])
        t.upload(T, basis)
        return t

    @classmethod
    def with_capacity(cls, T: np.ndarray, basis: Optional[np.ndarray], Rcap: int, Ccap: int) -> "DeviceTableau":
        """A handle of capacity (Rcap, Ccap) holding the smaller tableau T (lpx_tableau_set_shape + upload)."""
        T = np.ascontiguousarray(T, dtype=np.float64)
        t = cls(Rcap, Ccap)
        t.set_shape(*T.shape)
        t.upload(T, basis)
        return t

    def clone(self) -> "DeviceTableau":
        """A second handle in the state of this one (lpx_tableau_clone): the live window, the basis, the bounds with their flips
        and lower shifts, and the loop state.  The snapshot and the trace stay behind; this handle is left as it was."""
        t = object.__new__(type(self))
        t._h = C.c_void_p()
        check(lib().lpx_tableau_clone(self._h, C.byref(t._h)))
        t.R, t.C = self.R, self.C
        return t

    def set_shape(self, R: int, C_: int):
        check(lib().lpx_tableau_set_shape(self._h, int(R), int(C_)))
        self.R, self.C = int(R), int(C_)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().lpx_tableau_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def ld(self) -> int:
        ld = C.c_int()
        check(lib().lpx_tableau_shape(self._h, None, None, C.byref(ld)))
        return ld.value

    def device_ptr(self) -> Tuple[int, int]:
        p = C.c_void_p()
        ld = C.c_int()
        check(lib().lpx_tableau_device_ptr(self._h, C.byref(p), C.byref(ld)))
        return p.value, ld.value

    def upload(self, T: np.ndarray, basis: Optional[np.ndarray] = None):
        T = np.ascontiguousarray(T, dtype=np.float64)
        assert T.shape == (self.R, self.C), (T.shape, self.R, self.C)
        b = None
        if basis is not None:
            basis = np.ascontiguousarray(basis, dtype=np.int32)
            assert basis.shape == (self.R - 1,)
            b = basis.ctypes.data_as(ip)
        check(lib().lpx_tableau_upload(self._h, T.ctypes.data_as(dp), b))

    def download(self) -> Tuple[np.ndarray, np.ndarray]:
        T = np.empty((self.R, self.C), dtype=np.float64)
        basis = np.empty(max(self.R - 1, 0), dtype=np.int32)
        check(lib().lpx_tableau_download(self._h, T.ctypes.data_as(dp), basis.ctypes.data_as(ip)))
        return T, basis

    def snapshot(self):
        check(lib().lpx_tableau_snapshot(self._h))

    def restore(self):
        check(lib().lpx_tableau_restore(self._h))

    def trace(self) -> np.ndarray:
        n = C.c_int()
        check(lib().lpx_tableau_trace(self._h, None, 0, C.byref(n)))
        tr = np.zeros((max(n.value, 1), 2), dtype=np.int32)
        check(lib().lpx_tableau_trace(self._h, tr.ctypes.data_as(ip), n.value, C.byref(n)))
        return tr[: n.value].copy()

    def ranging(self, eps: float = 1e-9) -> TableauRanging:
        """Ranging of the current shape in one device pass; the tableau, basis and trace are left as they are."""
        R, C_ = C.c_int(), C.c_int()
        check(lib().lpx_tableau_shape(self._h, C.byref(R), C.byref(C_), None))
        n, m = C_.value - 1, R.value - 1
        out = [np.empty(k, dtype=t) for k, t in ((n, np.float64), (n, np.int32), (n, np.float64), (n, np.int32),
                                                  (m, np.float64), (m, np.int32), (m, np.float64), (m, np.int32))]
        ptrs = [a.ctypes.data_as(dp if a.dtype == np.float64 else ip) for a in out]
        lo, dj = C.c_double(), C.c_double()
        check(lib().lpx_tableau_ranging(self._h, float(eps), *ptrs, C.byref(lo), C.byref(dj)))
        return TableauRanging(*out, min_rhs=lo.value, min_dj=dj.value)

    def ranging_pairs(self, a, b, eps: float = 1e-9) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The column ratio test along T[:,a[k]] - T[:,b[k]] (equality rows). Returns (inc, inc_at, dec, dec_at)."""
        a = np.ascontiguousarray(a, dtype=np.int32)
        b = np.ascontiguousarray(b, dtype=np.int32)
        assert a.shape == b.shape and a.ndim == 1
        K = len(a)
        inc, dec = np.empty(K), np.empty(K)
        inc_at, dec_at = np.empty(K, dtype=np.int32), np.empty(K, dtype=np.int32)
        check(lib().lpx_tableau_ranging_pairs(self._h, float(eps), K, a.ctypes.data_as(ip), b.ctypes.data_as(ip),
                                              inc.ctypes.data_as(dp), inc_at.ctypes.data_as(ip),
                                              dec.ctypes.data_as(dp), dec_at.ctypes.data_as(ip)))
        return inc, inc_at, dec, dec_at

    def gmi_round(self, is_int, first_cut_col: int, opts=None, bounded: bool = False, **kw) -> Tuple[np.ndarray, np.ndarray]:
        """One GMI cut round on the device (lpx_tableau_gmi_round): is_int[j] marks the integer columns j < len(is_int);
        opts is an lpx_cut_opts (None: defaults with keyword overrides).  The handle takes the new shape.
        bounded=True is lpx_tableau_gmi_round_bounded: a flagged column counts as integer only where the handle's lo and ub are
        whole, ub / lo / flip follow the reshape (every bounded call accepts the handle afterwards), and cuts_per_round=0 is a
        purge-only call.  Returns (source rows, purged columns)."""
        o = opts if opts is not None else _lib.cut_opts(**kw)
        mask = np.ascontiguousarray(np.asarray(is_int) != 0, dtype=np.uint8)
        src = np.zeros(max(o.cuts_per_round, 1), dtype=np.int32)
        pcol = np.zeros(max(self.C, 1), dtype=np.int32)
        k, p = C.c_int(), C.c_int()
        fn = lib().lpx_tableau_gmi_round_bounded if bounded else lib().lpx_tableau_gmi_round
        check(fn(self._h, mask.ctypes.data_as(C.POINTER(C.c_uint8)), len(mask), int(first_cut_col),
                 C.byref(o), C.byref(k), src.ctypes.data_as(ip), C.byref(p), pcol.ctypes.data_as(ip)))
        R, C_ = C.c_int(), C.c_int()
        check(lib().lpx_tableau_shape(self._h, C.byref(R), C.byref(C_), None))
        self.R, self.C = R.value, C_.value
        return src[: k.value].copy(), pcol[: p.value].copy()

    def cut_loop(self, is_int, first_cut_col: int, nint: int, node_is_int=None, opts=None, run_opts: Optional[RunOpts] = None,
                 long_step: bool = False, cutoff: bool = False, form: str = "launches", **kw) -> dict:
        """Rounds of GMI cuts on a solved bounded handle with spare capacity (lpx_bounded_cut_loop): pick, bounded round,
        re-optimisation as a node without a bound edit (form "launches" | "onchip" | "auto", bit-equal), until the pick finds
        no fractional integer column, a round adds no cut, max_rounds are used up, or the re-optimisation ends INFEASIBLE (the
        integer program is infeasible) or at its iteration limit; then one purge-only call when opts.purge is set.  is_int /
        first_cut_col are the round's, nint / node_is_int the pick's; long_step / cutoff set the loop's flags (the cutoff is
        -inf).  Returns {rounds, added, purged, events, stop, status, R, C, var, candidates, x_var, z, z_before, z_after, rc}."""
        if form not in _lib.NODE_FORMS:
            raise ValueError(f"unknown form {form!r}")
        o = opts if opts is not None else _lib.cut_opts(**kw)
        mask = np.ascontiguousarray(np.asarray(is_int) != 0, dtype=np.uint8)
        keep, mp = self._mask(node_is_int, int(nint))
        zb, za = np.zeros(max(o.max_rounds, 1)), np.zeros(max(o.max_rounds, 1))
        rec = _lib.CutLoopRecord()
        rec.z_before, rec.z_after = zb.ctypes.data_as(dp), za.ctypes.data_as(dp)
        flags = (_lib.BDUAL_LONG_STEP if long_step else 0) | (_lib.BDUAL_CUTOFF if cutoff else 0)
        try:
            rc = check(lib().lpx_bounded_cut_loop(self._h, mask.ctypes.data_as(C.POINTER(C.c_uint8)), len(mask), int(first_cut_col),
                                                  int(nint), mp, C.byref(o), C.byref(run_opts) if run_opts is not None else None,
                                                  flags, _lib.NODE_FORMS[form], C.byref(rec)))
        finally:
            self._shape()
        return {"rounds": rec.rounds, "added": rec.added, "purged": rec.purged, "events": rec.events,
                "stop": _lib.CUTLOOP_STOPS[rec.stop], "status": rec.status, "R": rec.R, "C": rec.C, "var": rec.pick.var,
                "candidates": rec.pick.candidates, "x_var": rec.pick.x_var, "z": rec.pick.z,
                "z_before": zb[: rec.rounds].copy(), "z_after": za[: rec.rounds].copy(), "rc": rc}

    def _shape(self):
        R, C_ = C.c_int(), C.c_int()
        check(lib().lpx_tableau_shape(self._h, C.byref(R), C.byref(C_), None))
        self.R, self.C = R.value, C_.value

    def rhs_update(self, cols, v):
        """RHS column += the column combination sum_k v[k] T[:, cols[k]] (lpx_tableau_rhs_update, segment order of
        include/lpx.h)."""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        v = np.ascontiguousarray(v, dtype=np.float64)
        assert cols.shape == v.shape
        check(lib().lpx_tableau_rhs_update(self._h, len(cols), cols.ctypes.data_as(ip), v.ctypes.data_as(dp)))

    def objective_update(self, rows, w, dcols=(), dd=()):
        """Objective row minus the sparse deltas dd at dcols, plus the row combination sum_k w[k] T[rows[k], :], basic
        columns +0.0 (lpx_tableau_objective_update)."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        w = np.ascontiguousarray(w, dtype=np.float64)
        dcols = np.ascontiguousarray(dcols, dtype=np.int32)
        dd = np.ascontiguousarray(dd, dtype=np.float64)
        assert rows.shape == w.shape and dcols.shape == dd.shape
        check(lib().lpx_tableau_objective_update(self._h, len(rows), rows.ctypes.data_as(ip), w.ctypes.data_as(dp),
                                                 len(dcols), dcols.ctypes.data_as(ip), dd.ctypes.data_as(dp)))

    def add_column(self, cols, v, obj: float):
        """New column C-1 = the column combination with base (0, ..., 0, obj); the RHS moves right (lpx_tableau_add_column)."""
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        v = np.ascontiguousarray(v, dtype=np.float64)
        assert cols.shape == v.shape
        check(lib().lpx_tableau_add_column(self._h, len(cols), cols.ctypes.data_as(ip), v.ctypes.data_as(dp), float(obj)))
        self._shape()

    def add_row(self, rows, w, base):
        """New row m = base (C+1 entries, new shape) plus the row combination, basic columns +0.0; its slack becomes basic
        (lpx_tableau_add_row)."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        w = np.ascontiguousarray(w, dtype=np.float64)
        base = np.ascontiguousarray(base, dtype=np.float64)
        assert rows.shape == w.shape and base.shape == (self.C + 1,)
        check(lib().lpx_tableau_add_row(self._h, len(rows), rows.ctypes.data_as(ip), w.ctypes.data_as(dp),
                                        base.ctypes.data_as(dp)))
        self._shape()

    def primal_run(self, opts: Optional[RunOpts] = None, cb: Optional[PivotCallback] = None,
                   **kw) -> Tuple[int, dict]:
        """PrimalSimplex loop (Models/PrimalSimplex.cs:92-124). Returns (status, stats)."""
        o = opts if opts is not None else default_opts(False, **kw)
        st = Stats()
        c = _wrap_cb(cb)
        rc = check(lib().lpx_primal_run(self._h, C.byref(o), c, None, C.byref(st)))
        return rc, st.as_dict()

    def dual_run(self, opts: Optional[RunOpts] = None, cb: Optional[PivotCallback] = None,
                 **kw) -> Tuple[int, dict]:
        """DualSimplex loop (Models/DualSimplex.cs:24,:36-113). Returns (status, stats)."""
        o = opts if opts is not None else default_opts(True, **kw)
        st = Stats()
        c = _wrap_cb(cb)
        rc = check(lib().lpx_dual_run(self._h, C.byref(o), c, None, C.byref(st)))
        return rc, st.as_dict()

    def set_bounds(self, ub):
        """Upper bounds of the columns j < C-1, kept beside the tableau (lpx_tableau_set_bounds); clears every flip.
        None removes the bounds."""
        if ub is None:
            check(lib().lpx_tableau_set_bounds(self._h, 0, None))
            return
        ub = np.ascontiguousarray(ub, dtype=np.float64)
        assert ub.ndim == 1
        check(lib().lpx_tableau_set_bounds(self._h, len(ub), ub.ctypes.data_as(dp)))

    def bound_flags(self) -> np.ndarray:
        """flip[j] = 1: column j currently stands for u_j - x_j (lpx_tableau_bound_flags)."""
        f = np.zeros(max(self.C - 1, 1), dtype=np.uint8)
        check(lib().lpx_tableau_bound_flags(self._h, f.ctypes.data_as(C.POINTER(C.c_uint8))))
        return f[: self.C - 1]

    def bounded_run(self, opts: Optional[RunOpts] = None, cb: Optional[PivotCallback] = None,
                    form: str = "launches", **kw) -> Tuple[int, dict]:
        """Bounded-variable primal loop (lpx_bounded_run): one event per iteration -- a pivot (r, q), a pivot whose leaving
        variable goes to its upper bound (-2 - r, q), or a bound flip (-1, q).  Returns (status, stats).  form "onchip" | "auto"
        (lpx_bounded_run2): the whole loop in ONE kernel launch with the tableau in LDS ("auto": iff the live shape fits and
        there is no callback); everything the handle holds afterwards is bit-equal to "launches", the default."""
        if form not in _lib.NODE_FORMS:
            raise ValueError(f"unknown form {form!r}")
        o = opts if opts is not None else default_opts(False, **kw)
        st = Stats()
        c = _wrap_cb(cb)
        if form == "launches":
            rc = check(lib().lpx_bounded_run(self._h, C.byref(o), c, None, C.byref(st)))
        else:
            rc = check(lib().lpx_bounded_run2(self._h, C.byref(o), _lib.NODE_FORMS[form], c, None, C.byref(st)))
        return rc, st.as_dict()

    def bounded_counts(self) -> Tuple[int, int, int]:
        """Events of the last bounded_run: (pivots to zero, pivots to the upper bound, bound flips)."""
        k = (C.c_int64 * 3)()
        check(lib().lpx_bounded_counts(self._h, k))
        return int(k[0]), int(k[1]), int(k[2])

    def bounded_solution(self, nvars: int) -> Tuple[np.ndarray, float, np.ndarray]:
        """(x[nvars], z, at_upper[nvars]) of the current tableau with its flips undone (lpx_tableau_bounded_solution)."""
        x = np.zeros(max(nvars, 1))
        up = np.zeros(max(nvars, 1), dtype=np.uint8)
        z = C.c_double()
        check(lib().lpx_tableau_bounded_solution(self._h, int(nvars), x.ctypes.data_as(dp), C.byref(z),
                                                 up.ctypes.data_as(C.POINTER(C.c_uint8))))
        return x[:nvars], z.value, up[:nvars]

    def bound_state(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(lo, ub, flip) of the columns j < C-1 (lpx_tableau_bound_state); 0 / +inf / 0 on a handle without bounds."""
        n = max(self.C - 1, 1)
        lo, ub, flip = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.uint8)
        check(lib().lpx_tableau_bound_state(self._h, lo.ctypes.data_as(dp), ub.ctypes.data_as(dp),
                                            flip.ctypes.data_as(C.POINTER(C.c_uint8))))
        return lo[: self.C - 1], ub[: self.C - 1], flip[: self.C - 1]

    def change_bounds(self, cols, lower, upper):
        """New absolute bounds lower[k] <= x_cols[k] <= upper[k] on a solved tableau, in place (lpx_tableau_change_bounds):
        only the RHS column moves, flips and basis stay; re-optimise with bounded_dual_run."""
        cols = np.ascontiguousarray(np.atleast_1d(cols), dtype=np.int32)
        lower = np.ascontiguousarray(np.broadcast_to(np.asarray(lower, dtype=np.float64), cols.shape))
        upper = np.ascontiguousarray(np.broadcast_to(np.asarray(upper, dtype=np.float64), cols.shape))
        check(lib().lpx_tableau_change_bounds(self._h, len(cols), cols.ctypes.data_as(ip), lower.ctypes.data_as(dp),
                                              upper.ctypes.data_as(dp)))

    def bounded_dual_run(self, opts: Optional[RunOpts] = None, cb: Optional[PivotCallback] = None,
                         skip_fixed: bool = False, long_step: bool = False, cutoff: Optional[float] = None,
                         **kw) -> Tuple[int, dict]:
        """Bounded dual simplex (lpx_bounded_dual_run): one event per iteration -- a pivot (r, q) on a row whose basic
        variable is below zero, or (-2 - r, q) on a row whose basic variable is above its upper bound.  skip_fixed=True is
        lpx_bounded_dual_run2 with LPX_BDUAL_SKIP_FIXED: a column with ub = 0 does not enter.  long_step=True or a cutoff is
        lpx_bounded_dual_run3: boxed candidates that leave the row infeasible pass by a bound flip (-1, q) instead of
        entering; the loop ends with status CUTOFF once z <= cutoff.  Returns (status, stats)."""
        o = opts if opts is not None else default_opts(True, **kw)
        st = Stats()
        c = _wrap_cb(cb)
        if long_step or cutoff is not None:
            flags = ((_lib.BDUAL_SKIP_FIXED if skip_fixed else 0) | (_lib.BDUAL_LONG_STEP if long_step else 0)
                     | (_lib.BDUAL_CUTOFF if cutoff is not None else 0))
            rc = check(lib().lpx_bounded_dual_run3(self._h, C.byref(o), flags, float(cutoff if cutoff is not None else 0.0), c,
                                                   None, C.byref(st)))
        elif skip_fixed:
            rc = check(lib().lpx_bounded_dual_run2(self._h, C.byref(o), _lib.BDUAL_SKIP_FIXED, c, None, C.byref(st)))
        else:
            rc = check(lib().lpx_bounded_dual_run(self._h, C.byref(o), c, None, C.byref(st)))
        return rc, st.as_dict()

    def dualize(self, eps: float = 1e-9) -> Tuple[int, int]:
        """Dual-feasibility flips (lpx_tableau_dualize): every column with a reduced cost below -eps and a finite, positive
        upper bound is flipped to its other bound, in ascending order.  Returns (flips, unrepairable)."""
        k = (C.c_int64 * 2)()
        check(lib().lpx_tableau_dualize(self._h, float(eps), k))
        return int(k[0]), int(k[1])

    @staticmethod
    def _mask(is_int, nint):
        if is_int is None:
            return None, None
        a = np.ascontiguousarray(is_int, dtype=np.uint8)
        assert a.shape == (nint,)
        return a, a.ctypes.data_as(C.POINTER(C.c_uint8))

    def branch_pick(self, nint: int, is_int=None, tol: float = 1e-6) -> dict:
        """The branching variable of the tableau as it stands (lpx_tableau_branch_pick): the integer column j < nint whose
        fraction is closest to 0.5, lowest index on ties.  Returns {var (-1: none), candidates, x_var, z}."""
        keep, mp = self._mask(is_int, int(nint))
        out = _lib.BranchPick()
        check(lib().lpx_tableau_branch_pick(self._h, int(nint), mp, float(tol), C.byref(out)))
        return {"var": out.var, "candidates": out.candidates, "x_var": out.x_var, "z": out.z}

    def bounded_node(self, cols, lower, upper, nint: int, is_int=None, tol: float = 1e-6,
                     opts: Optional[RunOpts] = None, long_step: bool = False, cutoff: Optional[float] = None,
                     form: Optional[str] = None, stall_events: Optional[int] = None, fix_bound: Optional[float] = None,
                     **kw) -> dict:
        """One branch-and-bound node in one call (lpx_bounded_node): change_bounds, dualize, the dual loop in which fixed
        columns do not enter, and on OPTIMAL the branch pick.  long_step=True or a cutoff is lpx_bounded_node2: the loop runs
        with those flags and may end with status CUTOFF (no pick).  form "launches" | "onchip" | "auto" is lpx_bounded_node3:
        "onchip" evaluates the whole node in one kernel launch with the tableau in LDS (LpxError when bounded_node_fits() is
        False), "auto" does so iff it fits; the results are bit-equal in every form.  stall_events=S (lpx_bounded_node4; None:
        the calls above): the stall guard -- after S pivots without progress of the objective the loop selects by Bland's rule
        until the objective moves again; 0 is the node without it, above 0 needs the on-chip form (form None means "onchip"
        then).  The record then also carries bland_events and first_bland.  fix_bound=b (lpx_bounded_node5; None: the calls
        above): reduced-cost tightening -- a node that ends OPTIMAL with z > b shrinks the range of every nonbasic integer
        column whose reduced cost d leaves it floor((z - b) / d) steps, in the same launch; -inf is the node without it, any
        other value needs the on-chip form (form None means "onchip" then; stall_events None means 0).  The record then also
        carries fixed = (cols, lower, upper): the tightened columns, ascending, as the triples of a bound edit.  Returns the
        node record as a dict."""
        cols = np.ascontiguousarray(np.atleast_1d(cols), dtype=np.int32).reshape(-1)
        lower = np.ascontiguousarray(np.broadcast_to(np.asarray(lower, dtype=np.float64), cols.shape))
        upper = np.ascontiguousarray(np.broadcast_to(np.asarray(upper, dtype=np.float64), cols.shape))
        o = opts if opts is not None else default_opts(True, **kw)
        keep, mp = self._mask(is_int, int(nint))
        rec = _lib.NodeRecord()
        if fix_bound is not None:
            fix_bound = float(fix_bound)
            if fix_bound != fix_bound:
                raise ValueError("fix_bound is NaN")
            S = 0 if stall_events is None else int(stall_events)
            if S < 0:
                raise ValueError(f"stall_events = {stall_events}: stall_events must not be negative")
            needs_chip = S > 0 or fix_bound != -np.inf
            if form is None:
                form = "onchip" if needs_chip else "launches"
            if form not in _lib.NODE_FORMS:
                raise ValueError(f"unknown node form {form!r}")
            if fix_bound != -np.inf and form == "launches":
                raise ValueError("reduced-cost tightening has no launches form: fix_bound cannot be combined with form='launches'")
            flags = (_lib.BDUAL_SKIP_FIXED | (_lib.BDUAL_LONG_STEP if long_step else 0)
                     | (_lib.BDUAL_CUTOFF if cutoff is not None else 0))
            g = _lib.GuardRecord()
            cap = max(int(nint), 0)
            fc, fl, fu = np.zeros(cap, dtype=np.int32), np.zeros(cap), np.zeros(cap)
            fx = _lib.FixList(cap, 0, fc.ctypes.data_as(ip), fl.ctypes.data_as(dp), fu.ctypes.data_as(dp))
            check(lib().lpx_bounded_node5(self._h, len(cols), cols.ctypes.data_as(ip), lower.ctypes.data_as(dp),
                                          upper.ctypes.data_as(dp), C.byref(o), flags, float(cutoff if cutoff is not None else 0.0),
                                          S, fix_bound, int(nint), mp, float(tol), _lib.NODE_FORMS[form], C.byref(rec),
                                          C.byref(g), C.byref(fx)))
            d = _node_dict(rec)
            d["bland_events"], d["first_bland"] = g.bland_events, g.first_bland
            d["fixed"] = (fc[:fx.n].copy(), fl[:fx.n].copy(), fu[:fx.n].copy())
            return d
        if stall_events is not None:
            if int(stall_events) < 0:
                raise ValueError(f"stall_events = {stall_events}: stall_events must not be negative")
            if form is None:
                form = "onchip" if int(stall_events) > 0 else "launches"
            if form not in _lib.NODE_FORMS:
                raise ValueError(f"unknown node form {form!r}")
            if int(stall_events) > 0 and form == "launches":
                raise ValueError("the stall guard has no launches form: stall_events > 0 cannot be combined with form='launches'")
            flags = (_lib.BDUAL_SKIP_FIXED | (_lib.BDUAL_LONG_STEP if long_step else 0)
                     | (_lib.BDUAL_CUTOFF if cutoff is not None else 0))
            g = _lib.GuardRecord()
            check(lib().lpx_bounded_node4(self._h, len(cols), cols.ctypes.data_as(ip), lower.ctypes.data_as(dp),
                                          upper.ctypes.data_as(dp), C.byref(o), flags, float(cutoff if cutoff is not None else 0.0),
                                          int(stall_events), int(nint), mp, float(tol), _lib.NODE_FORMS[form], C.byref(rec),
                                          C.byref(g)))
            d = _node_dict(rec)
            d["bland_events"], d["first_bland"] = g.bland_events, g.first_bland
            return d
        if form is not None:
            if form not in _lib.NODE_FORMS:
                raise ValueError(f"unknown node form {form!r}")
            flags = (_lib.BDUAL_SKIP_FIXED | (_lib.BDUAL_LONG_STEP if long_step else 0)
                     | (_lib.BDUAL_CUTOFF if cutoff is not None else 0))
            check(lib().lpx_bounded_node3(self._h, len(cols), cols.ctypes.data_as(ip), lower.ctypes.data_as(dp),
                                          upper.ctypes.data_as(dp), C.byref(o), flags, float(cutoff if cutoff is not None else 0.0),
                                          int(nint), mp, float(tol), _lib.NODE_FORMS[form], C.byref(rec)))
        elif long_step or cutoff is not None:
            flags = (_lib.BDUAL_SKIP_FIXED | (_lib.BDUAL_LONG_STEP if long_step else 0)
                     | (_lib.BDUAL_CUTOFF if cutoff is not None else 0))
            check(lib().lpx_bounded_node2(self._h, len(cols), cols.ctypes.data_as(ip), lower.ctypes.data_as(dp),
                                          upper.ctypes.data_as(dp), C.byref(o), flags, float(cutoff if cutoff is not None else 0.0),
                                          int(nint), mp, float(tol), C.byref(rec)))
        else:
            check(lib().lpx_bounded_node(self._h, len(cols), cols.ctypes.data_as(ip), lower.ctypes.data_as(dp),
                                         upper.ctypes.data_as(dp), C.byref(o), int(nint), mp, float(tol), C.byref(rec)))
        return _node_dict(rec)

    def probe(self, nint: int, cand_max: int, probe_iter: Optional[int] = None, is_int=None, tol: float = 1e-6,
              opts: Optional[RunOpts] = None, long_step: bool = False, cutoff: Optional[float] = None,
              prune: float = -np.inf, **kw) -> dict:
        """Strong-branching probes of the tableau as it stands (lpx_bounded_probe): up to cand_max fractional integer columns,
        in the order (|fraction - 0.5|, column), each with its floor and its ceil child evaluated on a private copy by one
        workgroup of ONE launch; nothing of the handle changes.  probe_iter: the event limit of a child (None: the limit of
        opts).  Nothing is probed when the handle's last run did not end OPTIMAL or z <= prune.  Returns {count, candidates, z,
        records, idle}: records[2 c + d] is the dict of candidate c < count, direction d (0 floor, 1 ceil), bit-equal to
        bounded_node(var, lower, upper, form="onchip") on a clone; status None marks a child that call would refuse.  idle[w]:
        slot w of the 2 * cand_max holds no probe (LPX_PROBE_NONE)."""
        cand_max = int(cand_max)
        if cand_max < 1 or cand_max > 32:
            raise ValueError(f"cand_max = {cand_max}: cand_max must be in [1, 32]")
        o = opts if opts is not None else default_opts(True, **kw)
        keep, mp = self._mask(is_int, int(nint))
        flags = (_lib.BDUAL_SKIP_FIXED | (_lib.BDUAL_LONG_STEP if long_step else 0)
                 | (_lib.BDUAL_CUTOFF if cutoff is not None else 0))
        head = _lib.ProbeHead()
        recs = (_lib.ProbeRecord * (2 * cand_max))()
        check(lib().lpx_bounded_probe(self._h, C.byref(o), flags, float(cutoff if cutoff is not None else 0.0), float(prune),
                                      int(nint), mp, float(tol), cand_max, int(o.max_iter if probe_iter is None else probe_iter),
                                      C.byref(head), recs))
        return _probe_dict(head, recs, 0, cand_max)

    def bounded_node_fits(self) -> bool:
        """True iff the on-chip form of bounded_node accepts the live shape (lpx_bounded_node_fits: host arithmetic only)."""
        return bool(lib().lpx_bounded_node_fits(self.R, self.C))

    def forced_pivots(self, rows, cols, thresh: float = 0.1, opts: Optional[RunOpts] = None,
                      **kw) -> Tuple[np.ndarray, dict]:
        """Gauss-Jordan pivots (Models/PrimalSimplex.cs:245-257) at caller-chosen positions."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        assert rows.shape == cols.shape
        chosen = np.full(len(rows), -2, dtype=np.int32)
        o = opts if opts is not None else default_opts(False, **kw)
        st = Stats()
        check(lib().lpx_forced_pivots_run(self._h, rows.ctypes.data_as(ip), cols.ctypes.data_as(ip),
                                          len(rows), float(thresh), chosen.ctypes.data_as(ip),
                                          C.byref(o), C.byref(st)))
        return chosen, st.as_dict()


def _node_dict(rec) -> dict:
    return {"status": rec.status, "events": rec.events, "kind0": rec.kind0, "kind1": rec.kind1, "flips": rec.flips,
            "unrepairable": rec.unrepairable, "var": rec.pick.var, "candidates": rec.pick.candidates,
            "x_var": rec.pick.x_var, "z": rec.pick.z}


def _probe_dict(head, recs, first: int, cand_max: int) -> dict:
    """One entry's probes: the head and the records that ran (2 * count of them), in candidate order."""
    out = []
    for w in range(2 * min(int(head.count), cand_max)):
        r = recs[first + w]
        out.append({"status": None if r.status == -1 else r.status, "events": r.events, "kind0": r.kind0, "kind1": r.kind1,
                    "flips": r.flips, "var": r.var, "dir": r.dir, "x_var": r.x_var, "lower": r.lower, "upper": r.upper, "z": r.z})
    return {"count": int(head.count), "candidates": int(head.candidates), "z": head.z, "records": out,
            "idle": [recs[first + w].status == _lib.PROBE_NONE for w in range(2 * cand_max)]}


class NodeBatch:
    """B branch-and-bound nodes on B handles in ONE kernel launch (lpx_node_batch_*): every entry is bit-equal to
    DeviceTableau.bounded_node(form="onchip") on its handle.  The handles are borrowed: they must have bounds set, fit the on-chip
    form and outlive the batch."""

    def __init__(self, handles):
        self._handles = list(handles)
        self._W = len(self._handles)
        self._h = C.c_void_p()
        hs = (C.c_void_p * max(self._W, 1))(*[t._h for t in self._handles])
        check(lib().lpx_node_batch_create(self._W, hs, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().lpx_node_batch_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def solve(self, slots, opts: Optional[RunOpts] = None, **kw) -> list:
        """Entry i runs the bounded primal loop on handles[slots[i]] from the basis it holds, all in ONE kernel launch
        (lpx_node_batch_primal); the slots are distinct.  Every entry is bit-equal to DeviceTableau.bounded_run(form="onchip")
        on its handle.  Returns one dict per entry: status, events, kind0, kind1, flips, z."""
        slots = np.ascontiguousarray(np.atleast_1d(slots), dtype=np.int32).reshape(-1)
        B = len(slots)
        if B < 1 or B > self._W:
            raise ValueError(f"a batch of {B} entries on {self._W} handles: B must be in [1, W]")
        o = opts if opts is not None else default_opts(False, **kw)
        recs = (_lib.PrimalRecord * B)()
        rc = np.zeros(B, dtype=np.int32)
        check(lib().lpx_node_batch_primal(self._h, B, slots.ctypes.data_as(ip), C.byref(o), recs, rc.ctypes.data_as(ip)))
        return [{"status": int(rc[i]), "events": recs[i].events, "kind0": recs[i].kind0, "kind1": recs[i].kind1,
                 "flips": recs[i].flips, "z": recs[i].z} for i in range(B)]

    def run(self, slots, nodes, nint: int, is_int=None, tol: float = 1e-6, long_step: bool = False, cutoffs=None,
            opts: Optional[RunOpts] = None, stall_events: Optional[int] = None, fix_bounds=None, **kw) -> list:
        """Entry i evaluates nodes[i] = (cols, lower, upper) on handles[slots[i]]; the slots are distinct.  cutoffs: one objective
        cutoff per entry (None: no cutoff).  Returns one record dict per entry in the shape of DeviceTableau.bounded_node; an
        entry the kernel refused (its handle is as it was) has status None, and last_error() holds the first one's message.
        stall_events=S (lpx_node_batch_run2; None: lpx_node_batch_run): every entry runs with the stall guard of
        DeviceTableau.bounded_node and its record also carries bland_events and first_bland.  fix_bounds (lpx_node_batch_run3;
        one value or one per entry, -inf = none for that entry): every entry runs with the reduced-cost tightening of
        DeviceTableau.bounded_node(fix_bound=) and its record also carries fixed = (cols, lower, upper)."""
        if stall_events is not None and int(stall_events) < 0:
            raise ValueError(f"stall_events = {stall_events}: stall_events must not be negative")
        slots = np.ascontiguousarray(np.atleast_1d(slots), dtype=np.int32).reshape(-1)
        B = len(slots)
        if len(nodes) != B:
            raise ValueError(f"{B} slots but {len(nodes)} nodes")
        if B < 1 or B > self._W:
            raise ValueError(f"a batch of {B} entries on {self._W} handles: B must be in [1, W]")
        cs, ls, us = [], [], []
        for cols, lower, upper in nodes:
            c = np.ascontiguousarray(np.atleast_1d(cols), dtype=np.int32).reshape(-1)
            cs.append(c)
            ls.append(np.broadcast_to(np.asarray(lower, dtype=np.float64), c.shape))
            us.append(np.broadcast_to(np.asarray(upper, dtype=np.float64), c.shape))
        K = np.array([len(c) for c in cs], dtype=np.int32)
        cols = np.ascontiguousarray(np.concatenate(cs), dtype=np.int32)
        lower = np.ascontiguousarray(np.concatenate(ls), dtype=np.float64)
        upper = np.ascontiguousarray(np.concatenate(us), dtype=np.float64)
        flags = (_lib.BDUAL_SKIP_FIXED | (_lib.BDUAL_LONG_STEP if long_step else 0)
                 | (_lib.BDUAL_CUTOFF if cutoffs is not None else 0))
        cut, cp = None, None
        if cutoffs is not None:
            cut = np.ascontiguousarray(np.broadcast_to(np.asarray(cutoffs, dtype=np.float64), (B,)))
            cp = cut.ctypes.data_as(dp)
        o = opts if opts is not None else default_opts(True, **kw)
        keep, mp = DeviceTableau._mask(is_int, int(nint))
        recs = (_lib.NodeRecord * B)()
        rc = np.zeros(B, dtype=np.int32)
        guards = None
        fixes = None
        if fix_bounds is not None:
            fb = np.ascontiguousarray(np.broadcast_to(np.asarray(fix_bounds, dtype=np.float64), (B,)))
            if np.isnan(fb).any():
                raise ValueError("fix_bounds holds a NaN")
            guards = (_lib.GuardRecord * B)()
            cap = max(int(nint), 0)
            fc, fl, fu = np.zeros((B, cap), dtype=np.int32), np.zeros((B, cap)), np.zeros((B, cap))
            fixes = (_lib.FixList * B)(*[_lib.FixList(cap, 0, fc[i].ctypes.data_as(ip), fl[i].ctypes.data_as(dp),
                                                      fu[i].ctypes.data_as(dp)) for i in range(B)])
            check(lib().lpx_node_batch_run3(self._h, B, slots.ctypes.data_as(ip), K.ctypes.data_as(ip), cols.ctypes.data_as(ip),
                                            lower.ctypes.data_as(dp), upper.ctypes.data_as(dp), C.byref(o), flags, cp,
                                            int(stall_events or 0), fb.ctypes.data_as(dp), int(nint), mp, float(tol), recs, guards,
                                            fixes, rc.ctypes.data_as(ip)))
        elif stall_events is not None:
            guards = (_lib.GuardRecord * B)()
            check(lib().lpx_node_batch_run2(self._h, B, slots.ctypes.data_as(ip), K.ctypes.data_as(ip), cols.ctypes.data_as(ip),
                                            lower.ctypes.data_as(dp), upper.ctypes.data_as(dp), C.byref(o), flags, cp,
                                            int(stall_events), int(nint), mp, float(tol), recs, guards, rc.ctypes.data_as(ip)))
        else:
            check(lib().lpx_node_batch_run(self._h, B, slots.ctypes.data_as(ip), K.ctypes.data_as(ip), cols.ctypes.data_as(ip),
                                           lower.ctypes.data_as(dp), upper.ctypes.data_as(dp), C.byref(o), flags, cp, int(nint), mp,
                                           float(tol), recs, rc.ctypes.data_as(ip)))
        out = []
        for i in range(B):
            d = _node_dict(recs[i])
            if guards is not None:
                d["bland_events"], d["first_bland"] = guards[i].bland_events, guards[i].first_bland
            if fixes is not None:
                k = fixes[i].n
                d["fixed"] = (fc[i, :k].copy(), fl[i, :k].copy(), fu[i, :k].copy())
            if rc[i] < 0:
                d["status"] = None
            out.append(d)
        return out

    def run_probe(self, slots, nodes, nint: int, cand_max: int, probe_iter: Optional[int] = None, prune=-np.inf, is_int=None,
                  tol: float = 1e-6, long_step: bool = False, cutoffs=None, opts: Optional[RunOpts] = None, **kw):
        """run(), and behind its launch on the same stream the probes of every entry's handle as the node leaves it
        (lpx_node_batch_run_probe): two launches, ONE wait.  prune is one value or one per entry; probe_iter None is the event
        limit of opts.  Returns (records, probes): records as run() returns them, probes[i] as DeviceTableau.probe() would
        return it on handles[slots[i]] afterwards."""
        slots = np.ascontiguousarray(np.atleast_1d(slots), dtype=np.int32).reshape(-1)
        B = len(slots)
        if len(nodes) != B:
            raise ValueError(f"{B} slots but {len(nodes)} nodes")
        if B < 1 or B > self._W:
            raise ValueError(f"a batch of {B} entries on {self._W} handles: B must be in [1, W]")
        cand_max = int(cand_max)
        if cand_max < 1 or cand_max > 32:
            raise ValueError(f"cand_max = {cand_max}: cand_max must be in [1, 32]")
        cs, ls, us = [], [], []
        for cols, lower, upper in nodes:
            c = np.ascontiguousarray(np.atleast_1d(cols), dtype=np.int32).reshape(-1)
            cs.append(c)
            ls.append(np.broadcast_to(np.asarray(lower, dtype=np.float64), c.shape))
            us.append(np.broadcast_to(np.asarray(upper, dtype=np.float64), c.shape))
        K = np.array([len(c) for c in cs], dtype=np.int32)
        cols = np.ascontiguousarray(np.concatenate(cs), dtype=np.int32)
        lower = np.ascontiguousarray(np.concatenate(ls), dtype=np.float64)
        upper = np.ascontiguousarray(np.concatenate(us), dtype=np.float64)
        flags = (_lib.BDUAL_SKIP_FIXED | (_lib.BDUAL_LONG_STEP if long_step else 0)
                 | (_lib.BDUAL_CUTOFF if cutoffs is not None else 0))
        cut, cp = None, None
        if cutoffs is not None:
            cut = np.ascontiguousarray(np.broadcast_to(np.asarray(cutoffs, dtype=np.float64), (B,)))
            cp = cut.ctypes.data_as(dp)
        pr = np.ascontiguousarray(np.broadcast_to(np.asarray(prune, dtype=np.float64), (B,)))
        o = opts if opts is not None else default_opts(True, **kw)
        keep, mp = DeviceTableau._mask(is_int, int(nint))
        recs = (_lib.NodeRecord * B)()
        heads = (_lib.ProbeHead * B)()
        probes = (_lib.ProbeRecord * (B * 2 * cand_max))()
        rc = np.zeros(B, dtype=np.int32)
        check(lib().lpx_node_batch_run_probe(self._h, B, slots.ctypes.data_as(ip), K.ctypes.data_as(ip), cols.ctypes.data_as(ip),
                                             lower.ctypes.data_as(dp), upper.ctypes.data_as(dp), C.byref(o), flags, cp,
                                             pr.ctypes.data_as(dp), int(nint), mp, float(tol), cand_max,
                                             int(o.max_iter if probe_iter is None else probe_iter), recs, heads, probes,
                                             rc.ctypes.data_as(ip)))
        out, pout = [], []
        for i in range(B):
            d = _node_dict(recs[i])
            if rc[i] < 0:
                d["status"] = None
            out.append(d)
            pout.append(_probe_dict(heads[i], probes, i * 2 * cand_max, cand_max))
        return out, pout

    def plunge(self, slots, nodes, nint: int, depth, D: int, prune, is_int=None, tol: float = 1e-6, long_step: bool = False,
               cutoffs=None, opts: Optional[RunOpts] = None, **kw) -> list:
        """run() whose entry i is a chain of up to depth[i] <= D nodes in one launch, the tableau staying in LDS
        (lpx_node_batch_plunge): after a node that branches with z above prune[i], the same workgroup goes on into the ceil child.
        depth and prune are one value or one per entry (prune -inf: nothing is pruned).  Returns, per entry, the list of its
        chain's record dicts in order; a chain the kernel refused inside ends with a dict whose status is None (an entry
        refused at node 0 is that one dict alone)."""
        slots = np.ascontiguousarray(np.atleast_1d(slots), dtype=np.int32).reshape(-1)
        B = len(slots)
        if len(nodes) != B:
            raise ValueError(f"{B} slots but {len(nodes)} nodes")
        if B < 1 or B > self._W:
            raise ValueError(f"a batch of {B} entries on {self._W} handles: B must be in [1, W]")
        D = int(D)
        if D < 1 or D > 64:
            raise ValueError(f"D = {D}: D must be in [1, 64]")
        cs, ls, us = [], [], []
        for cols, lower, upper in nodes:
            c = np.ascontiguousarray(np.atleast_1d(cols), dtype=np.int32).reshape(-1)
            cs.append(c)
            ls.append(np.broadcast_to(np.asarray(lower, dtype=np.float64), c.shape))
            us.append(np.broadcast_to(np.asarray(upper, dtype=np.float64), c.shape))
        K = np.array([len(c) for c in cs], dtype=np.int32)
        cols = np.ascontiguousarray(np.concatenate(cs), dtype=np.int32)
        lower = np.ascontiguousarray(np.concatenate(ls), dtype=np.float64)
        upper = np.ascontiguousarray(np.concatenate(us), dtype=np.float64)
        flags = (_lib.BDUAL_SKIP_FIXED | (_lib.BDUAL_LONG_STEP if long_step else 0)
                 | (_lib.BDUAL_CUTOFF if cutoffs is not None else 0))
        cut, cp = None, None
        if cutoffs is not None:
            cut = np.ascontiguousarray(np.broadcast_to(np.asarray(cutoffs, dtype=np.float64), (B,)))
            cp = cut.ctypes.data_as(dp)
        pr = np.ascontiguousarray(np.broadcast_to(np.asarray(prune, dtype=np.float64), (B,)))
        dep = np.ascontiguousarray(np.broadcast_to(np.asarray(depth, dtype=np.int32), (B,)))
        o = opts if opts is not None else default_opts(True, **kw)
        keep, mp = DeviceTableau._mask(is_int, int(nint))
        recs = (_lib.NodeRecord * (B * D))()
        rc = np.zeros(B, dtype=np.int32)
        steps = np.zeros(B, dtype=np.int32)
        check(lib().lpx_node_batch_plunge(self._h, B, slots.ctypes.data_as(ip), K.ctypes.data_as(ip), cols.ctypes.data_as(ip),
                                          lower.ctypes.data_as(dp), upper.ctypes.data_as(dp), C.byref(o), flags, cp,
                                          pr.ctypes.data_as(dp), dep.ctypes.data_as(ip), D, int(nint), mp, float(tol), recs,
                                          steps.ctypes.data_as(ip), rc.ctypes.data_as(ip)))
        out = []
        for i in range(B):
            chain = [_node_dict(recs[i * D + s]) for s in range(int(steps[i]))]
            if rc[i] < 0:
                d = _node_dict(recs[i * D + int(steps[i])])
                d["status"] = None
                chain.append(d)
            out.append(chain)
        return out


def primal_tableau(T: np.ndarray, basis: np.ndarray, eps: float = 1e-9, max_iter: int = 10000,
                   cb: Optional[PivotCallback] = None):
    """One-shot host-buffer entry point lpx_primal_tableau (in place). Returns (status, stats)."""
    assert T.flags.c_contiguous and T.dtype == np.float64 and basis.dtype == np.int32
    st = Stats()
    rc = check(lib().lpx_primal_tableau(T.ctypes.data_as(dp), T.shape[0], T.shape[1],
                                        basis.ctypes.data_as(ip), eps, max_iter, _wrap_cb(cb), None,
                                        C.byref(st)))
    return rc, st.as_dict()


def dual_tableau(T: np.ndarray, basis: np.ndarray, eps: float = 1e-9, ratio_tol: float = 1e-12,
                 fdf_guard: int = 100, max_iter: int = 10000, cleanup: int = 0,
                 cb: Optional[PivotCallback] = None):
    """One-shot host-buffer entry point lpx_dual_tableau (in place). Returns (status, stats)."""
    assert T.flags.c_contiguous and T.dtype == np.float64 and basis.dtype == np.int32
    st = Stats()
    rc = check(lib().lpx_dual_tableau(T.ctypes.data_as(dp), T.shape[0], T.shape[1],
                                      basis.ctypes.data_as(ip), eps, ratio_tol, fdf_guard, max_iter,
                                      cleanup, _wrap_cb(cb), None, C.byref(st)))
    return rc, st.as_dict()


def multi_run(tableaux, dual, primal_opts: Optional[RunOpts] = None, dual_opts: Optional[RunOpts] = None):
    """lpx_multi_run: runs several device tableaux to completion together (B&B node batches, K9).
    Returns (statuses, [stats dict])."""
    k = len(tableaux)
    hs = (C.c_void_p * k)(*[t._h for t in tableaux])
    dl = (C.c_int * k)(*[1 if d else 0 for d in dual])
    st = (C.c_int * k)()
    ss = (Stats * k)()
    po = primal_opts if primal_opts is not None else default_opts(False)
    do = dual_opts if dual_opts is not None else default_opts(True)
    check(lib().lpx_multi_run(hs, dl, k, C.byref(po), C.byref(do), st, ss))
    return list(st), [s.as_dict() for s in ss]
