"""Python face of the reference's plugin boundary (Models/IPLAlgorithm.cs:5-8, Models/LPSolver.cs):
`LPSolver().Solve(problem, "Primal Simplex")`, `PrimalSimplex().Solve(problem)` ... with the same names
and error behaviour.  All solving goes through lpx_solve (C ABI) -> C++ host mirror -> HIP kernels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from enum import IntEnum
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import lib


class Sense(IntEnum):       # Models/PrimalSimplex.cs:8
    Max = 0
    Min = 1


class Rel(IntEnum):         # Models/PrimalSimplex.cs:9
    LE = 0
    GE = 1
    EQ = 2


@dataclass
class Constraint:           # Models/PrimalSimplex.cs:11-18
    A: Sequence[float]
    Relation: Rel
    B: float


@dataclass
class LPProblem:            # Models/PrimalSimplex.cs:20-36
    ObjectiveSense: Sense = Sense.Max
    C: Sequence[float] = field(default_factory=list)
    Constraints: List[Constraint] = field(default_factory=list)

    @property
    def NumVars(self) -> int:
        return len(self.C)

    @classmethod
    def from_arrays(cls, sense, c, A, rel, b) -> "LPProblem":
        A = np.asarray(A, dtype=np.float64).reshape(len(b), len(c))
        return cls(Sense(int(sense)), list(map(float, c)),
                   [Constraint(A[i].tolist(), Rel(int(rel[i])), float(b[i])) for i in range(len(b))])


@dataclass
class SimplexResult:        # Models/PrimalSimplex.cs:38-49 (+ engine extras after VarNames)
    Report: str
    Summary: str
    OptimalValue: float
    Solution: Optional[np.ndarray]
    Tableau: Optional[np.ndarray]
    Basis: Optional[np.ndarray]
    VarNames: Optional[List[str]]
    Status: int = 0
    Trace: Optional[np.ndarray] = None
    LpSolves: int = 0
    Nodes: int = 0
    NodeLog: Optional[np.ndarray] = None
    NodeZ: Optional[np.ndarray] = None
    Aux: Optional[list] = None
    Stats: Optional[dict] = None
    Extra: Optional[np.ndarray] = None      # revised / knapsack: numbers the reference only prints
    Cuts: Optional[np.ndarray] = None       # cutting plane: rows (A[0..n), B) in the order added
    Ranging: Optional["RangingReport"] = None   # LPSolver.SolveRanged only
    AtUpper: Optional[np.ndarray] = None    # LPSolver.SolveBounded only: 1 = x_j is nonbasic at its upper bound
    Flips: Optional[np.ndarray] = None      # ... flip state of every tableau column (1 = the column stands for u_j - x_j)
    BoundCounts: Optional[tuple] = None     # ... events: (pivots to zero, pivots to the upper bound, bound flips)


@dataclass
class PackedResult:         # lpx_packed_results (include/lpx.h): LPSolver.SolvePacked, one entry per model along axis 0
    Status: np.ndarray                      # (B,) int32: OPTIMAL, UNBOUNDED, ITER_LIMIT, or a negative LPX_E* of that model alone
    Solution: np.ndarray                    # (B, n)
    OptimalValue: np.ndarray                # (B,) in the user's sense
    Events: Optional[np.ndarray] = None     # (B,) pivots and flips                                         (want "rec")
    BoundCounts: Optional[np.ndarray] = None    # (B, 3): pivots to zero, pivots to the upper bound, flips  (want "rec")
    Z: Optional[np.ndarray] = None          # (B,) T[m, C-1] as the loop left it                            (want "rec")
    Basis: Optional[np.ndarray] = None      # (B, m) int32                                                  (want "basis")
    AtUpper: Optional[np.ndarray] = None    # (B, n) uint8: 1 = x_j is nonbasic at its upper bound          (want "at_upper")
    Stats: Optional[dict] = None


@dataclass
class PackedDualResult(PackedResult):   # lpx_packed_dual_results (include/lpx.h): LPSolver.SolvePackedDual
    # Status: OPTIMAL, INFEASIBLE, ITER_LIMIT or LPX_EINVAL of that model alone; BoundCounts (B, 3): kind-0 pivots, kind-1 pivots, passes
    Duals: Optional[np.ndarray] = None          # (B, m) y_i = d value / d b_i, the user's sense and rows       (want "y")
    ReducedCosts: Optional[np.ndarray] = None   # (B, n) d_j = c_j - sum_i y_i A_ij                              (want "d")
    Passes: Optional[np.ndarray] = None         # (B,) long-step passes                                          (want "rec")
    DualizeFlips: Optional[np.ndarray] = None   # (B,) dual-feasibility flips in front of the loop               (want "rec")


@dataclass
class PackedCostResult:     # lpx_packed_cost_results (include/lpx.h): PackedBase.solve_costs, one entry per scenario along axis 0
    Status: np.ndarray                      # (B,) int32: OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT or LPX_EINVAL of that scenario alone
    Solution: np.ndarray                    # (B, n)
    OptimalValue: np.ndarray                # (B,) in the user's sense
    Events: Optional[np.ndarray] = None     # (B,) PrimalEvents + DualEvents
    Z: Optional[np.ndarray] = None          # (B,) T[m, C-1] as the last loop left it
    Basis: Optional[np.ndarray] = None      # (B, m) int32
    AtUpper: Optional[np.ndarray] = None    # (B, n) uint8: 1 = x_j is nonbasic at its upper bound
    Stats: Optional[dict] = None
    Duals: Optional[np.ndarray] = None          # (B, m) y_i = d value / d b_i, the user's sense and rows
    ReducedCosts: Optional[np.ndarray] = None   # (B, n) d_j = c_j - sum_i y_i A_ij
    PrimalEvents: Optional[np.ndarray] = None   # (B,) pivots and bound flips of the primal loop
    DualEvents: Optional[np.ndarray] = None     # (B,) pivots and passes of the dual loop (0 without b)
    PrimalCounts: Optional[np.ndarray] = None   # (B, 3): kind-0 pivots, kind-1 pivots, bound flips
    DualCounts: Optional[np.ndarray] = None     # (B, 3): kind-0 pivots, kind-1 pivots, long-step passes


PACKED_COST_DTYPE = np.dtype([("status", "<i4"), ("primal_events", "<i4"), ("dual_events", "<i4"), ("pad", "<i4"),
                              ("primal_kind0", "<i8"), ("primal_kind1", "<i8"), ("primal_flips", "<i8"),
                              ("dual_kind0", "<i8"), ("dual_kind1", "<i8"), ("dual_passes", "<i8"), ("z", "<f8")])


@dataclass
class PackedBnbResult(PackedResult):    # lpx_packed_bnb_results (include/lpx.h): LPSolver.SolvePackedBnb
    # Status: OPTIMAL, INFEASIBLE, ITER_LIMIT (a budget: see Stop), the root's UNBOUNDED, or LPX_EINVAL / LPX_E_NEG_RHS of that model alone
    Stop: Optional[np.ndarray] = None           # (B,) int32 LPX_PBNB_*: done, root, nodes, node_iter, events, depth, refused (want "rec")
    Nodes: Optional[np.ndarray] = None          # (B,) nodes evaluated                                               (want "rec")
    Info: Optional[np.ndarray] = None           # (B,) structured: every counter of lpx_packed_bnb_record            (want "rec")
    Log: Optional[np.ndarray] = None            # (B, log_cap) of the BnbLog dtype; zero behind Logged[i] records     (log_cap > 0)
    Logged: Optional[np.ndarray] = None         # (B,) min(nodes, log_cap)                                            (log_cap > 0)


PACKED_BNB_DTYPE = np.dtype([("status", "<i4"), ("stop", "<i4"), ("nodes", "<i8"), ("events", "<i8"), ("flips", "<i8"),
                             ("incumbents", "<i8"), ("pruned_bound", "<i8"), ("pruned_infeasible", "<i8"), ("max_K", "<i4"),
                             ("deepest", "<i4"), ("root_events", "<i4"), ("logged", "<i4"), ("best", "<f8"), ("constant", "<f8")])


@dataclass
class RangingReport:       # lpx_ranging (include/lpx.h): ranges of the solved model in user terms
    valid: bool
    cost_lo: np.ndarray
    cost_hi: np.ndarray
    cost_lo_at: np.ndarray      # tableau column entering at that end (x1..xn = 0..n-1, then the slacks), -1 = none
    cost_hi_at: np.ndarray
    reduced_cost: np.ndarray    # d(optimal objective) / d(lower bound of x_j)
    rhs_lo: np.ndarray
    rhs_hi: np.ndarray
    rhs_lo_at: np.ndarray       # basic variable leaving at that end, -1 = none
    rhs_hi_at: np.ndarray
    dual: np.ndarray            # d(optimal objective) / d(b_i)
    min_rhs: float
    min_dj: float


@dataclass
class CutOpts:              # lpx_cut_opts (include/lpx.h): the GMI cut round and loop
    cuts_per_round: int = 8
    max_rounds: int = 50
    max_active: int = 64
    purge: int = 1
    away: float = 1e-3
    coef_eps: float = 1e-9
    max_dynamism: float = 1e6
    purge_tol: float = 1e-9
    int_tol: float = 1e-6

    def to_c(self) -> "_lib.CutOpts":
        o = _lib.CutOpts()
        for k, _ in o._fields_:
            setattr(o, k, getattr(self, k))
        return o


class SolverException(Exception):
    """The reference's `throw new Exception(message)`; `.code` is the LPX_E_* of include/lpx.h."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


def _problem_struct(p: LPProblem):
    n, m = p.NumVars, len(p.Constraints)
    c = np.ascontiguousarray(p.C, dtype=np.float64)
    A = np.zeros((max(m, 1), max(n, 1)), dtype=np.float64)
    rel = np.zeros(max(m, 1), dtype=np.int32)
    b = np.zeros(max(m, 1), dtype=np.float64)
    for i, k in enumerate(p.Constraints):
        if len(k.A) < n:
            # row.A[j] for j < n (Models/PrimalSimplex.cs:190)
            raise SolverException(_lib.EINVAL, "Index was outside the bounds of the array.")
        A[i, :n] = np.asarray(k.A[:n], dtype=np.float64)
        rel[i] = int(k.Relation)
        b[i] = float(k.B)
    st = _lib.Problem(int(p.ObjectiveSense), n, m, c.ctypes.data_as(_lib.dp), A.ctypes.data_as(_lib.dp),
                      rel.ctypes.data_as(_lib.ip), b.ctypes.data_as(_lib.dp))
    return st, (c, A, rel, b)


def _arr(ptr, n, dtype):
    if not ptr or n <= 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


def _solve_opts(engine: dict):
    """lpx_solve_opts from keyword engine options; returns (opts, objects to keep alive)."""
    L = lib()
    o = _lib.SolveOpts()
    L.lpx_default_solve_opts(C.byref(o))
    keep = []
    for k, v in engine.items():
        if k == "allreduce_max":
            if v is None:
                continue        # NULL: one process, or the library's own RCCL communicator (comm.py / lpx_comm_init)
            fn = v

            def _ar(_u, vals, count, fn=fn):
                a = np.ctypeslib.as_array(vals, shape=(count,))
                a[:] = fn(a.copy())
            cb = _lib.ALLREDUCE_CB(_ar)
            keep.append(cb)
            o.allreduce_max = cb
        elif k in ("test_node_lp", "test_knap_relax", "test_fail_after_nodes"):
            continue            # include/lpx_test.h seams: installed around the call by LPSolver.Solve
        elif hasattr(o, k):
            setattr(o, k, v)
        else:
            raise TypeError(f"unknown engine option {k!r}")
    return o, keep


def _take_result(r, n: int) -> "SimplexResult":
    """Copies an lpx_result into a SimplexResult and frees it. n = NumVars of the solved model."""
    try:
        has = bool(r.has_solution)
        T = _arr(r.T, r.R * r.C, np.float64).reshape(r.R, r.C) if r.R > 0 else None
        names = None
        if has and T is not None:
            ns = T.shape[1] - 1
            names = [f"x{j + 1}" for j in range(n)] + [f"c{j + 1}" for j in range(ns - n)]
        log = _arr(r.node_log, 3 * r.n_log, np.int32).reshape(-1, 3)
        res = SimplexResult(
            Report=(r.report or b"").decode(errors="replace"), Summary=(r.summary or b"").decode(errors="replace"),
            OptimalValue=r.optimal_value,
            Solution=_arr(r.x, r.n, np.float64) if has else None,
            Tableau=T if has else None,
            Basis=_arr(r.basis, max(r.R - 1, 0), np.int32) if has else None,
            VarNames=names, Status=r.status,
            Trace=_arr(r.trace, 2 * r.n_pivots, np.int32).reshape(-1, 2),
            LpSolves=r.lp_solves, Nodes=r.nodes, NodeLog=log, NodeZ=_arr(r.node_z, r.n_log, np.float64),
            Aux=list(r.aux), Stats=r.stats.as_dict(),
            Extra=None if has else (T.reshape(-1) if T is not None and T.size else _arr(r.x, r.n, np.float64)),
            Cuts=_arr(r.cuts, r.n_cuts * (n + 1), np.float64).reshape(-1, n + 1) if r.n_cuts > 0 else None)
        if not has and r.n > 0:
            res.Extra = _arr(r.x, r.n, np.float64)
        elif not has and T is not None:
            res.Extra = T.reshape(-1)
    finally:
        lib().lpx_result_free(C.byref(r))
    return res


# lpx_bnb_node_log as a NumPy record
BNB_LOG_DTYPE = np.dtype([("depth", "<i4"), ("K", "<i4"), ("status", "<i4"), ("events", "<i4"), ("flips", "<i4"),
                          ("var", "<i4"), ("z", "<f8")])


def _packed_inputs(c, A, b, upper, lower, sense, rel=None):
    """The arguments SolvePacked and SolvePackedDual share, checked: (sense, c, A, b, {"upper", "lower"}, rel, B, m, n).  An array
    without the batch axis is shared; B comes from whichever argument has the batch axis (none: B = 1).  rel (SolvePackedDual
    only): (m,) or (B, m) of 0 / 1 or "<=" / ">=", returned as int32."""
    if isinstance(sense, str):
        if sense.lower() not in ("max", "min"):
            raise ValueError(f"unknown sense {sense!r}")
        sense = 1 if sense.lower() == "min" else 0

    def _f64(v):
        return np.ascontiguousarray(np.asarray(v, dtype=np.float64))
    c, A, b = _f64(c), _f64(A), _f64(b)
    if c.ndim not in (1, 2) or A.ndim not in (2, 3) or b.ndim not in (1, 2):
        raise ValueError("c is (B, n) or (n,), A is (B, m, n) or (m, n), b is (B, m) or (m,)")
    m, n = A.shape[-2], A.shape[-1]
    if c.shape[-1] != n or b.shape[-1] != m:
        raise ValueError(f"A is {m} x {n}, but c has {c.shape[-1]} entries and b has {b.shape[-1]}")
    batched = [("c", c, 2), ("A", A, 3), ("b", b, 2)]
    bounds = {}
    for name, v in (("upper", upper), ("lower", lower)):
        if v is None:
            bounds[name] = None
            continue
        if np.ndim(v) == 0:
            v = np.full(n, float(v))                # one shared row, not one per model
        v = _f64(v)
        if v.ndim not in (1, 2) or v.shape[-1] != n:
            raise ValueError(f"{name} is (B, n), (n,) or a scalar with n = {n}")
        bounds[name] = v
        batched.append((name, v, 2))
    if rel is not None:
        rel = np.asarray(rel)
        if rel.dtype.kind in "US":
            known = np.isin(rel, ("<=", ">="))
            if not known.all():
                raise ValueError(f"rel holds {rel[~known].flat[0]!r}: a row is '<=' or '>=' (an = row is passed as its pair)")
            rel = rel == ">="
        elif rel.dtype.kind not in "biu":
            raise ValueError("rel holds integers (0 = <=, 1 = >=) or the strings '<=' / '>='")
        rel = np.ascontiguousarray(rel, dtype=np.int32)
        if rel.ndim not in (1, 2) or rel.shape[-1] != m:
            raise ValueError(f"rel is (B, m) or (m,) with m = {m}")
        batched.append(("rel", rel, 2))
    sizes = {name: v.shape[0] for name, v, nd in batched if v.ndim == nd}
    if len(set(sizes.values())) > 1:
        raise ValueError(f"the batch axes disagree: {sizes}")
    B = next(iter(sizes.values())) if sizes else 1
    if B < 1:
        raise ValueError("an empty batch")
    return sense, c, A, b, bounds, rel, B, m, n


class LPSolver:             # Models/LPSolver.cs:6-77
    def __init__(self, **engine):
        self.engine = engine
        self.FinalTableau = None

    def Solve(self, problem: LPProblem, algorithm: str,
              updatePivot: Optional[Callable[[str, Optional[np.ndarray]], None]] = None) -> SimplexResult:
        L = lib()
        o, keep = _solve_opts(self.engine)
        if updatePivot is not None:
            def _txt(_u, text, hl, R, Cc):
                mask = None
                if hl and R > 0:
                    mask = np.ctypeslib.as_array(hl, shape=(R * Cc,)).astype(bool).reshape(R, Cc)
                updatePivot(text.decode(errors="replace"), mask)
            tcb = _lib.TEXT_CB(_txt)
            keep.append(tcb)
            o.text_cb = tcb
        ps, hold = _problem_struct(problem)
        r = _lib.Result()
        seams = None
        if "test_node_lp" in self.engine or "test_knap_relax" in self.engine or "test_fail_after_nodes" in self.engine:      # test-only (include/lpx_test.h)
            seams = _lib.TestSeams()
            seams.fail_after_nodes = int(self.engine.get("test_fail_after_nodes", 0))
            if "test_node_lp" in self.engine:
                seams.node_lp = _lib.TEST_NODE_LP(self.engine["test_node_lp"])
            if "test_knap_relax" in self.engine:
                seams.knap_relax = _lib.TEST_KNAP_RELAX(self.engine["test_knap_relax"])
            L.lpx_test_set_seams(C.byref(seams))
        try:
            rc = L.lpx_solve(C.byref(ps), algorithm.encode() if algorithm is not None else b"", C.byref(o), C.byref(r))
        finally:
            if seams is not None:
                L.lpx_test_set_seams(None)
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        res = _take_result(r, problem.NumVars)
        if algorithm is not None and _algorithm_key(algorithm) in ("gmi cutting plane", "gmi"):
            _gmi_names(res, problem)
        self.FinalTableau = res.Tableau
        return res

    def SolveRanged(self, problem: LPProblem, algorithm: str) -> SimplexResult:
        """Solve (Primal Simplex or Dual Simplex) plus the ranging report of the final tableau, computed on the
        device tableau of the solve itself (lpx_solve_ranging); the result is otherwise what Solve returns."""
        L = lib()
        o, keep = _solve_opts(self.engine)
        ps, hold = _problem_struct(problem)
        r, g = _lib.Result(), _lib.Ranging()
        rc = L.lpx_solve_ranging(C.byref(ps), algorithm.encode() if algorithm is not None else b"", C.byref(o),
                                 C.byref(r), C.byref(g))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        try:
            rep = RangingReport(
                valid=bool(g.valid),
                cost_lo=_arr(g.cost_lo, g.n, np.float64), cost_hi=_arr(g.cost_hi, g.n, np.float64),
                cost_lo_at=_arr(g.cost_lo_at, g.n, np.int32), cost_hi_at=_arr(g.cost_hi_at, g.n, np.int32),
                reduced_cost=_arr(g.reduced_cost, g.n, np.float64),
                rhs_lo=_arr(g.rhs_lo, g.m, np.float64), rhs_hi=_arr(g.rhs_hi, g.m, np.float64),
                rhs_lo_at=_arr(g.rhs_lo_at, g.m, np.int32), rhs_hi_at=_arr(g.rhs_hi_at, g.m, np.int32),
                dual=_arr(g.dual, g.m, np.float64), min_rhs=g.min_rhs, min_dj=g.min_dj)
        finally:
            L.lpx_ranging_free(C.byref(g))
        res = _take_result(r, problem.NumVars)
        res.Ranging = rep
        self.FinalTableau = res.Tableau
        return res


    def SolveCuts(self, problem: LPProblem, opts: Optional[CutOpts] = None, **cut_opts) -> SimplexResult:
        """The GMI cutting-plane loop on the device (lpx_solve_cuts) with explicit options (CutOpts fields as keywords);
        Solve(problem, "GMI Cutting Plane") is this with the defaults.  Status: CUT_INTEGER, CUT_INCOMPLETE, INFEASIBLE
        or UNBOUNDED; NodeLog rows are (round, source row, slack column) per cut; Cuts are x-space LE rows (A, B)."""
        co = opts if opts is not None else CutOpts(**cut_opts)
        o, keep = _solve_opts(self.engine)
        ps, hold = _problem_struct(problem)
        r = _lib.Result()
        c = co.to_c()
        rc = lib().lpx_solve_cuts(C.byref(ps), C.byref(o), C.byref(c), C.byref(r))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        res = _take_result(r, problem.NumVars)
        _gmi_names(res, problem)
        self.FinalTableau = res.Tableau
        return res

    def SolveBoundedDual(self, problem: LPProblem, upper, lower=None, long_step: bool = True) -> SimplexResult:
        """The dual start (lpx_solve_bounded_dual): the bounded dual simplex from the slack basis, for the models SolveBounded
        refuses -- >= rows and negative right-hand sides are accepted; every variable that improves the objective needs a
        finite upper bound.  long_step: the bound-flipping ratio test (LPX_BDUAL_LONG_STEP).  Status OPTIMAL or INFEASIBLE; the
        result is laid out as SolveBounded's, BoundCounts = (kind-0 pivots, kind-1 pivots, passes)."""
        return self._solve_bounded(problem, upper, lower, _lib.BDUAL_LONG_STEP if long_step else 0)

    def SolveBounded(self, problem: LPProblem, upper=None, lower=None, form: str = "launches") -> SimplexResult:
        """The bounded-variable primal simplex on the device (lpx_solve_bounded): lower[j] <= x_j <= upper[j] without a row
        per bound (None: 0 / +inf).  Status, Solution (user variables), OptimalValue (user's sense), Tableau / Basis (the final
        internal tableau), Trace (events: (r, q) pivot, (-2 - r, q) pivot to the upper bound, (-1, q) bound flip), AtUpper,
        Flips, BoundCounts.  Solve(problem, "Bounded Primal Simplex") is this without bounds.  form "onchip" | "auto"
        (lpx_solve_bounded2): the whole loop in ONE kernel launch with the tableau in LDS ("auto": iff the model fits); the
        result is that of "launches", the default, apart from the launch count."""
        if form not in _lib.NODE_FORMS:
            raise ValueError(f"unknown form {form!r}")
        return self._solve_bounded(problem, upper, lower, None, form)

    def SolveBoundedBatch(self, problems, uppers=None, lowers=None) -> list:
        """Many independent bounded models in ONE kernel launch (lpx_solve_bounded_batch): 1 <= len(problems) <= 1024 models
        of any mix of shapes, each of which must fit the on-chip form.  uppers / lowers: None or one entry (None or bounds) per
        model.  Returns one SimplexResult per model, each equal to SolveBounded(..., form="onchip") of that model."""
        problems = list(problems)
        count = len(problems)
        if count < 1 or count > 1024:
            raise ValueError(f"{count} models: count must be in [1, 1024]")
        for name, v in (("uppers", uppers), ("lowers", lowers)):
            if v is not None and len(v) != count:
                raise ValueError(f"{len(v)} {name} for {count} models")
        o, keep = _solve_opts(self.engine)
        structs, holds, arrs = [], [], []
        lop, upp = (_lib.dp * count)(), (_lib.dp * count)()
        for i, pr in enumerate(problems):
            ps, hold = _problem_struct(pr)
            structs.append(ps); holds.append(hold)
            for ptrs, v in ((lop, lowers), (upp, uppers)):
                if v is not None and v[i] is not None:
                    a = np.ascontiguousarray(np.broadcast_to(np.asarray(v[i], dtype=np.float64), (pr.NumVars,)))
                    arrs.append(a)
                    ptrs[i] = a.ctypes.data_as(_lib.dp)
        pp = (C.POINTER(_lib.Problem) * count)(*[C.pointer(ps) for ps in structs])
        rs, infos = (_lib.Result * count)(), (_lib.BoundedInfo * count)()
        rc = lib().lpx_solve_bounded_batch(count, pp, lop, upp, C.byref(o), rs, infos)
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        return [self._bounded_result(rs[i], infos[i], problems[i].NumVars) for i in range(count)]

    def SolvePacked(self, c, A, b, upper=None, lower=None, sense="max", max_iter=None,
                    want=("rec", "basis", "at_upper")) -> PackedResult:
        """B bounded models of ONE shape (m rows, all <=; n variables) as arrays, solved in ONE kernel launch with one upload
        per array and one read-back (lpx_solve_packed).  c: (B, n) or (n,); A: (B, m, n) or (m, n); b: (B, m) or (m,); upper /
        lower: the shapes of c, a scalar, or None (+inf / 0).  An array without the batch axis is shared by every model (stride
        0) and is never tiled on the host.  B comes from whichever argument has the batch axis (none: B = 1); disagreeing axes
        are a ValueError.  sense: "max" | "min".  Every model gets its own Status: one that is refused (LPX_EINVAL for its bounds,
        LPX_E_NEG_RHS) or reaches the iteration limit does not fail the call.  Each entry is bit-equal to
        SolveBounded(model, upper, lower, form="onchip").  want: which of the optional outputs to fetch."""
        want = tuple(want)
        for w in want:
            if w not in ("rec", "basis", "at_upper"):
                raise ValueError(f"unknown output {w!r}")
        sense, c, A, b, bounds, _, B, m, n = _packed_inputs(c, A, b, upper, lower, sense)

        def _stride(v, nd, packed):
            return packed if v.ndim == nd else 0
        pm = _lib.PackedModels()
        pm.count, pm.m, pm.n, pm.sense = B, m, n, int(sense)
        pm.c, pm.A, pm.b = (v.ctypes.data_as(_lib.dp) for v in (c, A, b))
        pm.c_stride, pm.A_stride, pm.b_stride = _stride(c, 2, n), _stride(A, 3, m * n), _stride(b, 2, m)
        for name in ("upper", "lower"):
            v = bounds[name]
            if v is not None:
                setattr(pm, name, v.ctypes.data_as(_lib.dp))
                setattr(pm, name + "_stride", _stride(v, 2, n))
        status = np.zeros(B, dtype=np.int32); x = np.zeros((B, n)); value = np.zeros(B)
        pr = _lib.PackedResults()
        pr.status, pr.x, pr.value = status.ctypes.data_as(_lib.ip), x.ctypes.data_as(_lib.dp), value.ctypes.data_as(_lib.dp)
        recs = basis = at = None
        if "rec" in want:
            recs = (_lib.PrimalRecord * B)()
            pr.rec = recs
        if "basis" in want:
            basis = np.zeros((B, m), dtype=np.int32)
            pr.basis = basis.ctypes.data_as(_lib.ip)
        if "at_upper" in want:
            at = np.zeros((B, n), dtype=np.uint8)
            pr.at_upper = at.ctypes.data_as(C.POINTER(C.c_uint8))
        limit = max_iter if max_iter is not None else self.engine.get("max_iter")
        o = _lib.default_opts(False) if limit is None else _lib.default_opts(False, max_iter=int(limit))
        st = _lib.Stats()
        rc = lib().lpx_solve_packed(C.byref(pm), C.byref(o), C.byref(pr), C.byref(st))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        res = PackedResult(Status=status, Solution=x, OptimalValue=value, Basis=basis, AtUpper=at, Stats=st.as_dict())
        if recs is not None:
            r = np.frombuffer(recs, dtype=np.dtype([("status", "<i4"), ("events", "<i4"), ("kind0", "<i8"), ("kind1", "<i8"),
                                                    ("flips", "<i8"), ("z", "<f8")]))
            res.Events = r["events"].copy()
            res.BoundCounts = np.stack([r["kind0"], r["kind1"], r["flips"]], axis=1)
            res.Z = r["z"].copy()
        return res

    def SolvePackedDual(self, c, A, b, rel=None, upper=None, lower=None, sense="max", long_step: bool = True, max_iter=None,
                        want=("rec", "basis", "at_upper", "y", "d")) -> PackedDualResult:
        """SolvePacked by a dual start (lpx_solve_packed_dual): B models of ONE shape whose rows are <= or >= and whose right-hand
        sides may have either sign, in ONE kernel launch -- covering models, Min c.x, A x >= b, right-hand-side sweeps across zero.
        The arrays are SolvePacked's; rel: None (every row <=), (m,) shared by every model or (B, m), of 0 / 1 (LPX_LE / LPX_GE)
        or the strings "<=" / ">=".  Every variable that improves the objective needs a finite upper bound.  long_step: the
        bound-flipping ratio test (LPX_BDUAL_LONG_STEP).  Every model gets its own Status: OPTIMAL, INFEASIBLE, ITER_LIMIT, or
        LPX_EINVAL for its bounds, a bad entry of its own rel row, or an improving variable without an upper bound.  Each entry is
        bit-equal to SolveBoundedDual(model, upper, lower, long_step).  Duals y_i = d value / d b_i and ReducedCosts
        d_j = c_j - sum_i y_i A_ij are in the user's sense and on the user's rows.  want: which optional outputs to fetch."""
        want = tuple(want)
        for w in want:
            if w not in ("rec", "basis", "at_upper", "y", "d"):
                raise ValueError(f"unknown output {w!r}")
        sense, c, A, b, bounds, rel, B, m, n = _packed_inputs(c, A, b, upper, lower, sense, rel)

        def _stride(v, nd, packed):
            return packed if v.ndim == nd else 0
        pm = _lib.PackedDualModels()
        pm.count, pm.m, pm.n, pm.sense = B, m, n, int(sense)
        pm.c, pm.A, pm.b = (v.ctypes.data_as(_lib.dp) for v in (c, A, b))
        pm.c_stride, pm.A_stride, pm.b_stride = _stride(c, 2, n), _stride(A, 3, m * n), _stride(b, 2, m)
        for name in ("upper", "lower"):
            v = bounds[name]
            if v is not None:
                setattr(pm, name, v.ctypes.data_as(_lib.dp))
                setattr(pm, name + "_stride", _stride(v, 2, n))
        if rel is not None:
            pm.rel, pm.rel_stride = rel.ctypes.data_as(_lib.ip), _stride(rel, 2, m)
        status = np.zeros(B, dtype=np.int32); x = np.zeros((B, n)); value = np.zeros(B)
        pr = _lib.PackedDualResults()
        pr.status, pr.x, pr.value = status.ctypes.data_as(_lib.ip), x.ctypes.data_as(_lib.dp), value.ctypes.data_as(_lib.dp)
        recs = basis = at = y = d = None
        if "rec" in want:
            recs = (_lib.PackedDualRecord * B)()
            pr.rec = recs
        if "basis" in want:
            basis = np.zeros((B, m), dtype=np.int32)
            pr.basis = basis.ctypes.data_as(_lib.ip)
        if "at_upper" in want:
            at = np.zeros((B, n), dtype=np.uint8)
            pr.at_upper = at.ctypes.data_as(C.POINTER(C.c_uint8))
        if "y" in want:
            y = np.zeros((B, m))
            pr.y = y.ctypes.data_as(_lib.dp)
        if "d" in want:
            d = np.zeros((B, n))
            pr.d = d.ctypes.data_as(_lib.dp)
        limit = max_iter if max_iter is not None else self.engine.get("max_iter")
        o = _lib.default_opts(True) if limit is None else _lib.default_opts(True, max_iter=int(limit))
        st = _lib.Stats()
        rc = lib().lpx_solve_packed_dual(C.byref(pm), _lib.BDUAL_LONG_STEP if long_step else 0, C.byref(o), C.byref(pr), C.byref(st))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        res = PackedDualResult(Status=status, Solution=x, OptimalValue=value, Basis=basis, AtUpper=at, Stats=st.as_dict(),
                               Duals=y, ReducedCosts=d)
        if recs is not None:
            r = np.frombuffer(recs, dtype=np.dtype([("status", "<i4"), ("events", "<i4"), ("kind0", "<i8"), ("kind1", "<i8"),
                                                    ("passes", "<i8"), ("dualize_flips", "<i8"), ("z", "<f8")]))
            res.Events = r["events"].copy()
            res.BoundCounts = np.stack([r["kind0"], r["kind1"], r["passes"]], axis=1)
            res.Passes = r["passes"].copy()
            res.DualizeFlips = r["dualize_flips"].copy()
            res.Z = r["z"].copy()
        return res

    def SolvePackedBnb(self, c, A, b, upper, lower=None, integer=None, sense="max", long_step: bool = False, cutoff: bool = False,
                       max_nodes: int = 100000, max_events: int = 2000000, max_iter=None, max_depth: int = 0, log_cap: int = 0,
                       want=("rec",)) -> PackedBnbResult:
        """B small integer programs of ONE shape (m rows, all <=; n variables) in ONE kernel launch (lpx_solve_packed_bnb): every
        workgroup runs the whole branch and bound of SolveBnbBounded(node_form="onchip") for its model with the tableau staying in
        LDS.  The arrays are SolvePacked's; integer: None (every variable) or (n,) flags shared by every model; integer variables
        need finite, integral bounds (else that model is LPX_EINVAL).  long_step / cutoff: the flags of SolveBnbBounded.  The
        budgets are per model and mandatory: max_nodes and max_events at least 1, max_iter (events per node and of the root LP;
        None: the engine's, else 10000), max_depth (0 = n).  Status per model: OPTIMAL, INFEASIBLE, ITER_LIMIT (a budget stopped the
        search, Stop says which, Solution / OptimalValue are the incumbent so far or zeros), the root's UNBOUNDED, or the model's own
        LPX_EINVAL / LPX_E_NEG_RHS.  Each entry is bit-equal to SolveBnbBounded(model, ..., node_form="onchip", max_nodes=) wherever
        max_events and max_depth do not bind.  log_cap > 0: Log, the first log_cap node records of every model, and Logged."""
        return self._solve_packed_bnb(False, c, A, b, None, upper, lower, integer, sense, long_step, cutoff, max_nodes, max_events,
                                      max_iter, max_depth, log_cap, want)

    def SolvePackedBnbDual(self, c, A, b, rel, upper, lower=None, integer=None, sense="max", long_step: bool = False,
                           cutoff: bool = False, max_nodes: int = 100000, max_events: int = 2000000, max_iter=None,
                           max_depth: int = 0, log_cap: int = 0, want=("rec",)) -> PackedBnbResult:
        """SolvePackedBnb from a dual start (lpx_solve_packed_bnb_dual): B small integer programs of ONE shape whose rows are <= or
        >= and whose right-hand sides may have either sign, in ONE kernel launch -- covering models, rows of both senses, an = row as
        its pair, right-hand-side sweeps across zero.  rel: None (every row <=), (m,) shared by every model or (B, m), as
        SolvePackedDual takes it; everything else is SolvePackedBnb's.  Status per model: OPTIMAL, INFEASIBLE (Stop "root": the root
        LP is infeasible, Nodes 0; Stop "done": the search ran empty without an incumbent), ITER_LIMIT, or the model's own
        LPX_EINVAL (its bounds, an integer variable's bounds, a bad entry of its own rel row, or a continuous variable that
        improves the objective and has no upper bound).  Each entry is bit-equal to SolveBnbBoundedDual(model, ...,
        node_form="onchip", max_nodes=) wherever max_events and max_depth do not bind."""
        return self._solve_packed_bnb(True, c, A, b, rel, upper, lower, integer, sense, long_step, cutoff, max_nodes, max_events,
                                      max_iter, max_depth, log_cap, want)

    def _solve_packed_bnb(self, dual, c, A, b, rel, upper, lower, integer, sense, long_step, cutoff, max_nodes, max_events, max_iter,
                          max_depth, log_cap, want) -> PackedBnbResult:
        """lpx_solve_packed_bnb, or with dual lpx_solve_packed_bnb_dual: the same call shape plus rel."""
        want = tuple(want)
        for w in want:
            if w not in ("rec",):
                raise ValueError(f"unknown output {w!r}")
        if int(max_nodes) < 1 or int(max_events) < 1:
            raise ValueError("max_nodes and max_events must be at least 1: the budgets of a packed search are mandatory")
        if int(max_depth) < 0 or int(log_cap) < 0:
            raise ValueError("max_depth and log_cap must not be negative")
        limit = max_iter if max_iter is not None else self.engine.get("max_iter")
        limit = 10000 if limit is None else int(limit)
        if limit < 0:
            raise ValueError("max_iter must not be negative")
        sense, c, A, b, bounds, rel, B, m, n = _packed_inputs(c, A, b, upper, lower, sense, rel)
        mask = None
        if integer is not None:
            mask = np.ascontiguousarray(np.asarray(integer)).astype(np.uint8)
            if mask.shape != (n,):
                raise ValueError(f"integer is (n,) with n = {n}: one mask shared by every model")

        def _stride(v, nd, packed):
            return packed if v.ndim == nd else 0
        pm = _lib.PackedBnbDualModels() if dual else _lib.PackedBnbModels()
        pm.count, pm.m, pm.n, pm.sense = B, m, n, int(sense)
        pm.c, pm.A, pm.b = (v.ctypes.data_as(_lib.dp) for v in (c, A, b))
        pm.c_stride, pm.A_stride, pm.b_stride = _stride(c, 2, n), _stride(A, 3, m * n), _stride(b, 2, m)
        for name in ("upper", "lower"):
            v = bounds[name]
            if v is not None:
                setattr(pm, name, v.ctypes.data_as(_lib.dp))
                setattr(pm, name + "_stride", _stride(v, 2, n))
        if mask is not None:
            pm.is_int = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        if dual and rel is not None:
            pm.rel, pm.rel_stride = rel.ctypes.data_as(_lib.ip), _stride(rel, 2, m)
        po = _lib.PackedBnbOpts((_lib.BDUAL_LONG_STEP if long_step else 0) | (_lib.BDUAL_CUTOFF if cutoff else 0), limit,
                                int(max_depth), int(log_cap), int(max_nodes), int(max_events))
        status = np.zeros(B, dtype=np.int32); x = np.zeros((B, n)); value = np.zeros(B)
        pr = _lib.PackedBnbResults()
        pr.status, pr.x, pr.value = status.ctypes.data_as(_lib.ip), x.ctypes.data_as(_lib.dp), value.ctypes.data_as(_lib.dp)
        recs = log = None
        if "rec" in want or log_cap > 0:
            recs = np.zeros(B, dtype=PACKED_BNB_DTYPE)
            pr.rec = recs.ctypes.data_as(C.POINTER(_lib.PackedBnbRecord))
        if log_cap > 0:
            log = np.zeros((B, int(log_cap)), dtype=BNB_LOG_DTYPE)
            pr.log = log.ctypes.data_as(C.POINTER(_lib.BnbNodeLog))
        st = _lib.Stats()
        call = lib().lpx_solve_packed_bnb_dual if dual else lib().lpx_solve_packed_bnb
        rc = call(C.byref(pm), C.byref(po), C.byref(pr), C.byref(st))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        res = PackedBnbResult(Status=status, Solution=x, OptimalValue=value, Stats=st.as_dict())
        if recs is not None:
            res.Stop, res.Nodes, res.Info = recs["stop"].copy(), recs["nodes"].copy(), recs
            res.Events = recs["events"].copy()
        if log is not None:
            res.Log, res.Logged = log, recs["logged"].copy()
        return res

    def _solve_bounded(self, problem: LPProblem, upper, lower, dual_flags, form: str = "launches") -> SimplexResult:
        """lpx_solve_bounded (dual_flags None; with a form, lpx_solve_bounded2) or lpx_solve_bounded_dual: the same call shape
        and result layout."""
        n = problem.NumVars
        o, keep = _solve_opts(self.engine)
        ps, hold = _problem_struct(problem)

        def _vec(v):
            if v is None:
                return None, None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)))
            return a, a.ctypes.data_as(_lib.dp)
        lo, lop = _vec(lower)
        up, upp = _vec(upper)
        r, info = _lib.Result(), _lib.BoundedInfo()
        if dual_flags is None and form != "launches":
            rc = lib().lpx_solve_bounded2(C.byref(ps), lop, upp, C.byref(o), _lib.NODE_FORMS[form], C.byref(r), C.byref(info))
        elif dual_flags is None:
            rc = lib().lpx_solve_bounded(C.byref(ps), lop, upp, C.byref(o), C.byref(r), C.byref(info))
        else:
            rc = lib().lpx_solve_bounded_dual(C.byref(ps), lop, upp, int(dual_flags), C.byref(o), C.byref(r), C.byref(info))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        res = self._bounded_result(r, info, n)
        self.FinalTableau = res.Tableau
        return res

    @staticmethod
    def _bounded_result(r, info, n) -> SimplexResult:
        """The result of a bounded solve from its lpx_result and lpx_bounded_info (which it frees)."""
        try:
            flips = _arr(info.flip, info.ncols, np.uint8)
        finally:
            lib().lpx_bounded_info_free(C.byref(info))
        res = _take_result(r, n)
        res.Flips = flips
        basic = np.zeros(len(flips), dtype=bool)
        if res.Basis is not None:
            basic[res.Basis[(res.Basis >= 0) & (res.Basis < len(flips))]] = True
        res.AtUpper = ((flips[:n] != 0) & ~basic[:n]).astype(np.uint8)
        res.BoundCounts = (int(res.Aux[0]), int(res.Aux[1]), int(res.Aux[2]))
        return res

    def SolveBnbBounded(self, problem: LPProblem, upper, lower=None, integer=None, max_nodes: int = 0,
                        long_step: bool = False, cutoff: bool = False, node_form: Optional[str] = None,
                        divers: Optional[int] = None, plunge: Optional[int] = None, branching: Optional[str] = None,
                        candidates: int = 4, probe_iter: Optional[int] = None,
                        stall_events: Optional[int] = None, root_form: Optional[str] = None,
                        root_cuts: Optional[int] = None, cuts_per_round: int = 8, max_active: int = 64,
                        cut_opts: Optional["CutOpts"] = None, tighten: bool = False) -> SimplexResult:
        """Branch and bound by bound changes on one device tableau (lpx_solve_bnb_bounded): lower <= x <= upper, x_j integer
        where integer[j] (None: every variable); integer variables need finite, integral bounds.  Status OPTIMAL or INFEASIBLE,
        Solution, OptimalValue (user's sense), Nodes, BnbInfo (counters) and BnbLog, a structured array with one record per node
        (depth, K, status, events, flips, var, z).  A node or search limit raises SolverException(ITER_LIMIT) whose .result
        holds the incumbent so far.  long_step / cutoff (lpx_solve_bnb_bounded2): every node's dual loop runs with the
        long-step ratio test / stops as soon as its objective has fallen to the incumbent + 1e-6 (such a node is logged with
        status CUTOFF and counted as pruned by bound); both off is lpx_solve_bnb_bounded.  node_form "onchip" | "auto"
        (lpx_solve_bnb_bounded3): every node is one kernel launch with the tableau in LDS ("auto": iff the root fits); the node
        log is bit-equal to "launches", the default.  divers=W (lpx_solve_bnb_bounded4): W handles dive at once, every round
        evaluates one node per diver on chip in one kernel launch; divers=1 gives the log of node_form="onchip", any W gives a
        log that depends on the model, the flags and W alone.  Use long_step=True with divers on larger models: another W visits
        other nodes, and without the long step some of them make max_iter events and end the solve with ITER_LIMIT (on
        binary_ip(128, 64), W = 4, 64 and 256 do; the long step makes it rare, not impossible; stall_events below ends such
        nodes).  The result then carries BnbInfo["rounds" / "steals" /
        "largest_batch"] and BnbRound / BnbDiver, the round and the diver of every log record.  plunge=D
        (lpx_solve_bnb_bounded5, 1 <= D <= 64; without divers it means divers=1): a diver's workgroup goes on from a node that
        branches into its ceil child, up to D nodes per launch with the tableau staying in LDS.  plunge=1 gives the log of
        divers=W, divers=1 with any plunge the log of node_form="onchip".  The result then also carries BnbStep (every record's
        index in its chain) and BnbInfo["launched" / "dropped" / "longest_chain"].  branching "most_fractional" | "strong"
        (lpx_solve_bnb_bounded6; None: the paths above, unchanged; without divers it means divers=1): "strong" probes both
        children of up to `candidates` (1..32) fractional columns of every evaluated node in a second launch of the same round,
        at most probe_iter events each (None: the engine's max_iter), branches on the first largest product of the two
        objective losses and never pushes a child whose probe ended infeasible, cut off or not above the incumbent + 1e-6;
        "most_fractional" gives the log of divers=W.  BnbInfo then carries probe_launches, probes, probe_events, probe_limit,
        pruned_by_probe and changed_picks.  It is a rule beside the default one: it visits fewer nodes and pays for every
        node with a second launch.  stall_events=S (lpx_solve_bnb_bounded7; None: the paths above, unchanged; without divers
        it means divers=1): the search by divers whose nodes run with the stall guard -- after S pivots without progress of the
        objective a node's loop selects by Bland's rule until the objective moves again, so a node that cycles at a degenerate
        vertex ends instead of making max_iter events.  0 gives the log of divers=W; 50 is a reasonable value.  BnbInfo then
        carries guarded_nodes, bland_events and max_events.  It cannot be combined with node_form="launches", plunge > 1 or
        branching: those have no guard.  root_form "launches" | "onchip" | "auto" (lpx_solve_bnb_bounded8; None: the paths above,
        unchanged; without divers it means divers=1, without stall_events stall_events=0): the search by divers whose root LP
        is solved in that form; the node log is the same for every form.  It cannot be combined with node_form="launches",
        plunge or branching: those drivers have no root form.  root_cuts=N (lpx_solve_bnb_bounded9; None: the paths above,
        unchanged; without root_form it means root_form="launches"): cut-and-branch -- up to N rounds of cuts_per_round GMI cuts
        at the solved root (lpx_bounded_cut_loop) on a handle with up to max_active spare rows and columns, then the search by
        divers from that handle; cut_opts (a CutOpts) gives every option of the loop instead.  BnbInfo then carries cut_ran,
        cut_spare, cut_rounds, cuts_added, cuts_purged, cut_events, cut_stop, cut_R and cut_C, and the result CutZ, an array
        [rounds, 2] of the LP objective in front of and behind every round (internal sense).  Whether the tree shrinks depends
        on the model.  It cannot be combined with node_form="launches", plunge or branching.  tighten=True
        (lpx_solve_bnb_bounded10; False: the paths above, unchanged; without root_form it means root_form="launches"):
        reduced-cost tightening -- from the first incumbent on, every node that ends OPTIMAL above the incumbent + 1e-6 shrinks,
        in its own launch, the range of every nonbasic integer column whose reduced cost leaves it less room than its range,
        and the tighter ranges hold for the node's subtree.  BnbInfo then carries tightened_nodes, tightened_cols and
        max_per_node.  The tree usually shrinks; no speed-up is promised, and the default stays off.  It cannot be combined
        with node_form="launches", plunge or branching: those have no tightening."""
        if tighten:
            if node_form == "launches":
                raise ValueError("reduced-cost tightening has no launches form: tighten cannot be combined with node_form='launches'")
            if plunge is not None:
                raise ValueError("the plunge driver has no tightening: tighten cannot be combined with plunge")
            if branching is not None:
                raise ValueError("the strong-branching driver has no tightening: tighten cannot be combined with branching")
            if root_form is None:
                root_form = "launches"
        if root_cuts is not None or cut_opts is not None:
            if node_form == "launches":
                raise ValueError("root cuts belong to the search by divers: they cannot be combined with node_form='launches'")
            if plunge is not None:
                raise ValueError("the plunge driver has no root cuts: root_cuts cannot be combined with plunge")
            if branching is not None:
                raise ValueError("the strong-branching driver has no root cuts: root_cuts cannot be combined with branching")
            if cut_opts is None:
                cut_opts = CutOpts(cuts_per_round=int(cuts_per_round), max_rounds=int(root_cuts), max_active=int(max_active))
            if root_form is None:
                root_form = "launches"
        if root_form is not None:
            if root_form not in _lib.NODE_FORMS:
                raise ValueError(f"unknown root form {root_form!r}")
            if node_form == "launches":
                raise ValueError("root_form belongs to the search by divers: it cannot be combined with node_form='launches'")
            if plunge is not None:
                raise ValueError("the plunge driver has no root form: root_form cannot be combined with plunge")
            if branching is not None:
                raise ValueError("the strong-branching driver has no root form: root_form cannot be combined with branching")
            if stall_events is None:
                stall_events = 0
        if stall_events is not None:
            if int(stall_events) < 0:
                raise ValueError(f"stall_events = {stall_events}: stall_events must not be negative")
            if node_form == "launches":
                raise ValueError("the stall guard has no launches form: stall_events cannot be combined with node_form='launches'")
            if plunge is not None and plunge > 1:
                raise ValueError("the plunge has no stall guard: stall_events cannot be combined with plunge > 1")
            if branching is not None:
                raise ValueError("the probes have no stall guard: stall_events cannot be combined with branching")
            if divers is None:
                divers = 1
            plunge = None
        if branching is not None:
            if branching not in _lib.BRANCHINGS:
                raise ValueError(f"unknown branching rule {branching!r}")
            if node_form == "launches":
                raise ValueError("branching evaluates every node on chip: it cannot be combined with node_form='launches'")
            if plunge is not None and plunge > 1:      # a chain has no host decision between its nodes
                raise ValueError("a branching rule decides on the host between a node and its children: it cannot be combined "
                                 "with plunge > 1")
            if divers is None:
                divers = 1
            plunge = None
        if plunge is not None and node_form == "launches":
            raise ValueError("plunge evaluates every node on chip: it cannot be combined with node_form='launches'")
        if plunge is not None and divers is None:
            divers = 1
        if divers is not None and node_form == "launches":
            raise ValueError("divers evaluates every node on chip: it cannot be combined with node_form='launches'")
        if node_form is None:               # not given: "launches", the default; with divers every node is on chip
            node_form = "launches" if divers is None else "onchip"
        if node_form not in _lib.NODE_FORMS:
            raise ValueError(f"unknown node form {node_form!r}")
        n = problem.NumVars
        o, keep = _solve_opts(self.engine)
        ps, hold = _problem_struct(problem)

        def _vec(v):
            if v is None:
                return None, None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)))
            return a, a.ctypes.data_as(_lib.dp)
        lo, lop = _vec(lower)
        up, upp = _vec(upper)
        mask, mp = None, None
        if integer is not None:
            mask = np.ascontiguousarray(np.broadcast_to(np.asarray(integer, dtype=np.uint8), (n,)))
            mp = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        r, info, dinfo, pinfo = _lib.Result(), _lib.BnbBoundedInfo(), _lib.BnbDiversInfo(), _lib.BnbPlungeInfo()
        flags = (_lib.BDUAL_LONG_STEP if long_step else 0) | (_lib.BDUAL_CUTOFF if cutoff else 0)
        sinfo = _lib.BnbStrongInfo()
        ginfo = _lib.BnbGuardInfo()
        cinfo = _lib.BnbCutInfo()
        finfo = _lib.BnbFixInfo()
        if tighten:
            co = cut_opts.to_c() if cut_opts is not None else None
            rc = lib().lpx_solve_bnb_bounded10(C.byref(ps), lop, upp, mp, C.byref(o), int(max_nodes), flags, int(divers),
                                               int(stall_events), _lib.NODE_FORMS[root_form], C.byref(co) if co is not None else None,
                                               1, C.byref(r), C.byref(info), C.byref(dinfo), C.byref(ginfo), C.byref(cinfo),
                                               C.byref(finfo))
        elif cut_opts is not None:
            co = cut_opts.to_c()
            rc = lib().lpx_solve_bnb_bounded9(C.byref(ps), lop, upp, mp, C.byref(o), int(max_nodes), flags, int(divers),
                                              int(stall_events), _lib.NODE_FORMS[root_form], C.byref(co), C.byref(r), C.byref(info),
                                              C.byref(dinfo), C.byref(ginfo), C.byref(cinfo))
        elif root_form is not None:
            rc = lib().lpx_solve_bnb_bounded8(C.byref(ps), lop, upp, mp, C.byref(o), int(max_nodes), flags, int(divers),
                                              int(stall_events), _lib.NODE_FORMS[root_form], C.byref(r), C.byref(info), C.byref(dinfo),
                                              C.byref(ginfo))
        elif stall_events is not None:
            rc = lib().lpx_solve_bnb_bounded7(C.byref(ps), lop, upp, mp, C.byref(o), int(max_nodes), flags, int(divers),
                                              int(stall_events), C.byref(r), C.byref(info), C.byref(dinfo), C.byref(ginfo))
        elif branching is not None:
            cand = int(candidates)
            if cand < 1 or cand > 32:
                raise ValueError(f"candidates = {cand}: candidates must be in [1, 32]")
            rc = lib().lpx_solve_bnb_bounded6(C.byref(ps), lop, upp, mp, C.byref(o), int(max_nodes), flags, int(divers),
                                              _lib.BRANCHINGS[branching], cand, int((o.max_iter or 10000) if probe_iter is None else probe_iter),
                                              C.byref(r), C.byref(info), C.byref(dinfo), C.byref(sinfo))
        elif plunge is not None:
            rc = lib().lpx_solve_bnb_bounded5(C.byref(ps), lop, upp, mp, C.byref(o), int(max_nodes), flags, int(divers), int(plunge),
                                              C.byref(r), C.byref(info), C.byref(dinfo), C.byref(pinfo))
        elif divers is not None:
            rc = lib().lpx_solve_bnb_bounded4(C.byref(ps), lop, upp, mp, C.byref(o), int(max_nodes), flags, int(divers),
                                              C.byref(r), C.byref(info), C.byref(dinfo))
        elif node_form != "launches":
            rc = lib().lpx_solve_bnb_bounded3(C.byref(ps), lop, upp, mp, C.byref(o), int(max_nodes), flags, _lib.NODE_FORMS[node_form],
                                              C.byref(r), C.byref(info))
        elif flags:
            rc = lib().lpx_solve_bnb_bounded2(C.byref(ps), lop, upp, mp, C.byref(o), int(max_nodes), flags, C.byref(r), C.byref(info))
        else:
            rc = lib().lpx_solve_bnb_bounded(C.byref(ps), lop, upp, mp, C.byref(o), int(max_nodes), C.byref(r), C.byref(info))
        if rc != 0 and rc != _lib.ITER_LIMIT:
            raise SolverException(rc, _lib.last_error())
        msg = _lib.last_error() if rc else ""
        try:
            log = np.zeros(info.n_log, dtype=BNB_LOG_DTYPE)
            if info.n_log:
                C.memmove(log.ctypes.data, info.log, info.n_log * C.sizeof(_lib.BnbNodeLog))
            counters = {k: getattr(info, k) for k in ("nodes", "events", "flips", "incumbents", "pruned_bound",
                                                      "pruned_infeasible", "max_K", "constant")}
            if divers is not None:
                counters.update({k: getattr(dinfo, k) for k in ("rounds", "steals", "largest_batch")})
                rounds = np.ctypeslib.as_array(dinfo.round, (info.n_log,)).copy() if info.n_log else np.zeros(0, dtype=np.int32)
                who = np.ctypeslib.as_array(dinfo.diver, (info.n_log,)).copy() if info.n_log else np.zeros(0, dtype=np.int32)
            if branching is not None:
                counters.update({k: getattr(sinfo, k) for k in ("probe_launches", "probes", "probe_events", "probe_limit",
                                                                "pruned_by_probe", "changed_picks")})
            if stall_events is not None:
                counters.update({k: getattr(ginfo, k) for k in ("guarded_nodes", "bland_events", "max_events")})
            if tighten:
                counters.update({k: getattr(finfo, k) for k in ("tightened_nodes", "tightened_cols", "max_per_node")})
            if cut_opts is not None:
                counters.update(cut_ran=cinfo.ran, cut_spare=cinfo.spare, cut_rounds=cinfo.rounds, cuts_added=cinfo.added,
                                cuts_purged=cinfo.purged, cut_events=cinfo.events, cut_stop=_lib.CUTLOOP_STOPS[cinfo.stop] if cinfo.ran else None,
                                cut_R=cinfo.R, cut_C=cinfo.C)
                cutz = np.zeros((cinfo.n_z, 2))
                for i in range(cinfo.n_z):
                    cutz[i] = cinfo.z_before[i], cinfo.z_after[i]
            if plunge is not None:
                counters.update({k: getattr(pinfo, k) for k in ("launched", "dropped", "longest_chain")})
                step = np.ctypeslib.as_array(pinfo.step, (info.n_log,)).copy() if info.n_log else np.zeros(0, dtype=np.int32)
        finally:
            lib().lpx_bnb_bounded_info_free(C.byref(info))
            lib().lpx_bnb_divers_info_free(C.byref(dinfo))
            lib().lpx_bnb_plunge_info_free(C.byref(pinfo))
            lib().lpx_bnb_cut_info_free(C.byref(cinfo))
        res = _take_result(r, n)
        res.BnbLog, res.BnbInfo = log, counters
        if cut_opts is not None:
            res.CutZ = cutz
        if divers is not None:
            res.BnbRound, res.BnbDiver = rounds, who
        if plunge is not None:
            res.BnbStep = step
        if rc != 0:
            e = SolverException(rc, msg)
            e.result = res
            raise e
        return res

    def SolveBnbBoundedDual(self, problem: LPProblem, upper, lower=None, integer=None, max_nodes: int = 0, long_step: bool = False,
                            cutoff: bool = False, node_form: Optional[str] = None) -> SimplexResult:
        """SolveBnbBounded whose root is the dual start of SolveBoundedDual (lpx_solve_bnb_bounded_dual): >= rows, an = row as its
        pair and right-hand sides of either sign are accepted -- covering models, rows of both senses.  The arguments, the result,
        BnbInfo, BnbLog and the limits are SolveBnbBounded's for node_form ("launches", the default, "onchip" or "auto"; the node
        logs of "launches" and "onchip" are bit-equal).  A root LP that is infeasible gives Status INFEASIBLE with Nodes 0; so can a
        search that runs empty without an incumbent.  A continuous variable that improves the objective needs a finite upper bound."""
        if node_form is None:
            node_form = "launches"
        if node_form not in _lib.NODE_FORMS:
            raise ValueError(f"unknown node form {node_form!r}")
        n = problem.NumVars
        o, keep = _solve_opts(self.engine)
        ps, hold = _problem_struct(problem)

        def _vec(v):
            if v is None:
                return None, None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)))
            return a, a.ctypes.data_as(_lib.dp)
        lo, lop = _vec(lower)
        up, upp = _vec(upper)
        mask, mp = None, None
        if integer is not None:
            mask = np.ascontiguousarray(np.broadcast_to(np.asarray(integer, dtype=np.uint8), (n,)))
            mp = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        r, info = _lib.Result(), _lib.BnbBoundedInfo()
        flags = (_lib.BDUAL_LONG_STEP if long_step else 0) | (_lib.BDUAL_CUTOFF if cutoff else 0)
        rc = lib().lpx_solve_bnb_bounded_dual(C.byref(ps), lop, upp, mp, C.byref(o), int(max_nodes), flags, _lib.NODE_FORMS[node_form],
                                              C.byref(r), C.byref(info))
        if rc != 0 and rc != _lib.ITER_LIMIT:
            raise SolverException(rc, _lib.last_error())
        msg = _lib.last_error() if rc else ""
        try:
            log = np.zeros(info.n_log, dtype=BNB_LOG_DTYPE)
            if info.n_log:
                C.memmove(log.ctypes.data, info.log, info.n_log * C.sizeof(_lib.BnbNodeLog))
            counters = {k: getattr(info, k) for k in ("nodes", "events", "flips", "incumbents", "pruned_bound",
                                                      "pruned_infeasible", "max_K", "constant")}
        finally:
            lib().lpx_bnb_bounded_info_free(C.byref(info))
        res = _take_result(r, n)
        res.BnbLog, res.BnbInfo = log, counters
        if rc != 0:
            e = SolverException(rc, msg)
            e.result = res
            raise e
        return res

    def OpenBounded(self, problem: LPProblem, upper=None, lower=None) -> "BoundedSession":
        """SolveBounded that keeps its device tableau (lpx_bounded_open): .result is SolveBounded's result, then
        .set_bounds(vars, lower, upper) tightens, fixes or loosens bounds and re-optimises with the bounded dual simplex."""
        return BoundedSession(problem, upper=upper, lower=lower, **self.engine)

    def OpenPackedBase(self, c, A, b, rel=None, upper=None, lower=None, sense="max", long_step: bool = True,
                       max_iter=None) -> "PackedBase":
        """ONE model (c (n,), A (m, n), b (m,), rel / upper / lower as SolvePackedDual takes them without the batch axis) solved by
        the dual start and kept on the device (lpx_packed_base_open): .Base is SolvePackedDual's result for it, and
        .solve(b) re-solves a batch of right-hand sides of that model in ONE launch, every workgroup continuing from the base's
        optimal basis.  A base that is not OPTIMAL raises SolverException with its status as the code."""
        limit = max_iter if max_iter is not None else self.engine.get("max_iter")
        return PackedBase(c, A, b, rel, upper, lower, sense, long_step, limit)

    def Open(self, problem: LPProblem, **opts) -> "ModelSession":
        """A warm post-optimal session on the device (lpx_session_open): the model is solved once, then ChangeRHS /
        ChangeCost / AddActivity / AddConstraint each re-optimise from the current basis.  opts: extra_rows, extra_cols,
        max_iter, batch, want_tableau (lpx_session_opts)."""
        return ModelSession(problem, **opts)


def _packed_dual_outputs(B, m, n):
    """Every output array of an lpx_packed_dual_results for B models, the struct over them and a function that makes the result."""
    status = np.zeros(B, dtype=np.int32); x = np.zeros((B, n)); value = np.zeros(B)
    recs = (_lib.PackedDualRecord * B)()
    basis = np.zeros((B, m), dtype=np.int32); at = np.zeros((B, n), dtype=np.uint8); y = np.zeros((B, m)); d = np.zeros((B, n))
    pr = _lib.PackedDualResults(status.ctypes.data_as(_lib.ip), x.ctypes.data_as(_lib.dp), value.ctypes.data_as(_lib.dp), recs,
                                basis.ctypes.data_as(_lib.ip), at.ctypes.data_as(C.POINTER(C.c_uint8)), y.ctypes.data_as(_lib.dp),
                                d.ctypes.data_as(_lib.dp))

    def take(stats):
        r = np.frombuffer(recs, dtype=np.dtype([("status", "<i4"), ("events", "<i4"), ("kind0", "<i8"), ("kind1", "<i8"),
                                                ("passes", "<i8"), ("dualize_flips", "<i8"), ("z", "<f8")]))
        return PackedDualResult(Status=status, Solution=x, OptimalValue=value, Basis=basis, AtUpper=at, Stats=stats, Duals=y,
                                ReducedCosts=d, Events=r["events"].copy(), BoundCounts=np.stack([r["kind0"], r["kind1"], r["passes"]], axis=1),
                                Passes=r["passes"].copy(), DualizeFlips=r["dualize_flips"].copy(), Z=r["z"].copy())
    return pr, take


class PackedBase:           # lpx_packed_base (include/lpx.h): right-hand-side scenarios warm-started from one solved model
    def __init__(self, c, A, b, rel=None, upper=None, lower=None, sense="max", long_step: bool = True, max_iter=None):
        self._h = None
        sense, c, A, b, bounds, rel, B, m, n = _packed_inputs(c, A, b, upper, lower, sense, rel)
        if c.ndim != 1 or A.ndim != 2 or b.ndim != 1 or any(v is not None and v.ndim != 1 for v in (bounds["upper"], bounds["lower"], rel)):
            raise ValueError("the base is one model: c (n,), A (m, n), b (m,), rel (m,), upper / lower (n,) or a scalar")
        self.m, self.n = m, n
        pm = _lib.PackedBaseModel()
        pm.m, pm.n, pm.sense = m, n, int(sense)
        pm.c, pm.A, pm.b = (v.ctypes.data_as(_lib.dp) for v in (c, A, b))
        for name in ("upper", "lower"):
            if bounds[name] is not None:
                setattr(pm, name, bounds[name].ctypes.data_as(_lib.dp))
        if rel is not None:
            pm.rel = rel.ctypes.data_as(_lib.ip)
        pr, take = _packed_dual_outputs(1, m, n)
        o = _lib.default_opts(True) if max_iter is None else _lib.default_opts(True, max_iter=int(max_iter))
        h = C.c_void_p()
        rc = lib().lpx_packed_base_open(C.byref(pm), _lib.BDUAL_LONG_STEP if long_step else 0, C.byref(o), C.byref(pr), C.byref(h))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        self._h = h
        self._max_iter = max_iter
        self.Base = take(None)

    def solve(self, b, long_step: bool = True, max_iter=None) -> PackedDualResult:
        """b: (B, m) or (m,) right-hand sides of the base's model, re-solved in ONE launch (lpx_packed_base_solve).  Every scenario
        gets its own Status: OPTIMAL, INFEASIBLE, ITER_LIMIT, or LPX_EINVAL for a right-hand side that is not finite.  Events and
        BoundCounts count the scenario's own loop; DualizeFlips is 0.  max_iter: None = the one the base was opened with."""
        if self._h is None:
            raise SolverException(_lib.EINVAL, "the packed base is closed")
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float64))
        if b.ndim == 1:
            b = b[None, :]
        if b.ndim != 2 or b.shape[1] != self.m or b.shape[0] < 1:
            raise ValueError(f"b is (B, m) or (m,) with m = {self.m}")
        B = b.shape[0]
        pr, take = _packed_dual_outputs(B, self.m, self.n)
        limit = max_iter if max_iter is not None else self._max_iter
        o = _lib.default_opts(True) if limit is None else _lib.default_opts(True, max_iter=int(limit))
        st = _lib.Stats()
        rc = lib().lpx_packed_base_solve(self._h, B, b.ctypes.data_as(_lib.dp), _lib.BDUAL_LONG_STEP if long_step else 0, C.byref(o),
                                         C.byref(pr), C.byref(st))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        return take(st.as_dict())

    def solve_costs(self, c, b=None, long_step: bool = True, max_iter=None, primal_max_iter=None,
                    dual_max_iter=None) -> PackedCostResult:
        """c: (B, n) or (n,) cost vectors of the base's model; b: None (every scenario keeps the base's right-hand side), (B, m) or
        (m,), broadcast against c's batch.  ONE launch (lpx_packed_base_solve_costs): every workgroup moves the objective row of
        the base's solved tableau, continues the bounded primal loop from the base's basis and, with b, moves the RHS column and
        continues the dual loop.  Every scenario gets its own Status: OPTIMAL, UNBOUNDED, INFEASIBLE, ITER_LIMIT, or LPX_EINVAL for
        a cost or a right-hand side that is not finite.  max_iter: the limit of both loops; primal_max_iter / dual_max_iter: the
        limit of one loop alone, in front of max_iter.  With none given the dual loop takes the limit the base was opened with
        (which was a dual loop's) and the primal loop its default."""
        if self._h is None:
            raise SolverException(_lib.EINVAL, "the packed base is closed")
        c = np.asarray(c, dtype=np.float64)
        if c.ndim == 1:
            c = c[None, :]
        if c.ndim != 2 or c.shape[1] != self.n or c.shape[0] < 1:
            raise ValueError(f"c is (B, n) or (n,) with n = {self.n}")
        if b is not None:
            b = np.asarray(b, dtype=np.float64)
            if b.ndim == 1:
                b = b[None, :]
            if b.ndim != 2 or b.shape[1] != self.m or b.shape[0] < 1:
                raise ValueError(f"b is None, (B, m) or (m,) with m = {self.m}")
            if b.shape[0] != c.shape[0] and 1 not in (b.shape[0], c.shape[0]):
                raise ValueError(f"c has {c.shape[0]} scenarios and b has {b.shape[0]}")
            B = max(b.shape[0], c.shape[0])
            b = np.ascontiguousarray(np.broadcast_to(b, (B, self.m)))
            c = np.broadcast_to(c, (B, self.n))
        c = np.ascontiguousarray(c)
        B, m, n = c.shape[0], self.m, self.n
        status = np.zeros(B, dtype=np.int32); x = np.zeros((B, n)); value = np.zeros(B)
        recs = (_lib.PackedCostRecord * B)()
        basis = np.zeros((B, m), dtype=np.int32); at = np.zeros((B, n), dtype=np.uint8); y = np.zeros((B, m)); d = np.zeros((B, n))
        pr = _lib.PackedCostResults(status.ctypes.data_as(_lib.ip), x.ctypes.data_as(_lib.dp), value.ctypes.data_as(_lib.dp), recs,
                                    basis.ctypes.data_as(_lib.ip), at.ctypes.data_as(C.POINTER(C.c_uint8)), y.ctypes.data_as(_lib.dp),
                                    d.ctypes.data_as(_lib.dp))
        p_limit = primal_max_iter if primal_max_iter is not None else max_iter
        d_limit = dual_max_iter if dual_max_iter is not None else max_iter if max_iter is not None else self._max_iter
        op, od = ((_lib.default_opts(dual) if limit is None else _lib.default_opts(dual, max_iter=int(limit)))
                  for dual, limit in ((False, p_limit), (True, d_limit)))
        st = _lib.Stats()
        rc = lib().lpx_packed_base_solve_costs(self._h, B, c.ctypes.data_as(_lib.dp), None if b is None else b.ctypes.data_as(_lib.dp),
                                               _lib.BDUAL_LONG_STEP if long_step else 0, C.byref(op), C.byref(od), C.byref(pr), C.byref(st))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        r = np.frombuffer(recs, dtype=PACKED_COST_DTYPE)
        return PackedCostResult(Status=status, Solution=x, OptimalValue=value, Events=r["primal_events"] + r["dual_events"], Z=r["z"].copy(),
                                Basis=basis, AtUpper=at, Stats=st.as_dict(), Duals=y, ReducedCosts=d,
                                PrimalEvents=r["primal_events"].copy(), DualEvents=r["dual_events"].copy(),
                                PrimalCounts=np.stack([r["primal_kind0"], r["primal_kind1"], r["primal_flips"]], axis=1),
                                DualCounts=np.stack([r["dual_kind0"], r["dual_kind1"], r["dual_passes"]], axis=1))

    def close(self):
        if self._h is not None:
            lib().lpx_packed_base_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BoundedSession:       # lpx_bounded_session (include/lpx.h): bound edits re-optimised from the solved tableau
    def __init__(self, problem: LPProblem, upper=None, lower=None, **engine):
        n = problem.NumVars
        self.n = n
        o, keep = _solve_opts(engine)
        ps, hold = _problem_struct(problem)

        def _vec(v):
            if v is None:
                return None, None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)))
            return a, a.ctypes.data_as(_lib.dp)
        lo, lop = _vec(lower)
        up, upp = _vec(upper)
        h = C.c_void_p()
        r = _lib.Result()
        self._h = None
        rc = lib().lpx_bounded_open(C.byref(ps), lop, upp, C.byref(o), C.byref(h), C.byref(r))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        self._h = h
        self.result = self._take(r)

    def _take(self, r) -> SimplexResult:
        res = _take_result(r, self.n)
        res.BoundCounts = (int(res.Aux[0]), int(res.Aux[1]), int(res.Aux[2]))
        return res

    def set_bounds(self, vars, lower, upper) -> SimplexResult:
        """lower[k] <= x_vars[k] <= upper[k] (the user's absolute bounds; scalars broadcast), then the bounded dual simplex from
        the tableau as it stands.  Status OPTIMAL or INFEASIBLE; Trace / Stats are this edit's; BoundCounts = (kind 0, kind 1, 1)."""
        if self._h is None:
            raise SolverException(_lib.EINVAL, "session is closed")
        idx = np.ascontiguousarray(np.atleast_1d(vars), dtype=np.int32)
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lower, dtype=np.float64), idx.shape))
        up = np.ascontiguousarray(np.broadcast_to(np.asarray(upper, dtype=np.float64), idx.shape))
        r = _lib.Result()
        rc = lib().lpx_bounded_set_bounds(self._h, len(idx), idx.ctypes.data_as(_lib.ip), lo.ctypes.data_as(_lib.dp),
                                          up.ctypes.data_as(_lib.dp), C.byref(r))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        self.result = self._take(r)
        return self.result

    def close(self):
        if self._h is not None:
            lib().lpx_bounded_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ModelSession:         # lpx_session (include/lpx.h): warm re-optimisation after model edits
    def __init__(self, problem: LPProblem, **opts):
        L = lib()
        o = _lib.SessionOpts()
        L.lpx_default_session_opts(C.byref(o))
        for k, v in opts.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown session option {k!r}")
            setattr(o, k, int(v))
        self._want_T = bool(o.want_tableau)
        self.Problem = LPProblem(ObjectiveSense=problem.ObjectiveSense, C=list(problem.C),
                                 Constraints=[Constraint(A=list(k.A), Relation=k.Relation, B=k.B) for k in problem.Constraints])
        ps, hold = _problem_struct(problem)
        h = C.c_void_p()
        r = _lib.Result()
        rc = L.lpx_session_open(C.byref(ps), C.byref(o), C.byref(h), C.byref(r))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        self._h = h
        self.Result = self._take(r)

    def _take(self, r) -> SimplexResult:
        n = r.n
        has_T = bool(r.T) and self._want_T
        T = _arr(r.T, r.R * r.C, np.float64).reshape(r.R, r.C) if has_T else None
        try:
            res = SimplexResult(
                Report=(r.report or b"").decode(errors="replace"), Summary=(r.summary or b"").decode(errors="replace"),
                OptimalValue=r.optimal_value, Solution=_arr(r.x, n, np.float64), Tableau=T,
                Basis=_arr(r.basis, max(r.R - 1, 0), np.int32), VarNames=None, Status=r.status,
                Trace=_arr(r.trace, 2 * r.n_pivots, np.int32).reshape(-1, 2), LpSolves=r.lp_solves, Nodes=r.nodes,
                Aux=list(r.aux), Stats=r.stats.as_dict())
        finally:
            lib().lpx_result_free(C.byref(r))
        return res

    def _call(self, fn, *args) -> SimplexResult:
        if self._h is None:
            raise SolverException(_lib.EINVAL, "session is closed")
        r = _lib.Result()
        rc = fn(self._h, *args, C.byref(r))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        self.Result = self._take(r)
        return self.Result

    def ChangeRHS(self, i, value) -> SimplexResult:
        """b_i = value (i and value may be sequences: one edit of several right-hand sides)."""
        idx = np.atleast_1d(np.asarray(i, dtype=np.int32))
        val = np.atleast_1d(np.asarray(value, dtype=np.float64))
        res = self._call(lib().lpx_session_set_rhs, len(idx), idx.ctypes.data_as(_lib.ip), val.ctypes.data_as(_lib.dp))
        for k, v in zip(idx, val):
            self.Problem.Constraints[int(k)].B = float(v)
        return res

    def ChangeCost(self, j, value) -> SimplexResult:
        """c_j = value (j and value may be sequences)."""
        idx = np.atleast_1d(np.asarray(j, dtype=np.int32))
        val = np.atleast_1d(np.asarray(value, dtype=np.float64))
        res = self._call(lib().lpx_session_set_cost, len(idx), idx.ctypes.data_as(_lib.ip), val.ctypes.data_as(_lib.dp))
        for k, v in zip(idx, val):
            self.Problem.C[int(k)] = float(v)
        return res

    def AddActivity(self, c: float, column) -> SimplexResult:
        """A new variable with cost c and constraint coefficients `column` (one per constraint)."""
        col = np.ascontiguousarray(column, dtype=np.float64)
        if col.shape != (len(self.Problem.Constraints),):
            raise SolverException(_lib.EINVAL, "column needs one coefficient per constraint")
        res = self._call(lib().lpx_session_add_variable, float(c), col.ctypes.data_as(_lib.dp))
        self.Problem.C.append(float(c))
        for k, a in zip(self.Problem.Constraints, col):
            k.A.append(float(a))
        return res

    def AddConstraint(self, coeffs, rel, b: float) -> SimplexResult:
        """A new constraint coeffs . x (rel) b over every current variable."""
        a = np.ascontiguousarray(coeffs, dtype=np.float64)
        if a.shape != (self.Problem.NumVars,):
            raise SolverException(_lib.EINVAL, "coeffs needs one coefficient per variable")
        res = self._call(lib().lpx_session_add_constraint, a.ctypes.data_as(_lib.dp), int(rel), float(b))
        self.Problem.Constraints.append(Constraint(A=[float(v) for v in a], Relation=Rel(int(rel)), B=float(b)))
        return res

    def Ranging(self) -> RangingReport:
        """Ranging of the current basis in user terms (lpx_session_ranging); *_at name columns of the session tableau."""
        if self._h is None:
            raise SolverException(_lib.EINVAL, "session is closed")
        L = lib()
        g = _lib.Ranging()
        rc = L.lpx_session_ranging(self._h, C.byref(g))
        if rc != 0:
            raise SolverException(rc, _lib.last_error())
        try:
            return RangingReport(
                valid=bool(g.valid),
                cost_lo=_arr(g.cost_lo, g.n, np.float64), cost_hi=_arr(g.cost_hi, g.n, np.float64),
                cost_lo_at=_arr(g.cost_lo_at, g.n, np.int32), cost_hi_at=_arr(g.cost_hi_at, g.n, np.int32),
                reduced_cost=_arr(g.reduced_cost, g.n, np.float64),
                rhs_lo=_arr(g.rhs_lo, g.m, np.float64), rhs_hi=_arr(g.rhs_hi, g.m, np.float64),
                rhs_lo_at=_arr(g.rhs_lo_at, g.m, np.int32), rhs_hi_at=_arr(g.rhs_hi_at, g.m, np.int32),
                dual=_arr(g.dual, g.m, np.float64), min_rhs=g.min_rhs, min_dj=g.min_dj)
        finally:
            L.lpx_ranging_free(C.byref(g))

    def Close(self):
        if self._h is not None:
            lib().lpx_session_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.Close()

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass


def _algorithm_key(name: str) -> str:
    """The key lpx_solve matches algorithm names by (LPSolver.NormalizeAlgorithmKey, Models/LPSolver.cs:61-76): lower case,
    every "algorithm" removed, white space collapsed."""
    return " ".join(name.lower().replace("algorithm", "").split())


def _gmi_names(res: "SimplexResult", problem: LPProblem):
    """VarNames of a GMI result: x1..xn, the slacks of the prepared rows c1.., then the live cut slacks g1.. in column order."""
    if res.Tableau is None:
        return
    n = problem.NumVars
    ms = sum(2 if int(k.Relation) == int(Rel.EQ) else 1 for k in problem.Constraints)
    ncol = res.Tableau.shape[1] - 1
    res.VarNames = ([f"x{j + 1}" for j in range(n)] + [f"c{j + 1}" for j in range(ms)] +
                    [f"g{k + 1}" for k in range(ncol - n - ms)])


class _Algo:                # ILPAlgorithm, Models/IPLAlgorithm.cs:5-8
    NAME = ""

    def __init__(self, **engine):
        self._solver = LPSolver(**engine)

    def Solve(self, problem: LPProblem, updatePivot=None) -> SimplexResult:
        return self._solver.Solve(problem, self.NAME, updatePivot)


class PrimalSimplex(_Algo):             # Models/PrimalSimplex.cs:52
    NAME = "Primal Simplex"


class RevisedPrimalSimplex(_Algo):      # Models/RevisedPrimalSimplex.cs:12
    NAME = "Revised Primal Simplex"


class DualSimplex(_Algo):               # Models/DualSimplex.cs:11
    NAME = "Dual Simplex"


class BranchAndBound(_Algo):            # Models/Branch&Bound.cs:20
    NAME = "Branch and Bound"


class BranchAndBoundRevised(_Algo):     # Models/BranchAndBoundRevised.cs:17
    NAME = "Revised Branch and Bound"


class BranchAndBoundKnapsack(_Algo):    # Models/BranchAndBoundKnapsack.cs:12
    NAME = "Branch and Bound Knapsack"


class CuttingPlane(_Algo):              # Models/CuttingPlane.cs:9 (built by Form1.cs:251, not by LPSolver)
    NAME = "Cutting Plane"


class CuttingPlaneRevised(_Algo):       # Models/CuttingPlaneRevised.cs:9 (Form1.cs:258)
    NAME = "Revised Cutting Plane"


class GmiCuttingPlane(_Algo):           # not in the reference: the device GMI loop (lpx_solve_cuts)
    NAME = "GMI Cutting Plane"


class SensitivityAnalysis:
    """Models/SensitivityAnalysis.cs:11-297 over an LPProblem and the SimplexResult of solving it.
    The constructor checks of :24-43 are repeated by every call (they run in the library)."""

    def __init__(self, problem: LPProblem, result: SimplexResult, **engine):
        if problem is None:
            raise SolverException(_lib.EINVAL, "Value cannot be null. (Parameter 'problem')")
        if result is None:
            raise SolverException(_lib.EINVAL, "Value cannot be null. (Parameter 'result')")
        self.problem, self.result, self.engine = problem, result, engine
        self._call(lambda a: lib().lpx_sensitivity_shadow_prices(*a, None, 0))     # :24-43

    def _args(self):
        ps, hold = _problem_struct(self.problem)
        T = self.result.Tableau
        self._hold = hold
        if T is None:
            return [C.byref(ps), None, 0, 0, None], ps
        T = np.ascontiguousarray(T, dtype=np.float64)
        basis = np.ascontiguousarray(self.result.Basis if self.result.Basis is not None else [], dtype=np.int32)
        if len(basis) != T.shape[0] - 1:        # Basis length check of :40-41 needs the true length
            raise SolverException(_lib.EINVAL, f"Basis length invalid. Expected {T.shape[0] - 1}, got {len(basis)}.")
        self._hold = (hold, T, basis)
        return [C.byref(ps), T.ctypes.data_as(_lib.dp), T.shape[0], T.shape[1], basis.ctypes.data_as(_lib.ip)], ps

    def _call(self, fn):
        a, _ps = self._args()
        rc = fn(a)
        if rc < 0:
            raise SolverException(rc, _lib.last_error())
        return rc

    def _text(self, fn):
        n = self._call(lambda a: fn(a, None, 0))
        buf = C.create_string_buffer(n + 1)
        self._call(lambda a: fn(a, buf, n + 1))
        return buf.value.decode()

    def GetRangeReport(self, target: str) -> str:                       # :47-76
        t = target.encode()
        return self._text(lambda a, b, n: lib().lpx_sensitivity_range_report(*a, t, b, n))

    def GetRange(self, target: str):
        """The (min, max) GetRangeReport prints."""
        mn, mx = C.c_double(), C.c_double()
        self._call(lambda a: lib().lpx_sensitivity_range(*a, target.encode(), C.byref(mn), C.byref(mx)))
        return mn.value, mx.value

    def ApplyChange(self, target: str, value: float) -> str:            # :78-107 (mutates self.problem)
        t = target.encode()
        f, ix = C.c_int(-1), C.c_int(-1)
        msg = self._text(lambda a, b, n: lib().lpx_sensitivity_apply_change(*a, t, float(value), C.byref(f), C.byref(ix), b, n))
        if f.value == 0:
            self.problem.Constraints[ix.value].B = float(value)
        elif f.value == 1:
            c = list(self.problem.C)
            c[ix.value] = float(value)
            self.problem.C = c
        return msg

    def GetShadowPricesReport(self) -> str:                             # :109-128
        return self._text(lambda a, b, n: lib().lpx_sensitivity_shadow_prices(*a, b, n))

    def SolveUsingDuality(self) -> SimplexResult:                       # :130-219
        o, keep = _solve_opts(self.engine)
        r = _lib.Result()
        self._call(lambda a: lib().lpx_sensitivity_solve_duality(*a, C.byref(o), C.byref(r)))
        return _take_result(r, len(self.problem.Constraints))


def ParseFromText(text: str) -> LPProblem:
    """LPParser.ParseFromText (Models/LPParser.cs:9-79). Ragged rows are kept ragged."""
    L = lib()
    p = _lib.Parsed()
    rc = L.lpx_parse_text(text.encode(), C.byref(p))
    if rc != 0:
        raise SolverException(rc, _lib.last_error())
    try:
        c = _arr(p.c, p.n, np.float64)
        A = _arr(p.A, p.m * p.n, np.float64).reshape(p.m, p.n)
        rel = _arr(p.rel, p.m, np.int32)
        b = _arr(p.b, p.m, np.float64)
        prob = LPProblem.from_arrays(p.sense, c, A, rel, b)
        prob.ragged = bool(p.ragged)
    finally:
        L.lpx_parsed_free(C.byref(p))
    return prob


def format_number(v: float) -> str:
    buf = C.create_string_buffer(64)
    lib().lpx_format_number(float(v), buf, 64)
    return buf.value.decode()


class DeviceKnapsack:
    """Batched ComputeRelaxation (Models/BranchAndBoundKnapsack.cs:431-491) on the GPU."""

    def __init__(self, profit, weight, cap: float):
        self.profit = np.ascontiguousarray(profit, dtype=np.float64)
        self.weight = np.ascontiguousarray(weight, dtype=np.float64)
        self.n = len(self.profit)
        self._h = C.c_void_p()
        _lib.check(lib().lpx_knapsack_create(self.profit.ctypes.data_as(_lib.dp), self.weight.ctypes.data_as(_lib.dp),
                                             self.n, float(cap), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().lpx_knapsack_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def order(self) -> np.ndarray:
        o = np.zeros(self.n, np.int32)
        _lib.check(lib().lpx_knapsack_order(self._h, o.ctypes.data_as(_lib.ip)))
        return o

    def relax_batch2(self, nodes):
        """lpx_knapsack_relax_batch2: like relax_batch, and for every node also its two children (the node with its
        fractional item fixed to 0 / 1).  Returns arrays of shape (len(nodes), 3): column 0 the node, 1 and 2 the
        children; frac == -2 marks children that do not exist (no fractional item)."""
        off = [0]
        fidx, fval = [], []
        for nd in nodes:
            for i in sorted(nd):
                fidx.append(i)
                fval.append(nd[i])
            off.append(len(fidx))
        off = np.asarray(off, np.int32)
        fi = np.asarray(fidx if fidx else [0], np.int32)
        fv = np.asarray(fval if fval else [0], np.int8)
        k = len(nodes)
        p = np.zeros(3 * k); w = np.zeros(3 * k); fr = np.zeros(3 * k, np.int32); fx = np.zeros(3 * k)
        _lib.check(lib().lpx_knapsack_relax_batch2(self._h, k, off.ctypes.data_as(_lib.ip), fi.ctypes.data_as(_lib.ip),
                                                   fv.ctypes.data_as(C.POINTER(C.c_int8)), p.ctypes.data_as(_lib.dp),
                                                   w.ctypes.data_as(_lib.dp), fr.ctypes.data_as(_lib.ip),
                                                   fx.ctypes.data_as(_lib.dp)))
        return p.reshape(k, 3), w.reshape(k, 3), fr.reshape(k, 3), fx.reshape(k, 3)

    def expand_batch(self, parents, items, vals):
        """lpx_knapsack_expand_batch: node j = stored node parents[j] (-1 = root) + items[j] fixed to vals[j]; its list stays
        on the device.  Returns (ids, profit, weight, frac, fracval) with the last four of shape (len, 3) as relax_batch2;
        ids[j] + 1 / + 2 are the stored children of node j (fractional item fixed to 0 / 1)."""
        k = len(parents)
        par = np.asarray(parents, np.int64); it = np.asarray(items, np.int32); vv = np.asarray(vals, np.int8)
        ids = np.zeros(k, np.int64)
        p = np.zeros(3 * k); w = np.zeros(3 * k); fr = np.zeros(3 * k, np.int32); fx = np.zeros(3 * k)
        _lib.check(lib().lpx_knapsack_expand_batch(self._h, k, par.ctypes.data_as(C.POINTER(C.c_int64)), it.ctypes.data_as(_lib.ip),
                                                   vv.ctypes.data_as(C.POINTER(C.c_int8)), ids.ctypes.data_as(C.POINTER(C.c_int64)),
                                                   p.ctypes.data_as(_lib.dp), w.ctypes.data_as(_lib.dp), fr.ctypes.data_as(_lib.ip),
                                                   fx.ctypes.data_as(_lib.dp)))
        return ids, p.reshape(k, 3), w.reshape(k, 3), fr.reshape(k, 3), fx.reshape(k, 3)

    def node_list(self, node: int) -> dict:
        """The stored fixed list of a node as {item: 0/1}."""
        d = C.c_int()
        _lib.check(lib().lpx_knapsack_node_list(self._h, int(node), None, None, 0, C.byref(d)))
        idx = np.zeros(max(d.value, 1), np.int32); val = np.zeros(max(d.value, 1), np.int8)
        _lib.check(lib().lpx_knapsack_node_list(self._h, int(node), idx.ctypes.data_as(_lib.ip), val.ctypes.data_as(C.POINTER(C.c_int8)),
                                                d.value, C.byref(d)))
        assert list(idx[: d.value]) == sorted(idx[: d.value])
        return {int(i): int(v) for i, v in zip(idx[: d.value], val[: d.value])}

    def relax_batch(self, nodes):
        """nodes: list of dict {item_index: 0/1}. Returns (profit, weight, frac_sorted_idx, frac_value)."""
        off = [0]
        fidx, fval = [], []
        for nd in nodes:
            for i in sorted(nd):
                fidx.append(i)
                fval.append(nd[i])
            off.append(len(fidx))
        off = np.asarray(off, np.int32)
        fi = np.asarray(fidx if fidx else [0], np.int32)
        fv = np.asarray(fval if fval else [0], np.int8)
        k = len(nodes)
        p = np.zeros(k); w = np.zeros(k); fr = np.zeros(k, np.int32); fx = np.zeros(k)
        _lib.check(lib().lpx_knapsack_relax_batch(self._h, k, off.ctypes.data_as(_lib.ip), fi.ctypes.data_as(_lib.ip),
                                                  fv.ctypes.data_as(C.POINTER(C.c_int8)), p.ctypes.data_as(_lib.dp),
                                                  w.ctypes.data_as(_lib.dp), fr.ctypes.data_as(_lib.ip),
                                                  fx.ctypes.data_as(_lib.dp)))
        return p, w, fr, fx
