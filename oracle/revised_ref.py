"""Basis-only reference of the revised primal iteration (TEST INFRASTRUCTURE; pure numpy, no GPU, no C).

`oracle.revised_solve` restates the reference loop faithfully and re-inverts the m x m basis every iteration, so it
costs O(m^3) per pivot and stops being usable near m = 1000.  This module follows the same decision rules
(`oracle/revised.c`) but exploits the start basis: every run starts from the all-slack basis B = I, so after k pivots
B is the identity with at most k structural columns in it.  With

    T    = basis positions that hold structural columns (|T| = k),
    R_S  = rows covered by the slack columns still in the basis,
    R_T  = the other rows (|R_T| = k),
    M    = A[R_T, Bidx[T]]                      (k x k),

every solve with B reduces to one k x k system:

    B x = y       x_T = M^-1 y[R_T],   x_p = y_i - A[i, Bidx[T]] x_T   for the slack position p covering row i
    pi^T B = c_B  pi[R_S] = 0,         pi[R_T] = M^-T c_B[T]

M^-1 is formed in np.longdouble by a small Gauss-Jordan elimination with partial pivoting (numpy's linalg does not
take longdouble), so a step costs O((m + n) k + k^3).  The reduced costs, d and x_B are rounded to float64 before the
rules are applied in float64, as on the GPU: a value computed in longdouble can fall on the other side of the 1e-12
hysteresis band from the same value computed in double.

Rules (oracle/revised.c, Models/RevisedPrimalSimplex.cs:76-124):
  entering  the first strict minimum of rN below -eps, in Nidx list order;
  leaving   rows with d_i > eps in ascending order, a row is taken when theta < best - 1e-12;
  lists     Bidx[r] = q; Nidx.RemoveAt(pos); Nidx.Add(leaving).

Per step the reference keeps the rN and d it decided on, the decision margins, the exact reduced-cost ties that list
order (the kernels' order keys) decided, the ratio-test near-ties, and slack re-entries.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

LD = np.longdouble
OPTIMAL, UNBOUNDED, ITER_LIMIT = 0, 1, 3
EPS, RATIO_TOL = 1e-9, 1e-12


def _gj_inverse(M: np.ndarray) -> np.ndarray:
    """Inverse of a small longdouble matrix: Gauss-Jordan on [M | I], partial pivoting (first maximum of |a|)."""
    k = M.shape[0]
    W = np.concatenate([M.astype(LD), np.eye(k, dtype=LD)], axis=1)
    for col in range(k):
        p = col + int(np.argmax(np.abs(W[col:, col])))
        if W[p, col] == 0:
            raise np.linalg.LinAlgError("revised_ref: singular basis")
        if p != col:
            W[[col, p]] = W[[p, col]]
        W[col] /= W[col, col]
        f = W[:, col].copy()
        f[col] = 0
        W -= np.outer(f, W[col])
    return W[:, k:]


@dataclass
class Step:
    """One iteration: the values the rules saw (float64) and how close each decision was."""
    it: int                      # 0-based iteration number
    rc: np.ndarray               # reduced cost of every column [n + m] at the start of the step (+inf for basic ones)
    q: int                       # entering column (-1: optimal)
    d: Optional[np.ndarray]      # B^-1 a_q (None when optimal)
    r: int                       # leaving row (-1: optimal or unbounded)
    enter_gap: float             # (runner-up rN - min rN) / max(1, |min|) over candidates of another value; inf if none
    eps_gap: float               # min over nonbasic j of |rN_j + eps| / max(1, |rN_j|)
    ratio_gap: float             # min over eligible rows of |theta_i - (best_i - 1e-12)| / max(1, |best_i|); inf if none
    den_gap: float               # min over rows of |d_i - eps| / max(1, |d_i|)
    tie_cols: List[int] = field(default_factory=list)     # columns sharing the minimum exactly (>= 2 when a tie was decided)
    ratio_band: List[int] = field(default_factory=list)   # rows within 1e-12 of the best ratio in effect when they were scanned


class RevisedRef:
    """State of the revised iteration from the all-slack basis of  min c x, A x <= b, x >= 0  (b >= 0)."""

    def __init__(self, A: np.ndarray, c: np.ndarray, b: np.ndarray, eps: float = EPS, tol: float = RATIO_TOL):
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.c = np.ascontiguousarray(c, dtype=np.float64)
        self.b = np.ascontiguousarray(b, dtype=np.float64)
        self.m, self.n = self.A.shape
        self.eps, self.tol = eps, tol
        self.Bidx = list(range(self.n, self.n + self.m))
        self.Nidx = list(range(self.n))
        self.trace: List[List[int]] = []
        self.steps: List[Step] = []
        self.status = ITER_LIMIT
        self._factor()

    # ---- linear algebra of the current basis ------------------------------------------------------------------
    def _factor(self):
        m, n = self.m, self.n
        Bidx = np.asarray(self.Bidx)
        self.tpos = np.nonzero(Bidx < n)[0]                  # positions holding structural columns
        self.tcol = Bidx[self.tpos]
        spos = np.nonzero(Bidx >= n)[0]
        self.spos, self.srow = spos, Bidx[spos] - n           # slack position p covers row srow
        covered = np.zeros(m, bool)
        covered[self.srow] = True
        self.RT = np.nonzero(~covered)[0]
        assert len(self.RT) == len(self.tpos)
        k = len(self.tpos)
        self.Minv = _gj_inverse(self.A[np.ix_(self.RT, self.tcol)]) if k else np.zeros((0, 0), LD)
        self.AcolT = self.A[:, self.tcol].astype(LD)          # m x k
        x = self._solve(self.b.astype(LD))
        self.xB_ld = x
        cB = np.zeros(m, LD)
        cB[self.tpos] = self.c[self.tcol]
        self.z_ld = (cB * x).sum()
        pi = np.zeros(m, LD)
        if k:
            pi[self.RT] = self.Minv.T @ self.c[self.tcol].astype(LD)
        self.pi_ld = pi

    def _solve(self, y: np.ndarray) -> np.ndarray:
        """x = B^-1 y in longdouble (y longdouble, length m); x is indexed by basis position."""
        x = np.zeros(self.m, LD)
        xT = self.Minv @ y[self.RT] if len(self.RT) else np.zeros(0, LD)
        x[self.tpos] = xT
        x[self.spos] = y[self.srow] - (self.AcolT[self.srow] @ xT if len(xT) else 0)
        return x

    def _column(self, q: int) -> np.ndarray:
        if q < self.n:
            return self.A[:, q].astype(LD)
        e = np.zeros(self.m, LD)
        e[q - self.n] = 1
        return e

    def reduced_costs(self) -> np.ndarray:
        """rc[n + m] in float64: c_j - pi . a_j for nonbasic columns, +inf for basic ones."""
        n, m = self.n, self.m
        rc = np.empty(n + m, LD)
        rc[:n] = self.c.astype(LD)
        if len(self.RT):
            rc[:n] -= self.A[self.RT].astype(LD).T @ self.pi_ld[self.RT]
        rc[n:] = -self.pi_ld
        out = rc.astype(np.float64)
        out[np.asarray(self.Bidx)] = np.inf
        return out

    # ---- the iteration ---------------------------------------------------------------------------------------
    def run(self, max_iter: int) -> int:
        """Continues until `max_iter` iterations have been done in all (cumulative) or the run ends."""
        while self.status == ITER_LIMIT and len(self.trace) < max_iter:
            self._step()
        return self.status

    def _step(self):
        eps, tol = self.eps, self.tol
        rc = self.reduced_costs()
        rN = rc[np.asarray(self.Nidx)]
        eps_gap = float(np.min(np.abs(rN + eps) / np.maximum(1.0, np.abs(rN)))) if len(rN) else np.inf
        cand = rN < -eps
        it = len(self.trace)
        if not cand.any():
            self.steps.append(Step(it, rc, -1, None, -1, np.inf, eps_gap, np.inf, np.inf))
            self.status = OPTIMAL
            return
        pos = int(np.argmin(np.where(cand, rN, np.inf)))     # first occurrence = first in list order
        best = rN[pos]
        ties = np.nonzero(cand & (rN == best))[0]
        others = rN[cand & (rN != best)]
        enter_gap = float((others.min() - best) / max(1.0, abs(best))) if len(others) else np.inf
        q = self.Nidx[pos]
        d = self._solve(self._column(q)).astype(np.float64)
        xB = self.xB_ld.astype(np.float64)
        den_gap = float(np.min(np.abs(d - eps) / np.maximum(1.0, np.abs(d))))
        r, ratio_gap, band = self._ratio(d, xB)
        st = Step(it, rc, q, d, r, enter_gap, eps_gap, ratio_gap, den_gap,
                  [self.Nidx[i] for i in ties] if len(ties) > 1 else [], band)
        self.steps.append(st)
        if r < 0:
            self.status = UNBOUNDED
            return
        leaving = self.Bidx[r]
        self.Bidx[r] = q
        del self.Nidx[pos]
        self.Nidx.append(leaving)
        self.trace.append([r, q])
        self._factor()

    def _ratio(self, d: np.ndarray, xB: np.ndarray):
        """The hysteresis chain of :99-112 in float64; returns (row, margin, near-tied rows)."""
        tol = self.tol
        elig = np.nonzero(d > self.eps)[0]
        if not len(elig):
            return -1, np.inf, []
        theta = xB[elig] / d[elig]
        best_before = np.empty(len(theta))                   # best in effect when row elig[i] was scanned
        best, win, i = np.inf, -1, 0
        while i < len(theta):
            hit = np.nonzero(theta[i:] < best - tol)[0]
            j = i + int(hit[0]) if len(hit) else len(theta)
            best_before[i:j + 1] = best
            if j == len(theta):
                break
            best, win, i = theta[j], j, j + 1
        fin = np.isfinite(best_before)
        gaps = np.abs(theta[fin] - (best_before[fin] - tol)) / np.maximum(1.0, np.abs(best_before[fin]))
        ratio_gap = float(gaps.min()) if len(gaps) else np.inf
        band = elig[fin][np.abs(theta[fin] - best_before[fin]) <= tol].tolist()
        return int(elig[win]), ratio_gap, band

    # ---- what the engine exposes -----------------------------------------------------------------------------
    @property
    def xB(self) -> np.ndarray:
        return self.xB_ld.astype(np.float64)

    @property
    def z(self) -> float:
        return float(self.z_ld)

    @property
    def pi(self) -> np.ndarray:
        return self.pi_ld.astype(np.float64)

    def binv_rows(self, r0: int, r1: int) -> np.ndarray:
        """Rows r0 .. r1-1 of B^-1 in float64 (the identity plus the k-row structure; never the whole m x m at once)."""
        m = self.m
        out = np.zeros((r1 - r0, m), LD)
        tpos_of = {int(p): a for a, p in enumerate(self.tpos)}
        srow_of = {int(p): int(i) for p, i in zip(self.spos, self.srow)}
        for p in range(r0, r1):
            if p in tpos_of:
                out[p - r0, self.RT] = self.Minv[tpos_of[p]]
            else:
                i = srow_of[p]
                out[p - r0, i] = 1
                if len(self.RT):
                    out[p - r0, self.RT] = -(self.AcolT[i] @ self.Minv)
        return out.astype(np.float64)

    def binv(self) -> np.ndarray:
        return self.binv_rows(0, self.m)

    # ---- records ---------------------------------------------------------------------------------------------
    def key_order_ties(self) -> List[dict]:
        """Exact reduced-cost ties among entering candidates: which column won (first in list order) and whether its
        column index is larger than a tied loser's (key order and column order disagree)."""
        out = []
        for s in self.steps:
            if len(s.tie_cols) > 1:
                out.append({"it": s.it, "winner": s.q, "cols": list(s.tie_cols), "winner_larger": s.q > min(s.tie_cols)})
        return out

    def slack_reentries(self) -> List[dict]:
        """Slack columns that entered the basis again (every slack starts basic); `slack` is the row index."""
        return [{"it": s.it, "slack": s.q - self.n} for s in self.steps if s.q >= self.n]

    def min_margin(self, skip_exact_ties: bool = False) -> float:
        """Smallest decision margin over all steps (entering gap, ratio chain); skip_exact_ties ignores steps whose entering
        choice was an exact tie by construction."""
        v = np.inf
        for s in self.steps:
            if not (skip_exact_ties and len(s.tie_cols) > 1):
                v = min(v, s.enter_gap)
            v = min(v, s.ratio_gap)
        return v

    def min_threshold_margin(self) -> float:
        """Smallest distance of any rN or d entry to the eps threshold (relative to max(1, |value|))."""
        v = np.inf
        for s in self.steps:
            v = min(v, s.eps_gap, s.den_gap)
        return v
