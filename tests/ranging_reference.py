"""The specification of sensitivity ranging, written over the CPU oracle's primitives (DESIGN.md
section 7e).  Core sense: maximise c.x + constant, [A | I] x = rhs, x >= 0.  At an OPTIMAL basis B
with nonbasic set N, with the carried x by position and the FRESH reduced costs d of
tests/duals_reference.py by variable, both clamped at zero (xc = max(x, 0.0), dc = max(d, 0.0)):

    cost direction g:   Y = B^-T g_B                       LU::solve of B^T Y = g_B
                        delta_k = -neg_t_dot(N, Y)_k - g[N_k]     (d's formula with g for c)
    rhs direction h:    delta_p = (B^-1 h)_p               LU::solve of B delta = h
    candidate:          |delta| > pivot_tol,  r = -(clamped / delta)   one division, one negation
                        delta > 0: r bounds lo (the largest wins), delta < 0: r bounds hi (the
                        smallest wins); the first position wins a tie
    lo / hi:            -inf / +inf without candidate; *_var the variable at the winning position
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import oracle as ora
from tests import duals_reference as dref

DEFAULT_TOL = 1e-9


@dataclass
class RefRange:
    lo: float
    hi: float
    lo_var: int
    hi_var: int


def ratio_rule(clamped, delta, variables, tol: float) -> RefRange:
    """The candidate rule over positions 0, 1, ... in the arrays' own arithmetic (float64 for the
    reference, long double for the tests' yardsticks); the first position wins a tie (argmax and
    argmin return the first extremum)."""
    clamped, delta = np.asarray(clamped), np.asarray(delta)
    lo, hi, lo_var, hi_var = -np.inf, np.inf, -1, -1
    cand = np.abs(delta) > tol
    if cand.any():
        with np.errstate(divide="ignore", invalid="ignore"):
            r = -(clamped / delta)
        up = np.flatnonzero(cand & (delta > 0))
        if len(up):
            k = up[np.argmax(r[up])]
            lo, lo_var = float(r[k]), int(variables[k])
        down = np.flatnonzero(cand & ~(delta > 0))
        if len(down):
            k = down[np.argmin(r[down])]
            hi, hi_var = float(r[k]), int(variables[k])
    return RefRange(lo, hi, lo_var, hi_var)


class CoreRanging:
    """Ranging at the final basis of `res` (anything with basis, nonbasis, x) for the standard form
    `sf`: the basis is factorised once (Matrix::factorize), every direction is one LU::solve."""

    def __init__(self, sf: "ora.StdForm", res, duals: "dref.RefDuals | None" = None):
        self.sf, self.m, self.n = sf, sf.m, sf.n
        self.basis = np.asarray(res.basis, dtype=np.int64)
        self.nonbasis = np.asarray(res.nonbasis, dtype=np.int64)
        duals = dref.core_duals(sf, res) if duals is None else duals
        self.xc = np.maximum(np.asarray(res.x, dtype=np.float64), 0.0)
        self.dc = np.maximum(duals.d[self.nonbasis], 0.0)
        bmat = np.empty((self.m, self.m))
        for p, j in enumerate(self.basis):
            bmat[:, p] = ora.csc_column(self.m, sf.col_ptr, sf.row_idx, sf.val, int(j))
        self._lu = ora.lu_factorize(bmat) if self.m else None
        self._lut = ora.lu_factorize(np.ascontiguousarray(bmat.T)) if self.m else None

    def _solve(self, lu, rhs):
        return ora.lu_solve_factored(lu[0], lu[1], rhs) if self.m else np.zeros(0)

    def cost(self, direction: dict, tol: float = DEFAULT_TOL) -> RefRange:
        g = np.zeros(self.n)
        for j, v in direction.items():
            g[int(j)] = float(v)
        y = self._solve(self._lut, g[self.basis])
        delta = -ora.neg_t_dot(self.sf.col_ptr, self.sf.row_idx, self.sf.val, self.nonbasis, y) - g[self.nonbasis]
        return ratio_rule(self.dc, delta, self.nonbasis, tol)

    def rhs(self, direction: dict, tol: float = DEFAULT_TOL) -> RefRange:
        h = np.zeros(self.m)
        for i, v in direction.items():
            h[int(i)] = float(v)
        return ratio_rule(self.xc, self._solve(self._lu, h), self.basis, tol)


def refined_inverse(bmat, steps: int = 2):
    """B^-1 in long double: a double LU solve of the identity refined with residuals formed in long
    double, the way tests/duals_helpers.long_double_y refines one vector."""
    import scipy.linalg as sla

    ld = np.longdouble
    m = bmat.shape[0]
    if m == 0:
        return np.zeros((0, 0), dtype=ld)
    lu = sla.lu_factor(bmat)
    b_ld, eye = bmat.astype(ld), np.eye(m, dtype=ld)
    inv = sla.lu_solve(lu, np.eye(m)).astype(ld)
    for _ in range(steps):
        inv = inv + sla.lu_solve(lu, (eye - b_ld @ inv).astype(np.float64)).astype(ld)
    return inv


def ranges_from_inverse(inv, nmat, unit_rows, basis, nonbasis, x, d_n, cost_dirs, rhs_dirs,
                        tol: float = DEFAULT_TOL):
    """The rule in the arithmetic of `inv` (B^-1: long double, or numpy's double): (cost ranges, rhs
    ranges, and per direction of either kind whether some |delta| lies in [tol / 2, 2 tol], where
    rounding decides whether the position is a candidate).  nmat: the nonbasic columns, dense; unit_rows[k] = r where nonbasic column
    k is the slack e_r (its column of B^-1 N is a column of B^-1), -1 otherwise."""
    ft = inv.dtype
    m, n = inv.shape[0], len(basis) + len(nonbasis)
    unit_rows = np.asarray(unit_rows, dtype=np.int64)
    xc = np.maximum(np.asarray(x, dtype=ft), 0)
    dc = np.maximum(np.asarray(d_n, dtype=ft), 0)
    t = np.zeros((m, len(nonbasis)), dtype=ft)  # B^-1 N
    dense = np.flatnonzero(unit_rows < 0)
    t[:, dense] = inv @ nmat[:, dense].astype(ft)
    slack = np.flatnonzero(unit_rows >= 0)
    t[:, slack] = inv[:, unit_rows[slack]]
    where = np.full(n, -1, dtype=np.int64)
    where[np.asarray(basis)] = np.arange(m)

    def near(delta):
        size = np.abs(delta)
        return bool(np.any((size >= tol / 2) & (size <= 2 * tol)))

    cost, rhs, margin_c, margin_r = [], [], [], []
    for direction in cost_dirs:
        g = np.zeros(n, dtype=ft)
        delta = np.zeros(len(nonbasis), dtype=ft)
        for j, v in direction.items():
            g[int(j)] = v
            if where[int(j)] >= 0:
                delta = delta + ft.type(v) * t[where[int(j)]]
        delta = delta - g[np.asarray(nonbasis)]
        cost.append(ratio_rule(dc, delta, nonbasis, tol))
        margin_c.append(near(delta))
    for direction in rhs_dirs:
        delta = np.zeros(m, dtype=ft)
        for i, v in direction.items():
            delta = delta + ft.type(v) * inv[:, int(i)]
        rhs.append(ratio_rule(xc, delta, basis, tol))
        margin_r.append(near(delta))
    return cost, rhs, margin_c, margin_r


def long_double_ranges(bmat, nmat, basis, nonbasis, x, d_n, cost_dirs, rhs_dirs, tol: float = DEFAULT_TOL):
    """(cost, rhs) lists of RefRange from the long-double inverse of the basis.  bmat = columns of
    the basis, nmat = columns of the nonbasic variables (dense)."""
    cost, rhs, _, _ = ranges_from_inverse(refined_inverse(bmat), nmat, np.full(len(nonbasis), -1), basis,
                                          nonbasis, x, d_n, cost_dirs, rhs_dirs, tol)
    return cost, rhs
