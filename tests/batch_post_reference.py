"""The post-solve of the FAST batch (csrc/k_batch_post.hip, k_batch_fast_post), written down
again in plain numpy float64 on tests/batch_fast_from_reference.py's inverse and price and
tests/batch_fast_reference.py's ftran, in the orders the kernel documents:

    W = invert(B)                                   as a launch of the FAST batch builds it
    OPTIMAL     y_r = sum_p W[p][r] c[B_p]          four interleaved partial sums, p ascending
                d[N_k] = -dz_k - c[N_k]             dz = price(y);  d[B_p] = 0.0
                dual_obj = constant + rhs0 . y      the same four sums over the rows
    ranging     rhs direction h:   delta_p = sum_e W[p][r_e] h_e          entries in the order given
                cost direction g:  Y_r = sum_e g_e W[pos(e)][r] over its basic entries, in entry order
                                   delta_k = -dz_k(Y) - g[N_k];  no basic entry: delta_k = 0.0 - g[N_k]
                candidates: ranging_reference.ratio_rule
    UNBOUNDED   pos over (z, zbar), dx = ftran(W, a_j), d[j] = 1, d[B_p] = -dx_p,
                value = c[j] - dot4(c_B, dx), violation = max(dx, 0)
    INFEASIBLE  pos over (x, xbar), y = row pos of W, dz = price(y), d[N_k] = -dz_k, d[B_pos] = 1,
                value = dot4(rhs0, y), violation = max(dz, 0)

It is the CPU statement of what the kernel computes (tests/test_batch_post_host.py holds it to long
double with the project's rule) and not a bit-for-bit target, as in DESIGN 7g.

The planted cases enter the GPU through start=(basis, nonbasis) on the slack-basis form, so the state
the post-solve reads is the restart's x = W b, not the planted x.  Only g = 0 plants are used: a
recomputed x turns a planted exact 0.0 into +-1e-16, the restart state would not be optimal and the
solve would pivot.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from tests import batch_fast_from_reference as bffr
from tests import batch_fast_reference as fr
from tests import planted as pl
from tests import ranging_reference as rgref
from tests import state_check as sc

# (m, n_struct, k): bucket 0 full; PL = 32 and q below a wave; k = m; 33 rows; ld = 65; the smallest of
# bucket 3; the LDS cap twice
SHAPES = [(2, 3, 1), (16, 24, 7), (17, 12, 6), (32, 40, 32), (33, 15, 9), (64, 64, 20), (65, 8, 5),
          (128, 192, 50), (128, 130, 128)]
RAY_SHAPES = [(16, 24, 7), (33, 15, 9), (64, 64, 20), (128, 192, 50)]
EPS = 1e-9  # the solver's default epsilon


def dot4(a, b) -> float:
    """sum_j a[j] b[j] in ftran's order."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    prod = np.zeros((len(a) + 3) // 4 * 4)
    prod[:len(a)] = a * b
    s = np.zeros(4)
    for j in range(0, len(prod), 4):
        s = s + prod[j:j + 4]
    return float((s[0] + s[1]) + (s[2] + s[3]))


def _codes(a, basis, nonbasis):
    m, ns = a.shape
    codes = sc.var_codes(m + ns, ns)
    return codes[np.asarray(basis)], codes[np.asarray(nonbasis)]


def duals(a, rhs0, cc, constant, basis, nonbasis, x, z, w=None):
    """y, d (by variable) and the certificate's scalars, or None where the basis does not invert."""
    a = np.asarray(a, dtype=np.float64)
    cb, cn = _codes(a, basis, nonbasis)
    w = bffr.inverse(a, cb) if w is None else w
    if w is None:
        return None
    cc = np.asarray(cc, dtype=np.float64)
    y = fr.ftran(np.ascontiguousarray(w.T), cc[basis])
    d_n = -bffr.price(a, cn, y) - cc[nonbasis]
    d = np.zeros(len(cc))
    d[nonbasis] = d_n
    z = np.asarray(z, dtype=np.float64)
    return SimpleNamespace(
        y=y, d=d, w=w, dual_obj=constant + dot4(rhs0, y),
        primal_infeas=max(0.0, -float(np.min(x))) if len(x) else 0.0,
        dual_infeas=max(0.0, -float(np.min(d_n))) if len(d_n) else 0.0,
        z_diff=(float(np.max(np.abs(z - d_n))) / max(1.0, float(np.max(np.abs(d_n))))) if len(d_n) else 0.0)


def ranges(a, basis, nonbasis, x, d, w, cost_dirs, rhs_dirs, tol=rgref.DEFAULT_TOL):
    """(cost RefRanges, rhs RefRanges) from the inverse w, the carried x and the fresh d (by variable)."""
    a = np.asarray(a, dtype=np.float64)
    m = a.shape[0]
    basis, nonbasis = np.asarray(basis), np.asarray(nonbasis)
    _, cn = _codes(a, basis, nonbasis)
    where = np.full(len(basis) + len(nonbasis), -1, dtype=np.int64)
    where[basis] = np.arange(m)
    xc, dc = np.maximum(np.asarray(x, dtype=np.float64), 0.0), np.maximum(d[nonbasis], 0.0)
    cost, rhs = [], []
    for g in cost_dirs:
        gfull = np.zeros(len(where))
        yy, nbasic = np.zeros(m), 0
        for j, v in g.items():
            gfull[int(j)] = v
            if where[int(j)] >= 0:
                yy = yy + float(v) * w[where[int(j)]]
                nbasic += 1
        delta = (-bffr.price(a, cn, yy) if nbasic else np.zeros(len(nonbasis))) - gfull[nonbasis]
        cost.append(rgref.ratio_rule(dc, delta, nonbasis, tol))
    for h in rhs_dirs:
        delta = np.zeros(m)
        for r, v in h.items():
            delta = delta + w[:, int(r)] * float(v)
        rhs.append(rgref.ratio_rule(xc, delta, basis, tol))
    return cost, rhs


def first_pivot(y, ybar):
    """find_first_pivot (src/simplex.rs:423-437) on clean data: argmax of -y / ybar over ybar > 0, the
    lowest position on ties; (position, ratio), position -1: none."""
    y, ybar = np.asarray(y, dtype=np.float64), np.asarray(ybar, dtype=np.float64)
    cand = np.flatnonzero(ybar > 0.0)
    if not len(cand):
        return -1, 0.0
    r = -y[cand] / ybar[cand]
    k = int(np.argmax(r))
    return int(cand[k]), float(r[k])


def status_of(x, xbar, z, zbar, eps=EPS):
    """status() before the first pivot (src/simplex.rs:274-306): "optimal", or the step kind and the
    first-pivot position of the side that steps."""
    pj, mu_d = first_pivot(z, zbar)
    pi, mu_p = first_pivot(x, xbar)
    if pj >= 0 and pi >= 0:
        if mu_p <= eps and mu_d <= eps:
            return "optimal", -1
        return ("primal", pj) if mu_p < mu_d else ("dual", pi)
    if pj >= 0:
        return "primal", pj
    return ("dual", pi) if pi >= 0 else ("panic", -1)


def ray(a, rhs0, cc, basis, nonbasis, x, xbar, z, zbar, primal: bool, w=None):
    """The ray of the state, or None where the basis does not invert or no first pivot exists."""
    a = np.asarray(a, dtype=np.float64)
    m, ns = a.shape
    basis, nonbasis = np.asarray(basis), np.asarray(nonbasis)
    cb, cn = _codes(a, basis, nonbasis)
    w = bffr.inverse(a, cb) if w is None else w
    pos, mu = first_pivot(z, zbar) if primal else first_pivot(x, xbar)
    if w is None or pos < 0:
        return None
    cc = np.asarray(cc, dtype=np.float64)
    d, y = np.zeros(len(cc)), np.zeros(m)
    if primal:
        j = int(nonbasis[pos])
        dx = fr.ftran(w, fr.entering_column(a, ns, j)) if j < ns else w[:, j - ns].copy()
        d[basis] = -dx
        d[j] = 1.0
        value = float(cc[j]) - dot4(cc[basis], dx)
        vec, var = dx, j
    else:
        y = w[pos].copy()
        dz = bffr.price(a, cn, y)
        d[nonbasis] = -dz
        d[basis[pos]] = 1.0
        value = dot4(rhs0, y)
        vec, var = dz, int(basis[pos])
    violation = float("nan") if np.isnan(vec).any() else max(0.0, float(np.max(vec))) if len(vec) else 0.0
    proven = violation == 0.0 and (value > 0.0 if primal else value < 0.0)
    return SimpleNamespace(pos=pos, var=var, mu=mu, d=d, y=y, value=value, violation=violation, proven=proven)


# ---------------------------------------------------------------- the cases both test files use
def optimal_plant(shape) -> pl.Planted:
    m, ns, k = shape
    return pl.planted_optimal(7 + 1000 * m + 10 * k, m, ns, k)


def ray_plant(kind, shape) -> pl.Planted:
    """The seeds are planted.ray_case's: tests/test_batch_post_host.py checks for every case that
    batch_fast_from_reference.restart from the planted basis stops at the planted position before its
    first pivot."""
    return pl.ray_case(kind, *shape)


def restart_of(p: pl.Planted):
    """The FAST restart state of the planted basis on the slack-basis form of the plant's data."""
    return bffr.restart(p.a, None, p.b, p.cc, p.basis, p.nonbasis)
