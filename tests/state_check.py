"""A reference check of the state FAST numerics carries (x, xbar, z, zbar) against the state its basis
defines, in long double -- the sibling of tests/inverse_check.py, which checks the inverse itself.

The starting state (basis0, nonbasis0, x0, xbar0, z0, zbar0) is taken as the definition, so slack
starts, warm starts (core.warm_started: x = 1, z = -1) and resumed solves are all covered:

    r = B0 x0          rbar = B0 xbar0
    c' = 0 on the starting basics, -z0 on the starting nonbasics      (cbar' likewise with -zbar0)
    x^ = B^-1 r        xbar^ = B^-1 rbar
    z^_N = N^T (B^-T c'_B) - c'_N                                     (zbar^_N likewise from cbar')

On a slack start c' = c and r = b: what csrc/k_drift.hip recomputes at a refactorisation.  The
solves run in double (LAPACK LU) and are refined with residuals formed in long double; the last
correction is the helper's error estimate.  The metric is k_drift's own, per vector,
||v - v^||_inf / max(1, ||v^||_inf); D is its maximum over the four vectors.

B's column j is A[:, var_col[basis[j]]] for a structural variable and e_r for the slack of row r
(var_col code -1 - r), as inverse_check.basis_matrix builds it; without var_col the benchmark
convention holds (variables 0..ns-1 structural, ns + r the slack of row r).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.linalg as sla

from tests import inverse_check as ic

assert np.finfo(np.longdouble).nmant >= 63, "the state check needs an 80-bit long double"

U53 = 2.0 ** -53
LD = np.longdouble
VECTORS = ("x", "xbar", "z", "zbar")
CHUNK = ic.CHUNK

# D <= C_STATE[family] in tests/test_gpu_state.py: 10x the worst D the family showed on an MI355X
# (C_STATE_OBSERVED; pytest -s prints them).  D grows with the pivot count: config 2's whole solve
# (21 642 pivots) ends near 5e-10, above what a 1e-10 error in one entry adds, so the CPU controls
# (tests/test_state_check.py) reject such an error at every constant but config 2's (C_STATE_SHORT).
C_STATE_OBSERVED = {"config 2": 4.600e-10, "config 2 refactorised": 7.949e-10, "eta flush": 4.763e-13,
                    "csc": 4.472e-12, "warm start": 2.811e-13, "resumed": 8.609e-13}
C_STATE = {"config 2": 5e-9, "config 2 refactorised": 8e-9, "eta flush": 5e-12,
           "csc": 5e-11, "warm start": 3e-12, "resumed": 9e-12}
C_STATE_MAX = max(C_STATE.values())
C_STATE_SHORT = max(v for k, v in C_STATE.items() if not k.startswith("config 2"))


def get(state, name):
    """A field of a state: a CoreResult, a SolveResult, a CoreLP or a mapping (an .npz archive)."""
    return state[name] if hasattr(state, "keys") else getattr(state, name)


def var_codes(n: int, ns: int, var_col=None) -> np.ndarray:
    if var_col is not None:
        return np.asarray(var_col, dtype=np.int64)
    v = np.arange(n, dtype=np.int64)
    return np.where(v < ns, v, -1 - (v - ns))


def columns(a, m: int, codes) -> np.ndarray:
    """Dense m x len(codes): A's column for a code >= 0, e_r for the slack code -1 - r."""
    codes = np.asarray(codes, dtype=np.int64)
    out = np.zeros((m, len(codes)))
    s = np.flatnonzero(codes >= 0)
    if len(s):
        out[:, s] = ic._columns(a, codes[s])
    sl = np.flatnonzero(codes < 0)
    out[-1 - codes[sl], sl] = 1.0
    return out


def _times(a, m, codes, v) -> np.ndarray:
    """[columns of codes] v in long double."""
    v = np.asarray(v, dtype=LD)
    out = np.zeros(m, dtype=LD)
    for c0 in range(0, len(codes), CHUNK):
        out += columns(a, m, codes[c0:c0 + CHUNK]).astype(LD) @ v[c0:c0 + CHUNK]
    return out


def _t_times(a, m, codes, y) -> np.ndarray:
    """[columns of codes]^T y in long double, in column chunks."""
    y = np.asarray(y, dtype=LD)
    out = np.empty(len(codes), dtype=LD)
    for c0 in range(0, len(codes), CHUNK):
        out[c0:c0 + CHUNK] = columns(a, m, codes[c0:c0 + CHUNK]).T.astype(LD) @ y
    return out


def _refined(lu, bmat_ld, rhs, trans: int, steps: int):
    """Solve B v = rhs (trans=1: B^T v = rhs) in double, refine with long-double residuals; returns
    (v in long double, the last correction)."""
    v = sla.lu_solve(lu, np.asarray(rhs, dtype=np.float64), trans=trans).astype(LD)
    d = v.astype(np.float64)
    for _ in range(steps):
        res = rhs - (bmat_ld.T @ v if trans else bmat_ld @ v)
        d = sla.lu_solve(lu, res.astype(np.float64), trans=trans)
        v = v + d.astype(LD)
    return v, d


@dataclass
class Exact:
    """The state a basis defines (long double) and the helper's error estimate per vector
    (relative, in the metric's units)."""
    basis: np.ndarray
    nonbasis: np.ndarray
    x: np.ndarray
    xbar: np.ndarray
    z: np.ndarray
    zbar: np.ndarray
    err: dict

    def drift(self, state) -> dict:
        """k_drift's metric of `state`'s x, xbar, z, zbar against this one, and "D", their maximum."""
        out = {}
        for name in VECTORS:
            v, ref = np.asarray(get(state, name), dtype=LD), getattr(self, name)
            if len(ref) == 0:
                out[name] = 0.0
                continue
            out[name] = float(np.abs(v - ref).max() / max(LD(1), np.abs(ref).max()))
        out["D"] = max(out[name] for name in VECTORS)
        return out

    def rounded(self) -> dict:
        """The state rounded to double, in the layout oracle.simplex_solve resumes from."""
        return dict(basis=self.basis.copy(), nonbasis=self.nonbasis.copy(),
                    **{name: getattr(self, name).astype(np.float64) for name in VECTORS})


def exact_state(a, ns: int, start, basis, nonbasis, var_col=None, steps: int = 3) -> Exact:
    """The state (basis, nonbasis) defines, given the starting state `start` (anything with basis,
    nonbasis, x, xbar, z, zbar; xbar / zbar None: ones).  `a`: dense (m x ns) or inverse_check.Csc."""
    basis, nonbasis = np.asarray(basis, dtype=np.int64), np.asarray(nonbasis, dtype=np.int64)
    b0, nb0 = np.asarray(get(start, "basis"), dtype=np.int64), np.asarray(get(start, "nonbasis"), dtype=np.int64)
    m, q = len(basis), len(nonbasis)
    codes = var_codes(m + q, ns, var_col)
    x0 = np.asarray(get(start, "x"), dtype=np.float64)
    z0 = np.asarray(get(start, "z"), dtype=np.float64)
    xb0, zb0 = get(start, "xbar"), get(start, "zbar")
    xb0 = np.ones(m) if xb0 is None else np.asarray(xb0, dtype=np.float64)
    zb0 = np.ones(q) if zb0 is None else np.asarray(zb0, dtype=np.float64)

    r, rbar = _times(a, m, codes[b0], x0), _times(a, m, codes[b0], xb0)
    cp, cbarp = np.zeros(m + q, dtype=LD), np.zeros(m + q, dtype=LD)
    cp[nb0], cbarp[nb0] = -z0.astype(LD), -zb0.astype(LD)

    bm = columns(a, m, codes[basis])
    bm_ld = bm.astype(LD)
    lu = sla.lu_factor(bm)
    out, err = {}, {}
    for name, rhs in (("x", r), ("xbar", rbar)):
        v, last = _refined(lu, bm_ld, rhs, 0, steps)
        out[name] = v
        err[name] = float(np.abs(last).max(initial=0.0)) / max(1.0, float(np.abs(v).max(initial=0.0)))
    for name, cc in (("z", cp), ("zbar", cbarp)):
        y, last = _refined(lu, bm_ld, cc[basis], 1, steps)
        v = _t_times(a, m, codes[nonbasis], y) - cc[nonbasis]
        # the last correction of y, carried through N^T
        out[name] = v
        dz = np.abs(_t_times(a, m, codes[nonbasis], last).astype(np.float64)).max(initial=0.0)
        err[name] = float(dz) / max(1.0, float(np.abs(v).max(initial=0.0)))
    return Exact(basis.copy(), nonbasis.copy(), out["x"], out["xbar"], out["z"], out["zbar"], err)


def stdform(a, ns: int, c, state, var_col=None):
    """An oracle StdForm over all n columns ([A | I] as var_col says) in `state`'s basis, x and z."""
    from oracle import oracle as ora

    basis, nonbasis = np.asarray(get(state, "basis"), dtype=np.int64), np.asarray(get(state, "nonbasis"), dtype=np.int64)
    m, q = len(basis), len(nonbasis)
    codes = var_codes(m + q, ns, var_col)
    col_ptr, row_idx, val = ora.csc_from_dense(columns(a, m, codes))
    return ora.StdForm(m=m, n=m + q, col_ptr=col_ptr, row_idx=row_idx, val=val,
                       c=np.asarray(c, dtype=np.float64), constant=0.0, basis=basis.copy(),
                       nonbasis=nonbasis.copy(), x=np.asarray(get(state, "x"), dtype=np.float64).copy(),
                       z=np.asarray(get(state, "z"), dtype=np.float64).copy())


def referee(a, ns: int, c, exact: Exact, var_col=None):
    """The reference rule applied to the exact state rounded to double: the CPU oracle takes one
    pivot from it.  Returns (status, (kind, entering, leaving) or None when it stops first)."""
    from oracle import oracle as ora

    st = exact.rounded()
    res = ora.simplex_solve(stdform(a, ns, c, st, var_col), max_iter=1, xbar=st["xbar"], zbar=st["zbar"])
    piv = tuple(int(v) for v in res.pivots[0][:3]) if res.pivots else None
    return res.status, piv


def recompute_floor(binv, a, ns: int, start, exact: Exact, k: int, var_col=None) -> float:
    """How far k_drift's GPU recomputation of the state can be from `exact`, in the metric's units,
    given the inverse the refactorisation built (binv: all m rows, read back) -- so that
    |state_drift - D| <= this.  Per vector, entry by entry:

      x^:  |Binv r - x^|  (Binv's own error, in long double)  +  (k + 2) u |Binv| |r|
           (FTRAN's row function: k2 terms per row, then the basic slack's b)
      z^:  |N^T Binv^T c'_B - c'_N - z^|  +  |N|^T ((m/64 + 66) u |Binv|^T |c'_B|)
           (k_drift_y_part / _sum: 64 chunks of m/64 terms)  +  (m + 2) u |N|^T |y|  (pricing)
           +  u |z^|

    The metric of each vector moves by at most twice its error bound over max(1, ||v^||_inf)."""
    basis = np.asarray(get(start, "basis"), dtype=np.int64)
    m, q = len(exact.basis), len(exact.nonbasis)
    codes = var_codes(m + q, ns, var_col)
    x0 = np.asarray(get(start, "x"), dtype=np.float64)
    xb0 = get(start, "xbar")
    xb0 = np.ones(m) if xb0 is None else np.asarray(xb0, dtype=np.float64)
    zb0 = get(start, "zbar")
    zb0 = np.ones(q) if zb0 is None else np.asarray(zb0, dtype=np.float64)
    binv = np.asarray(binv, dtype=np.float64)
    binv_ld, abinv = binv.astype(LD), np.abs(binv)
    nmat = None
    floor = 0.0
    for name, vec in (("x", x0), ("xbar", xb0)):
        rr = _times(a, m, codes[basis], vec)
        phi = np.abs(binv_ld @ rr - getattr(exact, name)).astype(np.float64)
        phi += (k + 2) * U53 * (abinv @ np.abs(rr.astype(np.float64)))
        ref = getattr(exact, name)
        floor = max(floor, 2 * float(phi.max()) / max(1.0, float(np.abs(ref).max())))
    nb0 = np.asarray(get(start, "nonbasis"), dtype=np.int64)
    for name, zvec in (("z", np.asarray(get(start, "z"), dtype=np.float64)), ("zbar", zb0)):
        cc = np.zeros(m + q, dtype=LD)
        cc[nb0] = -zvec.astype(LD)
        cb = cc[exact.basis]
        y = binv_ld.T @ cb
        zz = _t_times(a, m, codes[exact.nonbasis], y) - cc[exact.nonbasis]
        ref = getattr(exact, name)
        phi = np.abs(zz - ref).astype(np.float64)
        if nmat is None:
            nmat = np.abs(columns(a, m, codes[exact.nonbasis]))
        ybound = (m // 64 + 66) * U53 * (abinv.T @ np.abs(cb.astype(np.float64)))
        phi += nmat.T @ ybound + (m + 2) * U53 * (nmat.T @ np.abs(y.astype(np.float64)))
        phi += U53 * np.abs(ref.astype(np.float64))
        floor = max(floor, 2 * float(phi.max()) / max(1.0, float(np.abs(ref).max())))
    return floor


def drift_vs_exact(s, lp, a, ns: int):
    """Refactorise the FAST solver s now and check its state_drift: (result, D's parts, floor), with
    |state_drift - D| <= floor (recompute_floor + the helper's own error) asserted."""
    s.refactor()
    r = s.result(log=False)
    binv, info = s.debug_inverse(0, lp.m)
    assert info["neta"] == 0 and info["k"] == r.dense_columns
    ex = exact_state(a, ns, lp, r.basis, r.nonbasis)
    d = ex.drift(r)
    floor = recompute_floor(binv, a, ns, lp, ex, info["k"]) + 2 * max(ex.err.values())
    assert abs(r.state_drift - d["D"]) <= floor, (r.state_drift, d, floor, r.iterations)
    assert r.state_drift >= d["D"] - floor, (r.state_drift, d, floor)
    return r, d, floor
