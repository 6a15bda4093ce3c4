"""A reference check of the basis inverse FAST numerics keeps (dzg_debug_basis_inverse).

The engine's own monitor, max_pivot_error, compares dx_p from FTRAN with -dz_r from BTRAN + pricing:
two summation orders of the same bilinear form e_p^T Binv a_q, which agree to rounding whatever
matrix Binv holds.  This module checks the matrix itself against the basis it claims to invert:

    R = Binv[rows] B - I[rows]         in long double (64-bit mantissa), B built from `basis`
    ||R_i||_inf <= c k_eff 2^-53 ||Binv_i||_1 max|B|        row by row

B's column j is A[:, basis[j]] for a structural variable (basis[j] < ns) and e_(basis[j] - ns) for a
slack.  `ratio` = the left side over the right side without c; the tests assert ratio <= c.
"""
from __future__ import annotations

import numpy as np

# a platform whose long double is double would make the residual as rough as what it measures
assert np.finfo(np.longdouble).nmant >= 63, "the inverse check needs an 80-bit long double"

U53 = 2.0 ** -53
# c of the criterion, per family of tests/test_gpu_inverse.py and tests/test_gpu_fullsize.py: 10x the
# worst ratio the family showed on an MI355X (C_INVERSE_OBSERVED; pytest -s prints them).  The CPU
# controls hold the loosest, C_MAX: a 1e-9 relative error in one entry of a 90-row inverse reads
# ~1.3e4 there (tests/test_inverse_check.py).
C_INVERSE_OBSERVED = {"1 refactorisation": 20.05, "2 eta file": 10.58, "3 sparse basis": 2.887,
                      "4 row-sharded": 2.118, "5 headline": 0.554,
                      "6 batch inverse": 1.623, "7 batch updates": 5.782}
C_INVERSE = {"1 refactorisation": 200.0, "2 eta file": 100.0, "3 sparse basis": 30.0,
             "4 row-sharded": 20.0, "5 headline": 6.0, "6 batch inverse": 16.3, "7 batch updates": 58.0}
# Families 6 and 7 (the batched FAST solver's inverse in LDS, tests/test_gpu_batch_fast_inverse.py)
# take their c from a reference instead: 10x the worst ratio of the float64 transcription of the
# documented algorithm (tests/batch_fast_reference.py) on the same inputs, all rows, rounded up;
# tests/test_batch_fast_inverse_host.py measures it again on every run and holds c to it.
C_REFERENCE_OBSERVED = {"6 batch inverse": 1.623, "7 batch updates": 5.782}
C_MAX = max(C_INVERSE.values())
ROWS_SAMPLED = 16   # rows checked where m >= 4096 (and where all rows would cost too much)
CHUNK = 512         # structural columns per long-double product


class Csc:
    """A CSC structural block: m rows, col_ptr / row_idx / val as CoreLP.from_csc takes them."""

    def __init__(self, m, col_ptr, row_idx, val):
        self.m = int(m)
        self.col_ptr = np.asarray(col_ptr, dtype=np.int64)
        self.row_idx = np.asarray(row_idx, dtype=np.int64)
        self.val = np.asarray(val, dtype=np.float64)

    def columns(self, cols) -> np.ndarray:
        out = np.zeros((self.m, len(cols)))
        for i, j in enumerate(cols):
            lo, hi = self.col_ptr[j], self.col_ptr[j + 1]
            out[self.row_idx[lo:hi], i] = self.val[lo:hi]
        return out


def _columns(a, cols) -> np.ndarray:
    return a.columns(cols) if isinstance(a, Csc) else np.asarray(a)[:, cols]


def basis_matrix(a, basis, ns: int) -> np.ndarray:
    """B itself (dense, m x m): for the synthetic checks; the GPU tests never form it."""
    basis = np.asarray(basis)
    m = len(basis)
    b = np.zeros((m, m))
    s = np.flatnonzero(basis < ns)
    b[:, s] = _columns(a, basis[s])
    sl = np.flatnonzero(basis >= ns)
    b[basis[sl] - ns, sl] = 1.0
    return b


def residual(binv_rows, rows, a, basis, ns: int, k_eff: int | None = None) -> np.ndarray:
    """Per-row ratio ||R_i||_inf / (k_eff 2^-53 ||Binv_i||_1 max|B|) of the rows `rows` of the
    inverse (binv_rows[i] = row rows[i]); k_eff defaults to max(1, structural basics)."""
    basis = np.asarray(basis)
    rows = np.asarray(rows, dtype=np.int64)
    binv_rows = np.asarray(binv_rows, dtype=np.float64).reshape(len(rows), len(basis))
    m = len(basis)
    s = np.flatnonzero(basis < ns)
    if k_eff is None:
        k_eff = max(1, len(s))
    lrows = binv_rows.astype(np.longdouble)
    r = np.zeros((len(rows), m), dtype=np.longdouble)
    sl = np.flatnonzero(basis >= ns)
    r[:, sl] = lrows[:, basis[sl] - ns]
    amax = 1.0
    for c0 in range(0, len(s), CHUNK):
        blk = _columns(a, basis[s[c0:c0 + CHUNK]])
        if blk.size:
            amax = max(amax, float(np.abs(blk).max()))
        r[:, s[c0:c0 + CHUNK]] = lrows @ blk.astype(np.longdouble)
    r[np.arange(len(rows)), rows] -= 1
    res = np.abs(r).max(axis=1).astype(np.float64)
    bound = k_eff * U53 * np.abs(binv_rows).sum(axis=1) * amax
    return res / bound


def sample_rows(m: int, basis, ns: int, recent=(), n: int = ROWS_SAMPLED, seed: int = 0,
                every_below: int = 0) -> np.ndarray:
    """Rows to check: all of them when m < every_below; otherwise n random ones plus a structural
    and a slack position, the first and last row of a 64-row panel and the positions in `recent`
    (the last pivots')."""
    if m < every_below:
        return np.arange(m)
    basis = np.asarray(basis)
    rng = np.random.default_rng(seed)
    must = [int(p) for p in recent if 0 <= p < m]
    st, sl = np.flatnonzero(basis < ns), np.flatnonzero(basis >= ns)
    for group in (st, sl):
        if len(group):
            must += [int(group[0]), int(group[-1]), int(rng.choice(group))]
    panel = int(rng.integers(0, max(1, m // 64)))
    must += [min(m - 1, 64 * panel), min(m - 1, 64 * panel + 63), 0, m - 1]
    rest = rng.choice(m, size=min(m, n), replace=False)
    return np.unique(np.concatenate([np.array(must, dtype=np.int64), rest.astype(np.int64)]))


def last_pivot_positions(basis, pivots, count: int = 4) -> list:
    """Basis positions of the variables the last `count` pivots brought in (still basic there)."""
    basis = np.asarray(basis)
    out = []
    for _, entering, _, _ in list(pivots)[-count:]:
        hit = np.flatnonzero(basis == entering)
        out += [int(h) for h in hit]
    return out
