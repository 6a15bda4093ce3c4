"""Shared pieces of the removal tests (tests/test_remove_host.py, tests/test_gpu_remove.py): what is
free to remove at a basis, the matrix cases, and the session's slack constraints.  The base LPs, the
cuts and columns of a round (`draw`) and the certificate are tests/extend_check.py's.

What is free at a basis: a row whose slack is basic, a structural column whose variable is nonbasic
(dzg_solver_remove).  `free_sets` lists every such row and every second such column in ascending
order; measured with HiGHS at the optimum of generator G1

    (31, 24, 40)    2 rows,  18 nonbasic columns, smallest basic slack 0.30
    (41, 37, 53)    9 rows,  25 nonbasic columns, smallest basic slack 0.0098
    (42, 300, 500) 15 rows, 215 nonbasic columns, smallest basic slack 0.027

(FREE_AT_LEAST; tests/test_remove_host.py asserts the first two through the CPU oracle on every run, so
that a GPU test that finds nothing to remove cannot pass silently).
"""
from __future__ import annotations

import dataclasses

import numpy as np

from dantzig_amd import core
from tests import extend_check as ec

base, draw, structural_values, check_certificate, BASES = (ec.base, ec.draw, ec.structural_values,
                                                           ec.check_certificate, ec.BASES)

# base -> (rows with a basic slack, nonbasic structural columns) at the optimum, at least
FREE_AT_LEAST = {(31, 24, 40): (2, 18), (41, 37, 53): (9, 25), (42, 300, 500): (15, 215)}

# The matrix cases of the GPU test: (m, ns, rows dropped, columns dropped), at the slack start, where
# everything is removable.  17x33 -[16] crosses lda 32 -> 16; 33x17 ends at m' = 16; 2050x8 crosses the
# 2048-row rule of the leading dimension downward; 300x500 draws its lists from a seed.
_rng = np.random.default_rng(300500)
MATRIX_CASES = [
    (2, 2, [1], []),
    (17, 33, [16], [0]),
    (17, 33, [0], [32]),
    (33, 17, list(range(1, 18)), []),
    (64, 64, list(range(0, 64, 2)), list(range(0, 64, 2))),
    (65, 130, [0, 64], [129]),
    (300, 500, sorted(_rng.choice(300, 15, replace=False).tolist()),
     sorted(_rng.choice(500, 200, replace=False).tolist())),
    (2050, 8, [0, 1024, 2049], []),
    (40, 24, [], [3, 4, 23]),          # columns only: the 16-byte path, m even
    (7, 9, [], [0]),                   # ... m odd
]

# Session.remove_constraints on the KAT models: the constraint of extend_check.ADDED loosened so that
# it is slack by 0.5 at the model's optimum (tests/test_remove_host.py checks >= 0.1 on the CPU).
LOOSENED = {
    "readme_quick_start": "z - 2 * x <= 1.5",
    "non_standard_variables": "x - 0.5 * y + z >= -5.5",
}


def at_basis(lp: core.CoreLP, res) -> core.CoreLP:
    """`lp` with the lists and the state of `res` (anything with basis, nonbasis, x, z)."""
    return dataclasses.replace(lp, basis=np.asarray(res.basis, dtype=np.int64).copy(),
                               nonbasis=np.asarray(res.nonbasis, dtype=np.int64).copy(),
                               x=np.asarray(res.x, dtype=np.float64).copy(),
                               z=np.asarray(res.z, dtype=np.float64).copy(), xbar=None, zbar=None)


def free_masks(lp: core.CoreLP):
    """(row_mask, col_mask) at lp.basis: rows with a basic slack, nonbasic structural columns -- what
    core.Solver.removable reports, computed on the host."""
    codes = ec.codes_of(lp)
    inb, out = codes[np.asarray(lp.basis)], codes[np.asarray(lp.nonbasis)]
    rows, cols = np.zeros(lp.m, bool), np.zeros(lp.n_struct, bool)
    rows[-1 - inb[inb < 0]] = True
    cols[out[out >= 0]] = True
    return rows, cols


def free_sets(lp: core.CoreLP):
    """(every row with a basic slack, every second nonbasic structural column) at lp.basis, ascending."""
    rows, cols = free_masks(lp)
    return np.flatnonzero(rows).tolist(), np.flatnonzero(cols)[::2].tolist()


def random_lp(m: int, ns: int) -> core.CoreLP:
    """The LP of a matrix case: uniform entries, the benchmark convention, the slack start."""
    rng = np.random.default_rng(1000 * m + ns)
    return core.CoreLP.from_inequality_form(rng.uniform(-1, 1, (m, ns)), rng.uniform(-1, 1, m),
                                            rng.uniform(-1, 1, ns))
