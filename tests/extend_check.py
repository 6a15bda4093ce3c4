"""Shared pieces of the extension tests (tests/test_extend_host.py, tests/test_gpu_extend.py): the
cuts and columns a solved LP is extended by, and the maps between the numbering an extended handle
keeps and the benchmark numbering tests/optimality.certificate reads.

Base LP: core.gen_dense_lp(seed, m, ns) in the benchmark convention.  With x* its optimum by
structural column and y* its dual values by row, an extension (p rows, r columns, seed s) is drawn in
this order:

    rng = np.random.default_rng(s)
    rows = rng.random((p, ns))                  rhs = 0.9 * rows @ x*
    cols = 2 * rng.random((m + p, r)) - 1       c_cols = cols.T @ [y*; 0_p] + 0.5

rows > 0 and x* >= 0, so every cut is violated at x* (rows @ x* > rhs unless x* = 0 on its support);
every new column has the reduced cost a_j . y* - c_j = -0.5 at y*, so it prices out favourably.  The
extended LP stays feasible (x = 0 satisfies the cuts: rhs >= 0) and, for the cases below, bounded with
an optimum that differs from the base one's: checked on the CPU with HiGHS (test_extend_host.py checks
the small shapes again on every run).  Every GPU test that relies on it asserts it again through the
oracle or a cold solve, and that the continuation takes at least one pivot.
"""
from __future__ import annotations

import functools

import numpy as np

from dantzig_amd import core

# (p, r, s)
RECIPE = [(1, 0, 1), (3, 0, 2), (0, 1, 3), (0, 2, 4), (2, 2, 5), (5, 3, 6)]
BASES = [(31, 24, 40), (41, 37, 53), (42, 300, 500)]
LARGE = (43, 640, 1280)
LARGE_RECIPE = [(2, 2, 7), (17, 0, 8)]

# Session.add_constraints on the KAT models: name -> (the added constraint over the model's variables,
# violated by the model's optimum; a second b of its normal form; the constraint written with that b).
# non_standard_variables has a split free variable (y) and bound rows, inventory_balance's is an ==
# (two rows) with variables on both sides.
ADDED = {
    "readme_quick_start": ("z - 2 * x <= 0.5", 0.25, "z - 2 * x <= 0.25"),
    "non_standard_variables": ("x - 0.5 * y + z >= -4.5", -4.0, "x - 0.5 * y + z >= -4.0"),
    "inventory_balance": ("x_2 == 0.1 * x_1 + 2", 4.0, "x_2 == 0.1 * x_1 + 4.0"),
}


@functools.lru_cache(maxsize=None)
def base(seed: int, m: int, ns: int):
    """(a, b, c) of generator G1; shared and never written to."""
    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    a = np.ascontiguousarray(a)
    for v in (a, b, c):
        v.setflags(write=False)
    return a, b, c


def codes_of(lp: core.CoreLP) -> np.ndarray:
    """The column code of every variable: >= 0 a structural column, -1 - r the slack of row r."""
    if lp.var_col is not None:
        return np.asarray(lp.var_col, dtype=np.int64)
    v = np.arange(lp.n, dtype=np.int64)
    return np.where(v < lp.n_struct, v, -1 - (v - lp.n_struct))


def inequality_form(lp: core.CoreLP):
    """(a, b, c by structural column) of an LP in its slack start, whatever its numbering."""
    codes = codes_of(lp)
    assert (codes[np.asarray(lp.basis)] == -1 - np.arange(lp.m)).all(), "not a slack start"
    c = np.zeros(lp.n_struct)
    s = np.flatnonzero(codes >= 0)
    c[codes[s]] = np.asarray(lp.c)[s]
    return np.asarray(lp.a), np.asarray(lp.x), c


def to_benchmark(lp: core.CoreLP, variables) -> np.ndarray:
    """Variables of `lp`'s numbering in the benchmark numbering of inequality_form(lp): structural
    column j -> j, the slack of row r -> n_struct + r (what tests/optimality.certificate reads)."""
    codes = codes_of(lp)[np.asarray(variables, dtype=np.int64)]
    return np.where(codes >= 0, codes, lp.n_struct + (-1 - codes))


def structural_values(lp: core.CoreLP, res) -> np.ndarray:
    """x by structural column at the basis of `res`."""
    value = np.zeros(lp.n)
    value[np.asarray(res.basis)] = res.x
    codes = codes_of(lp)
    out = np.zeros(lp.n_struct)
    s = np.flatnonzero(codes >= 0)
    out[codes[s]] = value[s]
    return out


def draw(lp: core.CoreLP, x_star, y_star, p: int, r: int, s: int) -> dict:
    """The extension (p rows, r columns, seed s) of `lp` at its optimum (x* by structural column, y* by
    row), as the keyword arguments of core.extended_lp / core.Solver.extend."""
    m, ns = lp.m, lp.n_struct
    rng = np.random.default_rng(s)
    rows = rng.random((p, ns))
    rhs = 0.9 * rows @ np.asarray(x_star)
    cols = 2 * rng.random((m + p, r)) - 1
    c_cols = cols.T @ np.concatenate([np.asarray(y_star), np.zeros(p)]) + 0.5
    out = {}
    if p:
        out.update(rows=rows, rhs=rhs)
    if r:
        out.update(cols=cols, c_cols=c_cols)
    return out


def highs(lp: core.CoreLP):
    """(status, objective, x by structural column, y by row) of the LP by HiGHS (scipy): the maximised
    objective without the constant, y >= 0 the duals of a x <= b."""
    from scipy.optimize import linprog

    a, b, c = inequality_form(lp)
    r = linprog(-c, A_ub=a, b_ub=b, bounds=(0, None), method="highs")
    if r.status != 0:
        return r.status, None, None, None
    return 0, -float(r.fun), np.asarray(r.x), -np.asarray(r.ineqlin.marginals)


def check_certificate(lp: core.CoreLP, res, tol: float = 1e-9) -> dict:
    """tests/optimality.certificate of the final basis of `res` on `lp` (any numbering), held to the
    thresholds of tests/test_gpu_reopt.py; returns the certificate with "y" added."""
    from tests.optimality import certificate

    a, b, c = inequality_form(lp)
    basis = to_benchmark(lp, res.basis)
    cert = certificate(a, b, c, basis)
    scale = max(1.0, abs(cert["primal_obj"]))
    assert cert["primal_infeas"] <= tol and cert["dual_infeas"] <= tol, cert
    assert abs(cert["primal_obj"] - cert["dual_obj"]) <= tol * scale, cert
    assert abs(res.objective - lp.constant - cert["primal_obj"]) <= tol * scale, (res.objective, cert)
    # y = B^-T c_B, as the certificate solves it
    m, ns = a.shape
    bm, cb = np.zeros((m, m)), np.zeros(m)
    for pos, var in enumerate(basis):
        if var < ns:
            bm[:, pos], cb[pos] = a[:, var], c[var]
        else:
            bm[var - ns, pos] = 1.0
    cert["y"] = np.linalg.solve(bm.T, cb)
    cert["scale"] = scale
    return cert
