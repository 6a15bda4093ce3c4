"""The specification of unboundedness and infeasibility rays, written over the CPU oracle's
primitives.  Core sense: maximise c.x + constant, [A | I] x = rhs0, x >= 0.
The state is the one the solve stopped in -- basis B, nonbasic set N, carried x, xbar, z, zbar; the
failed pivot was not executed.

    UNBOUNDED -> primal ray
        r = find_first_pivot(z, zbar), j = N[r], mu = -z[r] / zbar[r]
        dx = LU::solve(B, a_j)                                   (ora.lu_solve)
        d[j] = 1, d[B[p]] = -dx[p], 0 for the other nonbasics
        value = c[j] - sum_p c[B[p]] * dx[p]      from c[j], p ascending, each product rounded, no FMA
        violation = max_p max(dx[p], 0)
    INFEASIBLE -> Farkas ray
        p = find_first_pivot(x, xbar), i = B[p], mu = -x[p] / xbar[p]
        y = LU::solve(B^T, e_p), dz = neg_t_dot(N, y)            (ora.lu_solve, ora.neg_t_dot)
        d[N[k]] = -dz[k], d[i] = 1, 0 for the other basics
        value = sum_i rhs0[i] * y[i]              rows ascending, each product rounded
        violation = max_k max(dz[k], 0)
    violation is NaN if the vector it is taken over holds a NaN
    proven = violation == 0.0 and (value > 0 for a primal ray, value < 0 for a Farkas ray)

and, for a model (dzg_model_map_ray): var[u] = d[x+_u] - d[x-_u]; con / ub / lb are the d of the
rows' slacks for a primal ray and the y of the rows for a Farkas ray (ub before lb per variable, in
order of first appearance, as in duals_reference.model_duals).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import oracle as ora

PRIMAL, FARKAS = 1, 2  # DZG_RAY_PRIMAL, DZG_RAY_FARKAS


@dataclass
class RefRay:
    kind: int
    var: int
    pos: int
    mu: float
    d: np.ndarray         # n, by variable
    y: np.ndarray         # m; zeros for a primal ray
    value: float
    violation: float
    proven: bool
    vec: np.ndarray       # dx (primal) or dz (Farkas): what violation is taken over


def basis_matrix(sf: "ora.StdForm", basis) -> np.ndarray:
    bmat = np.empty((sf.m, sf.m))
    for p, j in enumerate(basis):
        bmat[:, p] = ora.csc_column(sf.m, sf.col_ptr, sf.row_idx, sf.val, int(j))
    return bmat


def core_ray(sf: "ora.StdForm", res, rhs0=None) -> "RefRay | None":
    """The ray of the final state of `res` (status, basis, nonbasis, x, xbar, z, zbar) for the
    standard form `sf`; rhs0: the x the solve started with (default: sf.x).  None unless the status
    is "unbounded" or "infeasible"."""
    if res.status not in ("unbounded", "infeasible"):
        return None
    m, n = sf.m, sf.n
    basis = np.asarray(res.basis, dtype=np.int64)
    nonbasis = np.asarray(res.nonbasis, dtype=np.int64)
    rhs0 = np.asarray(sf.x if rhs0 is None else rhs0, dtype=np.float64)
    c = np.asarray(sf.c, dtype=np.float64)
    bmat = basis_matrix(sf, basis)
    d, y = np.zeros(n), np.zeros(m)
    with np.errstate(all="ignore"):
        if res.status == "unbounded":
            z, zbar = np.asarray(res.z, dtype=np.float64), np.asarray(res.zbar, dtype=np.float64)
            pos = ora.find_first_pivot(z, zbar)
            var = int(nonbasis[pos])
            mu = float(-z[pos] / zbar[pos])
            vec = ora.lu_solve(bmat, ora.csc_column(m, sf.col_ptr, sf.row_idx, sf.val, var))
            d[var] = 1.0
            d[basis] = -vec
            value = float(c[var])
            for p in range(m):
                prod = float(c[basis[p]]) * float(vec[p])
                value = value - prod
            kind = PRIMAL
        else:
            x, xbar = np.asarray(res.x, dtype=np.float64), np.asarray(res.xbar, dtype=np.float64)
            pos = ora.find_first_pivot(x, xbar)
            var = int(basis[pos])
            mu = float(-x[pos] / xbar[pos])
            unit = np.zeros(m)
            unit[pos] = 1.0
            y = ora.lu_solve(np.ascontiguousarray(bmat.T), unit)
            vec = ora.neg_t_dot(sf.col_ptr, sf.row_idx, sf.val, nonbasis, y)
            d[nonbasis] = -vec
            d[var] = 1.0
            value = 0.0
            for i in range(m):
                prod = float(rhs0[i]) * float(y[i])
                value = value + prod
            kind = FARKAS
        violation = float("nan") if np.isnan(vec).any() else float(np.maximum(vec, 0.0).max(initial=0.0))
    proven = violation == 0.0 and (value > 0.0 if kind == PRIMAL else value < 0.0)
    return RefRay(kind=kind, var=var, pos=int(pos), mu=mu, d=d, y=y, value=value, violation=violation,
                  proven=bool(proven), vec=vec)


@dataclass
class RefModelRay:
    var: np.ndarray
    con: np.ndarray
    lb: np.ndarray
    ub: np.ndarray


def model_ray(model: dict, kind: int, d, y) -> RefModelRay:
    """d (by variable) and y (by row) of the standard form of a JSON-style model
    (tests/golden/reference_kats.json) in the model's terms."""
    sf = ora.build_standard_form(model)
    d = np.asarray(d, dtype=np.float64)
    y = np.zeros(sf.m) if y is None else np.asarray(y, dtype=np.float64)
    assert len(d) == sf.n and len(y) == sf.m
    vs, cons = model["vars"], model.get("constraints", [])
    nv, nc = len(vs), len(cons)
    # the slack of row r: the unit column e_r of the starting basis
    slack = np.full(sf.m, -1, dtype=np.int64)
    for j in sf.basis:
        col = ora.csc_column(sf.m, sf.col_ptr, sf.row_idx, sf.val, int(j))
        assert np.count_nonzero(col) == 1 and col.max() == 1.0
        slack[int(np.argmax(col))] = int(j)
    assert (slack >= 0).all()
    row_value = (lambda r: d[slack[r]]) if kind == PRIMAL else (lambda r: y[r])
    seen = []
    for u, _ in model["objective"]["terms"]:
        if u not in seen:
            seen.append(u)
    for con in cons:
        for u, _ in con["terms"]:
            if u not in seen:
                seen.append(u)
    lb, ub = np.zeros(nv), np.zeros(nv)
    row = nc
    for u in seen:  # ub before lb, src/simplex.rs:141-148
        if vs[u].get("ub") is not None:
            ub[u] = row_value(row)
            row += 1
        if vs[u].get("lb") is not None:
            lb[u] = row_value(row)
            row += 1
    assert row == sf.m, (row, sf.m)
    var = np.zeros(nv)
    for u in range(nv):
        if sf.pos_col[u] >= 0:
            var[u] = d[sf.pos_col[u]] - d[sf.neg_col[u]]
    con = np.array([row_value(r) for r in range(nc)], dtype=np.float64).reshape(nc)
    return RefModelRay(var=var, con=con, lb=lb, ub=ub)


def json_model(problem) -> dict:
    """A Minimize / Maximize of the modelling surface as the JSON-style model the oracle reads, in
    the core sense (maximised, rows coef.x <= b); variable u is the u-th of dantzig_amd.rust.lower's
    table."""
    from dantzig_amd import rust

    arrays, order = rust.lower(*problem._rust_problem())
    nt, nc = arrays["obj_nterms"], arrays["ncons"]
    ptr = arrays["con_ptr"]
    return {
        "vars": [{"lb": v.lb, "ub": v.ub} for v in order],
        "objective": {"terms": [[int(arrays["obj_var"][t]), float(arrays["obj_coef"][t])] for t in range(nt)],
                      "constant": float(arrays["obj_const"])},
        "constraints": [{"terms": [[int(arrays["con_var"][e]), float(arrays["con_coef"][e])]
                                   for e in range(int(ptr[r]), int(ptr[r + 1]))],
                         "b": float(arrays["con_b"][r])} for r in range(nc)],
    }


def solve_model_ray(model: dict):
    """(standard form, oracle result, RefRay or None) of a JSON-style model."""
    sf = ora.build_standard_form(model)
    res = ora.simplex_solve(sf)
    return sf, res, core_ray(sf, res)
