"""The specification of dual values and reduced costs, written over the CPU oracle's primitives
(DESIGN.md section 7d).  Core sense: maximise c.x + constant, [A | I] x = rhs, x >= 0.  At an
OPTIMAL basis B with nonbasic set N:

    y    = B^-T c_B                          LU::solve of B^T y = c_B (ora.lu_solve)
    d_N  = -neg_t_dot(N, y) - c_N            stored entries in row order (ora.neg_t_dot)
    d_B  = 0
    dual_obj = constant + sum_i rhs0[i] * y[i]     rows ascending, each product rounded, no FMA

and, for a model (dzg_model_map_duals): con_dual = y of the user rows, ub_dual / lb_dual = y of the
bound rows Simplex::new appends (ub before lb per variable, in order of first appearance), var_rc[u]
= c_u - sum_r a_{r,u} con_dual[r] over the user rows.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import oracle as ora


@dataclass
class RefDuals:
    y: np.ndarray         # m
    d: np.ndarray         # n, by variable, 0.0 for basics
    dual_obj: float
    primal_infeas: float
    dual_infeas: float
    z_diff: float


def core_duals(sf: "ora.StdForm", res, rhs0=None) -> RefDuals:
    """The duals of the final basis of `res` (anything with basis, nonbasis, x, z) for the standard
    form `sf`; rhs0: the x the solve started with (default: sf.x)."""
    m, n = sf.m, sf.n
    basis = np.asarray(res.basis, dtype=np.int64)
    nonbasis = np.asarray(res.nonbasis, dtype=np.int64)
    rhs0 = np.asarray(sf.x if rhs0 is None else rhs0, dtype=np.float64)
    c = np.asarray(sf.c, dtype=np.float64)
    bmat = np.empty((m, m))
    for p, j in enumerate(basis):
        bmat[:, p] = ora.csc_column(m, sf.col_ptr, sf.row_idx, sf.val, int(j))
    y = ora.lu_solve(np.ascontiguousarray(bmat.T), c[basis])
    d_n = -ora.neg_t_dot(sf.col_ptr, sf.row_idx, sf.val, nonbasis, y) - c[nonbasis]
    d = np.zeros(n)
    d[nonbasis] = d_n
    total = 0.0
    for i in range(m):
        prod = float(rhs0[i]) * float(y[i])
        total = total + prod
    x, z = np.asarray(res.x, dtype=np.float64), np.asarray(res.z, dtype=np.float64)
    dmax = float(np.abs(d_n).max(initial=0.0))
    return RefDuals(y=y, d=d, dual_obj=float(sf.constant) + total,
                    primal_infeas=max(0.0, -float(x.min(initial=np.inf))),
                    dual_infeas=max(0.0, -float(d_n.min(initial=np.inf))),
                    z_diff=float(np.abs(z - d_n).max(initial=0.0)) / max(1.0, dmax))


@dataclass
class RefModelDuals:
    con_dual: np.ndarray
    var_rc: np.ndarray
    lb_dual: np.ndarray
    ub_dual: np.ndarray


def model_duals(model: dict, y) -> RefModelDuals:
    """y of the standard form of a JSON-style model (tests/golden/reference_kats.json) in the
    model's terms."""
    y = np.asarray(y, dtype=np.float64)
    vs, cons = model["vars"], model.get("constraints", [])
    nv, nc = len(vs), len(cons)
    seen = []
    for u, _ in model["objective"]["terms"]:
        if u not in seen:
            seen.append(u)
    for con in cons:
        for u, _ in con["terms"]:
            if u not in seen:
                seen.append(u)
    lb_dual, ub_dual = np.zeros(nv), np.zeros(nv)
    row = nc
    for u in seen:  # ub before lb, src/simplex.rs:141-148
        if vs[u].get("ub") is not None:
            ub_dual[u] = y[row]
            row += 1
        if vs[u].get("lb") is not None:
            lb_dual[u] = y[row]
            row += 1
    assert row == len(y), (row, len(y))
    cu = np.zeros(nv)
    for u, coef in model["objective"]["terms"]:
        cu[u] = coef  # assignment: the last duplicate wins
    acc = np.zeros(nv)
    for r, con in enumerate(cons):
        row_coef = {}
        for u, coef in con["terms"]:
            row_coef[u] = coef
        for u, coef in row_coef.items():
            acc[u] = acc[u] + coef * y[r]
    return RefModelDuals(con_dual=y[:nc].copy(), var_rc=cu - acc, lb_dual=lb_dual, ub_dual=ub_dual)


# The three textbook models of the duals tests, in the JSON form of the golden fixtures (core sense:
# maximised, rows coef.x <= b) with the values the oracle gives.
NN = {"lb": 0.0, "ub": None}
T1 = {"vars": [NN, NN], "objective": {"terms": [[0, 3.0], [1, 5.0]], "constant": 0.0},
      "constraints": [{"terms": [[0, 1.0]], "b": 4.0}, {"terms": [[1, 2.0]], "b": 12.0},
                      {"terms": [[0, 3.0], [1, 2.0]], "b": 18.0}]}
# min 2x + 3y, x + y >= 4, x + 3y >= 6 lowered: max -2x - 3y, -x - y <= -4, -x - 3y <= -6
T2 = {"vars": [NN, NN], "objective": {"terms": [[0, -2.0], [1, -3.0]], "constant": 0.0},
      "constraints": [{"terms": [[0, -1.0], [1, -1.0]], "b": -4.0},
                      {"terms": [[0, -1.0], [1, -3.0]], "b": -6.0}]}
# max x + 2y, x + y == 3, x >= 0, 0 <= y <= 2
T3 = {"vars": [NN, {"lb": 0.0, "ub": 2.0}], "objective": {"terms": [[0, 1.0], [1, 2.0]], "constant": 0.0},
      "constraints": [{"terms": [[0, 1.0], [1, 1.0]], "b": 3.0},
                      {"terms": [[0, -1.0], [1, -1.0]], "b": -3.0}]}
TEXTBOOK = {"T1": (T1, 36.0), "T2": (T2, -9.0), "T3": (T3, 5.0)}


def solve_model_duals(model: dict):
    """(standard form, oracle result, RefDuals) of a JSON-style model."""
    sf = ora.build_standard_form(model)
    res = ora.simplex_solve(sf)
    return sf, res, (core_duals(sf, res) if res.status == "optimal" else None)
