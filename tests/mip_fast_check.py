"""Checks of a branch and bound whose node LPs ran in FAST numerics (dzg_mip_solve_nodes, DESIGN.md
7c "FAST node LPs").  Not a test: tests/test_mip_fast_host.py tests the checker on the CPU,
tests/test_gpu_mip_fast.py runs it on the GPU search.

check_search   one search against the CPU oracle node by node: each logged node's bounds are rebuilt
               from its parent chain, its node model is solved by mip_reference.solve_node, and the
               status must be the same, the objective within within_tol (tests/test_gpu_mip_warm.py's
               rule) and bit-equal where the node's route is STRICT (0: batched, 2: FAST rejected,
               then STRICT); then the incumbent is checked against the model itself.
certificate    the acceptance certificate of k_mip_node_fast in float64: the inverse of the final
               basis by Gauss-Jordan with partial pivoting, x = W rhs and y = W^T c_B in dot4's order,
               z = N^T y - c_N, and the sign check against DZG_MIP_WARM_TOL.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle as ora
from tests import mip_reference as mr
from tests import mip_warm_reference as mw

INF = math.inf
ROUTE_STRICT, ROUTE_FAST, ROUTE_REJECTED, ROUTE_SEQUENTIAL = 0, 1, 2, 3


def within_tol(a, b):
    return abs(a - b) <= 1e-9 * max(1.0, abs(b)) + 1e-9


def root_bounds(md, flags):
    ints = [u for u, f in enumerate(flags) if f]
    bnd = []
    for u in ints:
        v = md["vars"][u]
        bnd += [-INF if v.get("lb") is None else float(v["lb"]), INF if v.get("ub") is None else float(v["ub"])]
    return ints, bnd


def node_bounds(md, flags, log):
    """{node id: bounds} of every logged node, each from its parent's (log entries are
    (id, parent, branch_var, direction, bound, ...); a parent is logged before its children)."""
    ints, root = root_bounds(md, flags)
    k_of = {u: k for k, u in enumerate(ints)}
    out = {}
    for e in log:
        i, parent, bvar, direction, bound = e[:5]
        if parent < 0:
            out[i] = list(root)
            continue
        assert parent in out, f"node {i}: its parent {parent} is not logged before it"
        cb = list(out[parent])
        cb[2 * k_of[bvar] + (1 if direction < 0 else 0)] = bound
        out[i] = cb
    return ints, out


def cold_children(md, flags, log):
    """The logged children whose branch made a bound finite (another structure: a cold start)."""
    ints, bnds = node_bounds(md, flags, log)
    return [e[0] for e in log if e[1] >= 0 and mw.mask_of(bnds[e[0]]) != mw.mask_of(bnds[e[1]])]


def check_search(md, flags, res, values, log, route, *, int_tol=1e-6, cold_objective=None):
    """Raises AssertionError unless the search (res: anything with status / has_incumbent / objective;
    values: the incumbent's; log: 8-tuples as rust._mip_call returns them; route: one code per log
    entry) is right node by node and at its incumbent.  cold_objective: the cold reference search's
    optimum, when the search ran to the end."""
    assert len(route) == len(log), (len(route), len(log))
    ints, bnds = node_bounds(md, flags, log)
    for e, rt in zip(log, route):
        i, st, obj = e[0], e[5], e[7]
        want_st, _, want_obj, _ = mr.solve_node(mr.node_model(md, ints, bnds[i]))
        assert st == want_st, f"node {i} (route {rt}): status {st}, the oracle's {want_st}"
        if st != 0:
            continue
        assert obj is not None and within_tol(obj, want_obj), f"node {i} (route {rt}): {obj!r} vs {want_obj!r}"
        if rt in (ROUTE_STRICT, ROUTE_REJECTED):
            assert obj == want_obj, f"node {i} (route {rt}) is STRICT: {obj!r} is not {want_obj!r} bit for bit"
    if not res.has_incumbent:
        assert cold_objective is None, "the cold search has an optimum, this one has no incumbent"
        return
    vals = np.asarray(values, dtype=float)[:len(flags)]
    for u in ints:
        assert abs(vals[u] - round(vals[u])) <= int_tol, f"variable {u} = {vals[u]!r} is not integral"
    for u, v in enumerate(md["vars"]):
        if v.get("lb") is not None:
            assert vals[u] >= v["lb"] - 1e-7, (u, vals[u], v["lb"])
        if v.get("ub") is not None:
            assert vals[u] <= v["ub"] + 1e-7, (u, vals[u], v["ub"])
    for r, con in enumerate(md["constraints"]):
        lhs = sum(coef * vals[u] for u, coef in con["terms"])
        assert lhs <= con["b"] + 1e-7, f"constraint {r}: {lhs!r} > {con['b']!r}"
    obj = sum(coef * vals[u] for u, coef in md["objective"]["terms"]) + md["objective"].get("constant", 0.0)
    assert within_tol(obj, res.objective), f"c.values + constant = {obj!r}, the search reports {res.objective!r}"
    if cold_objective is not None:
        assert within_tol(res.objective, cold_objective), (res.objective, cold_objective)


# ---------------------------------------------------------------- the certificate, float64
def dot4(rows, v):
    """rows @ v in the kernel's order: four interleaved partial sums, j ascending, then
    (s0 + s1) + (s2 + s3); every product rounded before it is added."""
    m = len(v)
    s = [np.zeros(rows.shape[0]) for _ in range(4)]
    for j in range(m):
        s[j % 4] = s[j % 4] + rows[:, j] * v[j]
    return (s[0] + s[1]) + (s[2] + s[3])


def gauss_jordan_inverse(b):
    """B^-1 by Gauss-Jordan with partial pivoting (first maximum of |.|, lowest row on ties), the
    row swaps undone as column swaps at the end; None when a pivot is zero or not finite."""
    m = b.shape[0]
    w = np.array(b, dtype=float)
    piv = []
    for k in range(m):
        pr = k + int(np.argmax(np.abs(w[k:, k])))
        piv.append(pr)
        if pr != k:
            w[[k, pr]] = w[[pr, k]]
        pivot = w[k, k]
        if not (pivot != 0.0) or not math.isfinite(pivot):
            return None
        colk = w[:, k].copy()
        w[:, k] = 0.0
        w[k, k] = 1.0
        rowk = w[k] / pivot
        w = w - np.outer(colk, rowk)  # every product rounded before it is subtracted; row k is replaced below
        w[k] = rowk
    for k in range(m - 1, -1, -1):
        if piv[k] != k:
            w[:, [k, piv[k]]] = w[:, [piv[k], k]]
    return w


def certificate(sf, basis, nonbasis, tol=mw.WARM_TOL):
    """(accepted, x, z) of the basis for the standard form sf (an oracle StdForm in its initial
    state: sf.x is the right-hand side)."""
    basis, nonbasis = np.asarray(basis, dtype=np.int64), np.asarray(nonbasis, dtype=np.int64)
    dense = ora.csc_to_dense(sf.m, sf.n, sf.col_ptr, sf.row_idx, sf.val)
    w = gauss_jordan_inverse(dense[:, basis])
    if w is None:
        return False, None, None
    x = dot4(w, np.asarray(sf.x, dtype=float))
    y = dot4(np.ascontiguousarray(w.T), np.asarray(sf.c, dtype=float)[basis])
    z = dense[:, nonbasis].T @ y - np.asarray(sf.c, dtype=float)[nonbasis]
    ok = bool(np.all(x >= -tol)) and bool(np.all(z >= -tol))  # NaN fails
    return ok, x, z
