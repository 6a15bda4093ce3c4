"""Helpers of the ray tests: two continuous LP families whose verdict is built in and found late in
the solve, the property check of a ray in a model's own terms, and the long-double ray of a basis."""
import numpy as np

from tests import rays_reference as rref


# ---------------------------------------------------------------- the two families
def _g1(seed, m, ns):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (m, ns)); x0 = rng.uniform(0, 1, ns); y0 = rng.uniform(0, 1, m)
    return rng, a, a @ x0 + rng.uniform(0, 1, m), a.T @ y0 - rng.uniform(0, 1, ns)


def unbounded_lp(seed, m, ns, delta=1e-3, ps=1e-2):
    """Feasible and dual feasible G1 data plus a column `at` such that column `at` + column j is a
    ray gaining delta: (a, b, c) of max c.x st a x <= b, x >= 0."""
    rng, a, b, c = _g1(seed, m, ns - 1)
    j = int(rng.integers(0, ns - 1)); at = int(rng.integers(0, ns))
    col = -a[:, j] - ps * rng.uniform(0.1, 1, m)
    return np.insert(a, at, col, axis=1), b, np.insert(c, at, -c[j] + delta)


def infeasible_lp(seed, m, ns, delta=1e-3, ps=1e-2):
    """The same plus a row `at` such that row `at` + row r reads (p >= 0).x <= -delta."""
    rng, a, b, c = _g1(seed, m - 1, ns)
    r = int(rng.integers(0, m - 1)); at = int(rng.integers(0, m))
    row = -a[r] + ps * rng.uniform(0.1, 1, ns)
    return np.insert(a, at, row, axis=0), np.insert(b, at, -b[r] - delta), c


# ---------------------------------------------------------------- a ray in the model's terms
TOL_SIGN = 1e-12   # the reference's own rays stay below 1.4e-15 on 3 000 such models
TOL_VALUE = 1e-9


def _rows(model):
    """(coefficients by variable, b) per user row; a repeated variable keeps its last coefficient."""
    out = []
    for con in model.get("constraints", []):
        coef = {}
        for u, k in con["terms"]:
            coef[u] = k
        out.append((coef, con["b"]))
    return out


def check_model_ray(model: dict, kind: int, var, con, lb, ub, value, what=""):
    """The properties a proven ray has in the terms of the JSON-style model (core sense: maximised,
    rows coef.x <= b): see tests/test_rays_host.py, test 2.  Returns the largest sign miss found."""
    vs = model["vars"]
    nv = len(vs)
    var, con, lb, ub = (np.asarray(v, dtype=np.float64) for v in (var, con, lb, ub))
    rows = _rows(model)
    worst = 0.0
    if kind == rref.PRIMAL:
        s = max(1.0, float(np.abs(var).max(initial=0.0)))
        for r, (coef, _) in enumerate(rows):
            lhs = sum(k * var[u] for u, k in coef.items())
            worst = max(worst, lhs / s)
            assert lhs <= TOL_SIGN * s, f"{what}: row {r} grows along the ray: {lhs}"
        for u in range(nv):
            if vs[u].get("ub") is not None:
                worst = max(worst, var[u] / s)
                assert var[u] <= TOL_SIGN * s, f"{what}: variable {u} leaves its upper bound"
            if vs[u].get("lb") is not None:
                worst = max(worst, -var[u] / s)
                assert var[u] >= -TOL_SIGN * s, f"{what}: variable {u} leaves its lower bound"
        cu = {}
        for u, k in model["objective"]["terms"]:
            cu[u] = k
        rate = sum(k * var[u] for u, k in cu.items())
        assert abs(rate - value) <= TOL_VALUE * abs(value), f"{what}: c.dir = {rate}, value = {value}"
    else:
        s = max(1.0, float(np.abs(con).max(initial=0.0)), float(np.abs(lb).max(initial=0.0)),
                float(np.abs(ub).max(initial=0.0)))
        for u in range(nv):
            agg = sum(coef.get(u, 0.0) * con[r] for r, (coef, _) in enumerate(rows)) + ub[u] - lb[u]
            worst = max(worst, abs(agg) / s)
            assert abs(agg) <= TOL_SIGN * s, f"{what}: variable {u} keeps coefficient {agg}"
        low = min(float(con.min(initial=0.0)), float(lb.min(initial=0.0)), float(ub.min(initial=0.0)))
        worst = max(worst, -low / s)
        assert low >= -TOL_SIGN * s, f"{what}: a multiplier is negative: {low}"
        rhs = sum(b * con[r] for r, (_, b) in enumerate(rows))
        for u in range(nv):
            if vs[u].get("ub") is not None:
                rhs += vs[u]["ub"] * ub[u]
            if vs[u].get("lb") is not None:
                rhs -= vs[u]["lb"] * lb[u]
        assert abs(rhs - value) <= TOL_VALUE * abs(value), f"{what}: b.y = {rhs}, value = {value}"
    return worst


# ---------------------------------------------------------------- long double
LD = np.longdouble


def refined_solve(bmat, rhs, trans: int, steps: int = 3):
    """B v = rhs (trans = 0) or B^T v = rhs (trans = 1): a double LU solve refined with residuals
    formed in long double, as tests/state_check.py does it."""
    import scipy.linalg as sla

    lu = sla.lu_factor(bmat)
    b_ld = bmat.astype(LD).T if trans else bmat.astype(LD)
    rhs = np.asarray(rhs, dtype=LD)
    v = sla.lu_solve(lu, rhs.astype(np.float64), trans=trans).astype(LD)
    for _ in range(steps):
        v = v + sla.lu_solve(lu, (rhs - b_ld @ v).astype(np.float64), trans=trans).astype(LD)
    return v


def dense_ray_vectors(a, basis, nonbasis, kind: int, pos: int, solve):
    """(d, y) of the ray of the basis for max c.x st a x <= b (variables: ns structurals, then the m
    slacks) with `solve(bmat, rhs, trans)` as the linear solve; products in the solve's precision."""
    m, ns = a.shape
    full = np.concatenate([a, np.eye(m)], axis=1)
    bmat = np.ascontiguousarray(full[:, basis])
    dtype = LD if solve is refined_solve else np.float64
    d, y = np.zeros(m + ns, dtype=dtype), np.zeros(m, dtype=dtype)
    if kind == rref.PRIMAL:
        j = int(nonbasis[pos])
        dx = solve(bmat, full[:, j], 0)
        d[j] = 1.0
        d[basis] = -dx
    else:
        unit = np.zeros(m)
        unit[pos] = 1.0
        y = solve(bmat, unit, 1)
        d[nonbasis] = full[:, nonbasis].astype(dtype).T @ y
        d[int(basis[pos])] = 1.0
    return d, y


def numpy_solve(bmat, rhs, trans: int):
    return np.linalg.solve(bmat.T if trans else bmat, rhs)
