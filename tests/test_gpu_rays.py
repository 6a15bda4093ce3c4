"""Unboundedness and infeasibility rays on the GPU (csrc/k_rays.hip, dzg_solver_ray,
dzg_batch_solve_rays, solve(rays=True)): the batch and the STRICT handle are the reference's
arithmetic bit for bit (tests/rays_reference.py), FAST is held to a multiple of LAPACK's own error
against long-double vectors, CSC solvers say that they have no rays, and the verdicts the reference's
pivot rule gets wrong on degenerate data come back unproven."""
import functools

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi, core, rust
from oracle import oracle as ora
from tests import rays_reference as rref
from tests.duals_helpers import assert_bit_equal, assert_same_run, random_problem
from tests.rays_helpers import (LD, check_model_ray, dense_ray_vectors, infeasible_lp, numpy_solve,
                                refined_solve, unbounded_lp)
from tests.test_gpu_duals import C_DUALS, _metric, _same_state, _strict_set
from tests.test_rays_host import COUNTS, UNPROVEN_UNBOUNDED

pytestmark = pytest.mark.gpu

# FAST against the long-double ray of the returned basis: the error ratio (device error / numpy's
# double-precision solve error, same metric) an MI355X shows per case, as (d, y); the bound is 32
# (pytest -s prints them)
C_RAYS_OBSERVED = {"97x161 unbounded": (0.005, 0.0), "97x161 infeasible": (0.000, 0.000),
                   "150x260 unbounded": (0.000, 0.0), "150x260 infeasible": (0.000, 0.000),
                   "300x520 unbounded": (0.003, 0.0), "300x520 infeasible": (0.000, 0.000),
                   "8x17000 unbounded": (0.002, 0.0), "8x17000 infeasible": (0.000, 0.000)}
# (before the FAST route refined its vectors once against a double-double residual, 97x161 unbounded
# stood at 48.5: the explicit inverse loses |M| |a_j| eps where the entering column nearly cancels a
# basic one, and numpy's own error on that system is small by luck)


# ------------------------------------------------------------------ 1. textbook, end to end
def test_textbook_models_end_to_end():
    for cls, sign in ((dz.Maximize, 1.0), (dz.Minimize, -1.0)):
        x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
        row = x - y <= 1.0
        problem = cls(sign * (x + y)).subject_to(row)
        with pytest.raises(dz.exceptions.UnboundedError) as info:
            problem.solve(rays=True)
        ray = info.value.ray
        assert ray.proven and ray.violation == 0.0
        assert ray.objective_rate > 0 if sign > 0 else ray.objective_rate < 0
        dx, dy = ray.direction(x), ray.direction(y)
        assert dx - dy <= 1e-12 and dx >= 0.0 and dy >= 0.0 and dx + dy > 0.0
        assert abs(sign * (dx + dy) - ray.objective_rate) <= 1e-12
        assert ray.slack_rate(row)[0] >= 0.0
        with pytest.raises(dz.exceptions.UnboundedError) as info:
            problem.solve()
        assert info.value.ray is None

    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    c1, c2 = x + y <= 1.0, x + y >= 2.0
    problem = dz.Maximize(x).subject_to([c1, c2])
    with pytest.raises(dz.exceptions.InfeasibleError) as info:
        problem.solve(rays=True)
    ray = info.value.ray
    assert ray.proven and ray.violation == 0.0 and ray.rhs_value < 0
    m1, m2 = ray.multiplier(c1), ray.multiplier(c2)
    assert m1 >= 0.0 >= m2 and m1 > 0.0
    for v in (x, y):  # the combined row has no variable left: m1 + m2 + ub - lb on each
        lb, ub = ray.bound_multipliers(v)
        assert lb >= 0.0 and ub == 0.0
        assert abs(m1 + m2 + ub - lb) <= 1e-12 and abs(ray.aggregated(v)) <= 1e-12
    assert abs((1.0 * m1 + 2.0 * m2) - ray.rhs_value) <= 1e-12
    with pytest.raises(dz.exceptions.InfeasibleError) as info:
        problem.solve()
    assert info.value.ray is None
    # an optimal solve is what it was, with duals too
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    c3 = x + y <= 4.0
    sol = dz.Maximize(x + 2 * y).subject_to(c3).solve(rays=True, duals=True)
    assert abs(sol.objective_value - 8.0) <= 1e-12 and abs(sol.dual(c3) - 2.0) <= 1e-12


# ------------------------------------------------------------------ 2, 3. the batch is the reference
@functools.lru_cache(maxsize=None)
def _ref_rays():
    """RefRay or None per LP of test_gpu_duals._strict_set (kinds 1 and 2, seeds 0..199, and its
    kind-0 set), computed once."""
    return [rref.core_ray(ora.stdform_from_dense(a, b, c), res) for _, a, b, c, _, res, _ in _strict_set()]


@functools.lru_cache(maxsize=None)
def _rays_batch():
    return core.solve_batch([item[4] for item in _strict_set()], rays=True, log_cap=1 << 12)


def _assert_ray(got, ref, what):
    assert got is not None and got.kind_code == ref.kind, what
    assert got.kind == ("primal" if ref.kind == rref.PRIMAL else "farkas"), what
    assert (got.var, got.pos) == (ref.var, ref.pos), what
    assert_bit_equal([got.mu, got.value, got.violation], [ref.mu, ref.value, ref.violation], what + " scalars")
    assert_bit_equal(got.d, ref.d, what + " d")
    assert_bit_equal(got.y, ref.y, what + " y")
    assert got.proven == ref.proven, what


def test_batch_rays_are_the_reference():
    items, refs, got = _strict_set(), _ref_rays(), _rays_batch()
    plain = core.solve_batch([item[4] for item in items], log_cap=1 << 12)
    counts = {0: {}, 1: {}, 2: {}}
    unproven = {0: [], 1: [], 2: []}
    seeds = {0: 0, 1: 0, 2: 0}
    for i, ((kind, a, b, c, lp, res, _), ref, g, p) in enumerate(zip(items, refs, got, plain)):
        what = f"LP {i} (kind {kind}, {a.shape[0]} x {a.shape[1]})"
        seed = seeds[kind]
        seeds[kind] += 1
        assert_same_run(g, p, what)       # res is what dzg_batch_solve fills
        assert_same_run(g, res, what)     # ... which is the oracle's run
        if ref is None:
            assert res.status in ("optimal", "panic") and g.ray is None, what
            continue
        _assert_ray(g.ray, ref, what)
        key = (g.status, g.ray.proven)
        counts[kind][key] = counts[kind].get(key, 0) + 1
        if g.status == "unbounded" and not g.ray.proven:
            unproven[kind].append(seed)
    assert counts[1] == COUNTS[1] and counts[2] == COUNTS[2], counts
    assert unproven[1] == UNPROVEN_UNBOUNDED[1] and unproven[2] == UNPROVEN_UNBOUNDED[2], unproven
    assert {s for _, _, _, _, _, res, _ in items for s in [res.status]} >= {"optimal", "unbounded", "infeasible",
                                                                            "panic"}
    # with the duals as well: both are what they are alone
    some = [i for i in range(0, len(items), 9)]
    both = core.solve_batch([items[i][4] for i in some], rays=True, duals=True, log_cap=1 << 12)
    alone = core.solve_batch([items[i][4] for i in some], duals=True, log_cap=1 << 12)
    for i, g, d in zip(some, both, alone):
        what = f"LP {i} rays + duals"
        assert_same_run(g, d, what)
        assert (g.duals is None) == (d.duals is None) and (g.ray is None) == (got[i].ray is None), what
        if g.duals is not None:
            assert_bit_equal(g.duals.y, d.duals.y, what + " y")
            assert_bit_equal(g.duals.d, d.duals.d, what + " d")
        if g.ray is not None:
            _assert_ray(g.ray, refs[i], what)


def _handle_ray(lp, status, what, **opts):
    with core.Solver(lp, **opts) as s:
        assert s.run(0) == status, what
        return s.result(log=False), s.ray()


def test_strict_handle_equals_the_batch():
    items, refs, batch = _strict_set(), _ref_rays(), _rays_batch()
    checked = 0
    for i, ((kind, a, b, c, lp, res, _), ref, g) in enumerate(zip(items, refs, batch)):
        if ref is None:
            continue
        what = f"LP {i} (kind {kind}, {a.shape[0]} x {a.shape[1]})"
        _, ray = _handle_ray(lp, res.status, what, numerics=core.STRICT)
        _assert_ray(ray, ref, what)
        assert_bit_equal(ray.d, g.ray.d, what + " d against the batch")
        checked += 1
    assert checked == 154 + 20 + 40 + 13


# above the batch limit, inside AUTO's STRICT range; and 8 x 17 000, whose q is beyond the 16 384
# threads of k_ray_finish
@pytest.mark.parametrize("make,status", [(unbounded_lp, "unbounded"), (infeasible_lp, "infeasible")],
                         ids=["unbounded", "infeasible"])
@pytest.mark.parametrize("m,ns", [(150, 260), (8, 17000)])
def test_default_handle_is_the_reference(m, ns, make, status):
    a, b, c = make(0, m, ns)
    sf = ora.stdform_from_dense(a, b, c)
    res = ora.simplex_solve(sf)
    assert res.status == status
    ref = rref.core_ray(sf, res)
    assert ref.proven and ref.violation == 0.0
    r, ray = _handle_ray(core.CoreLP.from_inequality_form(a, b, c), status, f"{m} x {ns}")
    assert r.numerics == "strict" and r.basis.tolist() == res.basis.tolist()
    _assert_ray(ray, ref, f"{m} x {ns} {status}")


# ------------------------------------------------------------------ 4. preconditions
def test_preconditions():
    a, b, c = core.gen_dense_lp(seed=5, m=20, n_struct=30)
    lp = core.CoreLP.from_inequality_form(np.array(a), b, c)
    with core.Solver(lp, numerics=core.STRICT) as s:
        s.run(3)  # stopped by its budget
        with pytest.raises(_ffi.DantzigAmdError, match="UNBOUNDED.*INFEASIBLE"):
            s.ray()
        assert s.run(0) == "optimal"
        with pytest.raises(_ffi.DantzigAmdError, match="UNBOUNDED.*INFEASIBLE"):
            s.ray()
        assert _ffi.lib().dzg_solver_ray(s._h, None) == _ffi.E_ARG
    a, b, c = unbounded_lp(0, 33, 50)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), numerics=core.FAST, refactor_interval=0) as s:
        assert s.run(0) == "unbounded"
        before = s.result(log=False)
        with pytest.raises(_ffi.DantzigAmdError, match="refactor_interval"):
            s.ray()
        _same_state(before, s.result(log=False), "a refused ray() leaves the solver alone")


# ------------------------------------------------------------------ 5. FAST against long double
# 8 x 17 000: q beyond the 16 384 threads of k_ray_finish; m = 300 is beyond the 256 rows of one
# workgroup of k_ray_v_fast, every m here beyond the 64 lanes k_ray_dx_fast strides by
@pytest.mark.parametrize("make,status", [(unbounded_lp, "unbounded"), (infeasible_lp, "infeasible")],
                         ids=["unbounded", "infeasible"])
@pytest.mark.parametrize("m,ns", [(97, 161), (150, 260), (300, 520), (8, 17000)])
def test_fast_rays_against_long_double(m, ns, make, status):
    a, b, c = make(0, m, ns)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=-1) as s:
        assert s.run(0) == status
        before = s.result(log=False)
        ray = s.ray()
        after = s.result(log=False)
        again = s.ray()
    _same_state(before, after, f"{m} x {ns}: result() around ray()")
    assert_bit_equal(ray.d, again.d, "second call d")
    assert_bit_equal(ray.y, again.y, "second call y")
    assert_bit_equal([ray.mu, ray.value, ray.violation], [again.mu, again.value, again.violation],
                     "second call scalars")
    assert (ray.var, ray.pos, ray.proven, ray.kind) == (again.var, again.pos, again.proven, again.kind)
    if status == "unbounded":
        pos = ora.find_first_pivot(before.z, before.zbar)
        assert ray.kind == "primal" and ray.pos == pos and ray.var == before.nonbasis[pos]
        assert (ray.y == 0.0).all()
    else:
        pos = ora.find_first_pivot(before.x, before.xbar)
        assert ray.kind == "farkas" and ray.pos == pos and ray.var == before.basis[pos]
    kind = rref.PRIMAL if status == "unbounded" else rref.FARKAS
    d_hat, y_hat = dense_ray_vectors(a, before.basis, before.nonbasis, kind, pos, refined_solve)
    d_np, y_np = dense_ray_vectors(a, before.basis, before.nonbasis, kind, pos, numpy_solve)
    base_d, base_y = _metric(d_np, d_hat), _metric(y_np, y_hat)
    tol_d, tol_y = max(C_DUALS * base_d, 1e-13), max(C_DUALS * base_y, 1e-13)
    err_d, err_y = _metric(ray.d, d_hat), _metric(ray.y, y_hat)
    ratio_d, ratio_y = err_d / max(base_d, 1e-13 / C_DUALS), err_y / max(base_y, 1e-13 / C_DUALS)
    if kind == rref.PRIMAL:
        value_hat = float(np.concatenate([c, np.zeros(m)]).astype(LD) @ d_hat)
    else:
        value_hat = float(np.asarray(b, dtype=LD) @ y_hat)
    print(f"\n{m}x{ns} {status}: k = {before.dense_columns}, pivots = {before.iterations}: d error "
          f"{err_d:.3e} (ratio {ratio_d:.3f}), y error {err_y:.3e} (ratio {ratio_y:.3f}), value {ray.value!r} "
          f"(long double {value_hat!r}), violation {ray.violation:.3e}, proven {ray.proven}")
    assert err_d <= tol_d, (err_d, tol_d)
    assert err_y <= tol_y, (err_y, tol_y)
    assert abs(ray.value - value_hat) <= max(tol_d, tol_y) * max(1.0, abs(value_hat))
    assert ray.violation <= 1e-9
    assert ray.proven == (ray.violation == 0.0 and (ray.value > 0 if kind == rref.PRIMAL else ray.value < 0))


# ------------------------------------------------------------------ 6. CSC: no rays
def test_csc_solvers_have_no_rays():
    a, b, c = infeasible_lp(0, 33, 50)
    col_ptr, row_idx, val = ora.csc_from_dense(a)
    lp = core.CoreLP.from_csc(33, col_ptr, row_idx, val, b, c)
    with core.Solver(lp, numerics=core.FAST) as s:
        assert s.run(0) == "infeasible"
        with pytest.raises(NotImplementedError, match="not supported"):
            s.ray()
        out = _ffi.Ray()
        import ctypes as C
        assert _ffi.lib().dzg_solver_ray(s._h, C.byref(out)) == _ffi.E_ARG
        assert s.result(log=False).status == "infeasible"
    # the model route: a standard form large and sparse enough to be stored as CSC (2 200 rows x
    # 2 200 structural columns); the reference ends it INFEASIBLE after 2 pivots
    xs = [dz.Variable.nonneg() for _ in range(1100)]
    problem = dz.Maximize(xs[0]).subject_to([xs[0] + xs[1] <= 1.0, xs[0] + xs[1] >= 2.0] +
                                            [x <= 1.0 for x in xs[2:]])
    with pytest.raises(dz.exceptions.InfeasibleError) as info:
        problem.solve(rays=True)
    assert info.value.ray is None


# ------------------------------------------------------------------ 7. solve_many(rays=True)
def _ray_fields(exc):
    ray = exc.ray._ray
    ids = sorted(ray.var)
    return ([ray.value, ray.violation, ray.mu] + [ray.var[i] for i in ids] + list(ray.con) +
            [ray.lb[i] for i in ids] + [ray.ub[i] for i in ids]), (ray.kind, ray.proven)


def test_solve_many_with_rays_equals_one_solve_per_model():
    rng = np.random.default_rng(78)
    items = [random_problem(rng, int(rng.integers(0, 12))) for _ in range(24)]
    got = dz.solve_many([p for _, p in items], rays=True, return_exceptions=True)
    both = dz.solve_many([p for _, p in items], rays=True, duals=True, return_exceptions=True)
    duals = dz.solve_many([p for _, p in items], duals=True, return_exceptions=True)
    kinds = set()
    for i, ((vs, p), g, gb, gd) in enumerate(zip(items, got, both, duals)):
        assert type(g) is type(gb) is type(gd), (i, g, gb, gd)
        try:
            w = p.solve(rays=True)
        except Exception as e:  # noqa: BLE001
            assert type(g) is type(e) and f"(model {i})" in str(g), (i, g, e)
            kinds.add(type(e).__name__)
            if not isinstance(e, dz.exceptions.SolveError):
                continue
            assert type(g.ray) is type(e.ray) is type(gb.ray) and g.ray is not None, i
            fg, kg = _ray_fields(g)
            fe, ke = _ray_fields(e)
            fb, kb = _ray_fields(gb)
            assert kg == ke == kb, i
            assert_bit_equal(fg, fe, f"model {i} ray")
            assert_bit_equal(fb, fe, f"model {i} ray, with duals")
            if g.ray.proven:  # the property check of tests/test_rays_host.py on the returned object
                model = rref.json_model(p)
                order = rust.lower(*p._rust_problem())[1]
                ray = g.ray._ray
                by_order = lambda table: [table[v.id] for v in order]  # noqa: E731
                check_model_ray(model, rref.PRIMAL if ray.kind == "primal" else rref.FARKAS, by_order(ray.var),
                                ray.con, by_order(ray.lb), by_order(ray.ub), ray.value, f"model {i}")
                kinds.add("proven " + ray.kind)
            continue
        kinds.add("optimal")
        assert_bit_equal([g.objective_value, gb.objective_value], [w.objective_value] * 2, f"model {i}")
        assert_bit_equal([g[v] for v in vs], [w[v] for v in vs], f"model {i} values")
        assert_bit_equal([gb.dual(con) for con in p.constraints], [gd.dual(con) for con in p.constraints],
                         f"model {i} duals")
        assert_bit_equal([gb.reduced_cost(v) for v in vs], [gd.reduced_cost(v) for v in vs],
                         f"model {i} reduced costs")
        cb, cd = gb.certificate, gd.certificate
        assert_bit_equal([cb.primal_objective, cb.dual_objective, cb.gap, cb.z_diff],
                         [cd.primal_objective, cd.dual_objective, cd.gap, cd.z_diff], f"model {i} certificate")
    assert {"optimal", "proven primal", "proven farkas"} <= kinds, kinds
