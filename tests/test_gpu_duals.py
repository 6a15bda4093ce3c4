"""Dual values and reduced costs on the GPU (csrc/k_duals.hip, dzg_solver_duals,
dzg_batch_solve_duals, solve(duals=True)): STRICT is the reference's arithmetic bit for bit
(tests/duals_reference.py), FAST is held to a multiple of LAPACK's own error against long-double
values, CSC solvers hand back the carried values and say so."""
import ctypes as C
import functools

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi, core
from oracle import oracle as ora
from tests import duals_reference as dref
from tests import state_check as sc
from tests.lp_families import make_lp
from tests.duals_helpers import (assert_bit_equal, assert_same_run, family as _family, long_double_y,
                                 random_problem as _random_problem)

pytestmark = pytest.mark.gpu

# FAST against the long-double values of the returned basis: the error ratio (device error /
# numpy's double-precision solve error, same metric) an MI355X shows per shape, as (y, d_N); the bound
# is 32 (pytest -s prints them)
C_DUALS_OBSERVED = {"97x161": (1.994, 2.634), "601x1203": (2.422, 2.305)}
C_DUALS = 32.0


# ------------------------------------------------------------------ 1. textbook, end to end
def test_textbook_models_end_to_end():
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    c1, c2, c3 = x <= 4.0, 2 * y <= 12.0, 3 * x + 2 * y <= 18.0
    t1 = dz.Maximize(3 * x + 5 * y).subject_to([c1, c2, c3]).solve(duals=True)
    assert abs(t1.objective_value - 36.0) <= 1e-12
    for con, want in ((c1, 0.0), (c2, 1.5), (c3, 1.0)):
        assert abs(t1.dual(con) - want) <= 1e-12
    assert abs(t1.reduced_cost(x)) <= 1e-12 and abs(t1.reduced_cost(y)) <= 1e-12
    assert t1.certificate.source == "fresh" and abs(t1.certificate.gap) <= 1e-12
    moved = dz.Maximize(3 * x + 5 * y).subject_to([c1, c2, 3 * x + 2 * y <= 18.5]).solve()
    assert abs((moved.objective_value - t1.objective_value) - 0.5 * t1.dual(c3)) <= 1e-12

    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    g1, g2 = x + y >= 4.0, x + 3 * y >= 6.0
    t2 = dz.Minimize(2 * x + 3 * y).subject_to([g1, g2]).solve(duals=True)
    assert abs(t2.objective_value - 9.0) <= 1e-12
    assert abs(t2.dual(g1) - 1.5) <= 1e-12 and abs(t2.dual(g2) - 0.5) <= 1e-12
    assert t2.certificate.source == "fresh" and abs(t2.certificate.gap) <= 1e-12
    assert abs(t2.certificate.primal_objective - 9.0) <= 1e-12

    x, y = dz.Variable.nonneg(), dz.Variable(lb=0.0, ub=2.0)
    eq = x + y == 3.0
    t3 = dz.Maximize(x + 2 * y).subject_to(eq).solve(duals=True)
    assert abs(t3.objective_value - 5.0) <= 1e-12
    assert abs(t3.dual(eq) - 1.0) <= 1e-12 and abs(t3.reduced_cost(y) - 1.0) <= 1e-12
    assert abs(t3._solution.duals.ub_dual[y.id] - 1.0) <= 1e-12
    assert t3.certificate.source == "fresh" and abs(t3.certificate.gap) <= 1e-12
    with pytest.raises(KeyError):
        t3.dual(g1)
    with pytest.raises(RuntimeError, match=r"solve\(duals=True\)"):
        dz.Maximize(x + 2 * y).subject_to(eq).solve().dual(eq)


# ------------------------------------------------------------------ 2, 3. STRICT is the reference
@functools.lru_cache(maxsize=None)
def _strict_set():
    """The LPs of tests 2 and 3 with the oracle's result and the reference duals of the optimal
    ones: (kind, a, b, c, CoreLP, oracle result, RefDuals or None), computed once."""
    data = [(kind,) + make_lp(seed, kind, 4, 48) for kind in (1, 2) for seed in range(200)]
    data += [(0,) + make_lp(seed, 0, 4, 48) for seed in range(40)]
    data += [(0,) + _family(3, 0, 128, 200), (0,) + _family(1, 0, 1, 3)]
    out = []
    for kind, a, b, c in data:
        sf = ora.stdform_from_dense(a, b, c)
        res = ora.simplex_solve(sf)
        ref = dref.core_duals(sf, res) if res.status == "optimal" else None
        out.append((kind, a, b, c, core.CoreLP.from_inequality_form(a, b, c), res, ref))
    return out


@functools.lru_cache(maxsize=None)
def _strict_batch():
    return core.solve_batch([item[4] for item in _strict_set()], duals=True, log_cap=1 << 12)


def test_strict_batch_duals_are_the_reference():
    items, got = _strict_set(), _strict_batch()
    plain = core.solve_batch([item[4] for item in items], log_cap=1 << 12)
    counts = {0: 0, 1: 0, 2: 0}
    for i, ((kind, a, b, c, lp, res, ref), g, p) in enumerate(zip(items, got, plain)):
        what = f"LP {i} (kind {kind}, {a.shape[0]} x {a.shape[1]})"
        assert_same_run(g, p, what)       # res is what dzg_batch_solve fills
        assert_same_run(g, res, what)     # ... which is the oracle's run
        if ref is None:
            assert g.duals is None, what
            continue
        counts[kind] += 1
        du = g.duals
        assert du.source == "fresh" and du.source_code == _ffi.DUALS_FRESH, what
        assert_bit_equal(du.y, ref.y, what + " y")
        assert_bit_equal(du.d, ref.d, what + " d")
        assert_bit_equal([du.dual_obj], [ref.dual_obj], what + " dual_obj")
        assert_bit_equal([du.primal_obj], [res.objective], what + " primal_obj")
        assert_bit_equal([du.primal_infeas, du.dual_infeas, du.z_diff],
                         [ref.primal_infeas, ref.dual_infeas, ref.z_diff], what + " scalars")
        assert (du.d[g.basis] == 0.0).all(), what
    assert counts[1] >= 20 and counts[2] >= 100 and counts[0] == 42, counts
    ms = [item[1].shape[0] for item in items if item[6] is not None]
    assert min(ms) == 1 and max(ms) == 128


def test_strict_handle_equals_the_batch():
    items, batch = _strict_set(), _strict_batch()
    checked = 0
    for i, ((kind, a, b, c, lp, res, ref), g) in enumerate(zip(items, batch)):
        if ref is None:
            continue
        what = f"LP {i} (kind {kind}, {a.shape[0]} x {a.shape[1]})"
        with core.Solver(lp, numerics=core.STRICT) as s:
            assert s.run(0) == "optimal", what
            du = s.duals()
        assert du.source == "fresh", what
        assert_bit_equal(du.y, g.duals.y, what + " y")
        assert_bit_equal(du.d, g.duals.d, what + " d")
        assert_bit_equal([du.primal_obj, du.dual_obj, du.primal_infeas, du.dual_infeas, du.z_diff],
                         [g.duals.primal_obj, g.duals.dual_obj, g.duals.primal_infeas,
                          g.duals.dual_infeas, g.duals.z_diff], what + " scalars")
        checked += 1
    assert checked >= 162
    # above the batch limit, inside AUTO's STRICT range
    a, b, c = _family(5, 0, 150, 260)
    sf = ora.stdform_from_dense(a, b, c)
    res = ora.simplex_solve(sf)
    assert res.status == "optimal"
    ref = dref.core_duals(sf, res)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c)) as s:
        assert s.run(0) == "optimal"
        r, du = s.result(log=False), s.duals()
    assert r.numerics == "strict" and r.basis.tolist() == res.basis.tolist()
    assert_bit_equal(du.y, ref.y, "150 x 260 y")
    assert_bit_equal(du.d, ref.d, "150 x 260 d")
    assert_bit_equal([du.dual_obj, du.primal_obj], [ref.dual_obj, res.objective], "150 x 260 objectives")
    # a solver that has not ended optimal has no duals
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), numerics=core.STRICT) as s:
        s.run(3)
        with pytest.raises(_ffi.DantzigAmdError, match="OPTIMAL"):
            s.duals()


# ------------------------------------------------------------------ 4. FAST, fresh values
def _metric(v, ref):
    v, ref = np.asarray(v, dtype=sc.LD), np.asarray(ref, dtype=sc.LD)
    return float(np.abs(v - ref).max(initial=0.0) / max(sc.LD(1), np.abs(ref).max(initial=0.0)))


def _same_state(r0, r1, what):
    assert r0.basis.tolist() == r1.basis.tolist() and r0.nonbasis.tolist() == r1.nonbasis.tolist(), what
    assert r0.iterations == r1.iterations and r0.status == r1.status, what
    for name in ("x", "xbar", "z", "zbar"):
        assert_bit_equal(getattr(r0, name), getattr(r1, name), f"{what} {name}")
    assert_bit_equal([r0.objective], [r1.objective], what + " objective")


@pytest.mark.parametrize("m,ns", [(97, 161), (601, 1203)])
def test_fast_fresh_duals_against_long_double(m, ns):
    a, b, c = _family(21, 0, m, ns)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=-1) as s:
        assert s.run(0) == "optimal"
        before = s.result(log=False)
        du = s.duals()
        after = s.result(log=False)
        again = s.duals()
    _same_state(before, after, f"{m} x {ns}: result() around duals()")
    assert du.source == "fresh"
    assert_bit_equal(du.y, again.y, "second call y")
    assert_bit_equal(du.d, again.d, "second call d")
    assert_bit_equal([du.primal_obj, du.dual_obj, du.primal_infeas, du.dual_infeas, du.z_diff],
                     [again.primal_obj, again.dual_obj, again.primal_infeas, again.dual_infeas,
                      again.z_diff], "second call scalars")
    assert_bit_equal([du.primal_obj], [before.objective], "primal_obj")
    assert (du.d[before.basis] == 0.0).all()

    # long-double values of the returned basis: z^ from state_check, y the same way
    ex = sc.exact_state(a, ns, lp, before.basis, before.nonbasis)
    codes = sc.var_codes(m + ns, ns)
    bm = sc.columns(a, m, codes[before.basis])
    call = np.asarray(lp.c, dtype=np.float64)
    y_hat = long_double_y(bm, call[before.basis])
    d_hat = ex.z
    # numpy's plain double solve of the same basis, priced in double: its error is what a backward
    # stable double-precision solve owes for this basis; the device applies a blocked LU as an
    # explicit inverse, a small multiple of that
    y_np = np.linalg.solve(bm.T, call[before.basis])
    d_np = sc.columns(a, m, codes[before.nonbasis]).T @ y_np - call[before.nonbasis]
    tol_y = max(C_DUALS * _metric(y_np, y_hat), 1e-13)
    tol_d = max(C_DUALS * _metric(d_np, d_hat), 1e-13)
    err_y, err_d = _metric(du.y, y_hat), _metric(du.d[before.nonbasis], d_hat)
    ratio_y = err_y / max(_metric(y_np, y_hat), 1e-13 / C_DUALS)
    ratio_d = err_d / max(_metric(d_np, d_hat), 1e-13 / C_DUALS)
    print(f"\n{m}x{ns}: k = {before.dense_columns}, pivots = {before.iterations}: y error {err_y:.3e} "
          f"(ratio {ratio_y:.3f}), d_N error {err_d:.3e} (ratio {ratio_d:.3f}), "
          f"gap {abs(du.primal_obj - du.dual_obj):.3e}, z_diff {du.z_diff:.3e}, "
          f"infeas {du.primal_infeas:.3e} / {du.dual_infeas:.3e}")
    assert err_y <= tol_y, (err_y, tol_y)
    assert err_d <= tol_d, (err_d, tol_d)
    # "the same tolerance": the test computes one per vector; the gap involves both sides (y through
    # rhs0 . y, the reduced costs through complementary slackness), so the larger of the two is meant
    tol_gap = max(tol_y, tol_d)
    assert abs(du.primal_obj - du.dual_obj) <= tol_gap * max(1.0, abs(du.primal_obj))
    assert du.primal_infeas <= 1e-9 and du.dual_infeas <= 1e-9


def test_fast_slack_optimum_and_missing_workspace():
    # c <= 0 with b >= 0: the slack basis is optimal, k = 0
    a, _, c = _family(22, 0, 40, 60)
    c = -np.abs(c)
    lp = core.CoreLP.from_inequality_form(a, np.ones(40), c)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=-1) as s:
        assert s.run(0) == "optimal"
        r, du = s.result(log=False), s.duals()
    assert r.iterations == 0 and r.dense_columns == 0 and du.source == "fresh"
    assert (du.y == 0.0).all()
    assert_bit_equal(du.d[:60], -c, "d = -c")
    assert (du.d[60:] == 0.0).all() and du.dual_obj == 0.0 and du.z_diff == 0.0
    # without the refactorisation workspace a FAST handle cannot recompute anything
    a, b, c = _family(23, 0, 30, 50)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), numerics=core.FAST, refactor_interval=0) as s:
        assert s.run(0) == "optimal"
        with pytest.raises(_ffi.DantzigAmdError, match="refactor_interval"):
            s.duals()
        out = _ffi.Duals()
        assert _ffi.lib().dzg_solver_duals(s._h, C.byref(out)) == _ffi.E_ARG
        assert _ffi.lib().dzg_solver_duals(s._h, None) == _ffi.E_ARG


# ------------------------------------------------------------------ 5. carried fallback
def test_csc_solver_returns_the_carried_values():
    m, ns = 200, 400
    col_ptr, row_idx, val, b, c = core.gen_sparse_lp(7, m, ns, 8)
    lp = core.CoreLP.from_csc(m, col_ptr, row_idx, val, b, c)
    with core.Solver(lp, numerics=core.FAST) as s:
        assert s.run(0) == "optimal"
        r, du = s.result(log=False), s.duals()
    assert du.source == "carried" and du.source_code == _ffi.DUALS_CARRIED and du.z_diff == 0.0
    assert_bit_equal(du.d[r.nonbasis], r.z, "d_N is the carried z")
    assert (du.d[r.basis] == 0.0).all()
    y = np.zeros(m)
    for k, var in enumerate(r.nonbasis):
        if var >= ns:
            y[var - ns] = r.z[k]
    assert_bit_equal(du.y, y, "y is the slack part of z")
    total = 0.0
    for i in range(m):
        total = total + float(b[i]) * float(y[i])
    assert_bit_equal([du.dual_obj, du.primal_obj], [total, r.objective], "objectives")


# ------------------------------------------------------------------ 6. solve_many(duals=True)
def test_solve_many_with_duals_equals_one_solve_per_model():
    rng = np.random.default_rng(78)
    items = [_random_problem(rng, int(rng.integers(0, 12))) for _ in range(24)]
    got = dz.solve_many([p for _, p in items], duals=True, return_exceptions=True)
    plain = dz.solve_many([p for _, p in items], return_exceptions=True)
    kinds = set()
    for i, ((vs, p), g, q) in enumerate(zip(items, got, plain)):
        assert type(g) is type(q), (i, g, q)
        try:
            w = p.solve(duals=True)
        except Exception as e:  # noqa: BLE001
            assert type(g) is type(e) and f"(model {i})" in str(g), (i, g, e)
            kinds.add(type(e).__name__)
            continue
        kinds.add("optimal")
        assert_bit_equal([g.objective_value, q.objective_value], [w.objective_value] * 2, f"model {i}")
        assert_bit_equal([g[v] for v in vs], [w[v] for v in vs], f"model {i} values")
        assert_bit_equal([g.dual(con) for con in p.constraints], [w.dual(con) for con in p.constraints],
                         f"model {i} duals")
        assert_bit_equal([g.reduced_cost(v) for v in vs], [w.reduced_cost(v) for v in vs],
                         f"model {i} reduced costs")
        cg, cw = g.certificate, w.certificate
        assert cg.source == cw.source == "fresh"
        assert_bit_equal([cg.primal_objective, cg.dual_objective, cg.gap, cg.primal_infeasibility,
                          cg.dual_infeasibility, cg.z_diff],
                         [cw.primal_objective, cw.dual_objective, cw.gap, cw.primal_infeasibility,
                          cw.dual_infeasibility, cw.z_diff], f"model {i} certificate")
        assert abs(cg.gap) <= 1e-9 * max(1.0, abs(cg.primal_objective))
    assert "optimal" in kinds and len(kinds) >= 2, kinds
