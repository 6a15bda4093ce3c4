"""Sensitivity ranging on the GPU (csrc/k_ranging.hip, dzg_solver_ranging, dzg_batch_solve_ranging,
solve(ranging=True)): STRICT is the reference's arithmetic bit for bit (tests/ranging_reference.py),
FAST is held to a multiple of LAPACK's own error against long-double endpoints, CSC solvers say that
they have no ranging.

FAST error ratios (device error / numpy's double-precision error, same metric, bound 32) an MI355X
shows per shape, as (cost, rhs), in C_RANGING_OBSERVED below; pytest -s prints them with the count
of skipped directions (a long-double delta within a factor 2 of pivot_tol).  The first run on the
gen_dense_lp shapes counted 0 skipped of 249 directions at 97x161 and 0 of 1 256 at 601x1203."""
import ctypes as C
import functools

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi, core, rust
from dantzig_amd.model import Constraint
from oracle import oracle as ora
from tests import ranging_reference as rref
from tests import state_check as sc
from tests.lp_families import make_lp
from tests.duals_helpers import (assert_bit_equal, assert_same_run, family as _family,
                                 random_problem as _random_problem)

pytestmark = pytest.mark.gpu

C_RANGING_OBSERVED = {"97x161": (2.263, 1.636), "601x1203": (1.227, 2.251)}
C_RANGING_SKIPPED_OBSERVED = {"97x161": 0, "601x1203": 0}
C_DUALS = 32.0
INF = float("inf")


# ------------------------------------------------------------------ 1. textbook, end to end
def _pair(r):
    return (r.lo, r.hi)


def _near(got, want, tol=1e-12):
    for g, w in zip(got, want):
        if np.isfinite(w):
            assert abs(g - w) <= tol, (got, want)
        else:
            assert g == w, (got, want)


def _moves(lo, hi, at):
    """Where the re-solve check moves a value to: the midpoint of each finite side, 1.0 along an
    infinite one."""
    return [at + (lo - at) / 2 if np.isfinite(lo) else at - 1.0, at + (hi - at) / 2 if np.isfinite(hi) else at + 1.0]


def _resolve_check(make, variables, tol):
    """make(b_shift={constraint index: t}, c_shift={variable index: t}) -> (problem, constraints):
    solves make({}, {}) with ranging; inside every range the optimal value of the moved model
    differs by t * dual (or t * value).  Returns the Solution."""
    problem, cons = make({}, {})
    sol = problem.solve(ranging=True)
    for i, con in enumerate(cons):
        rg = sol.rhs_range(con)
        b = con._signs[0] * con.rust_inequalities()[0]._b
        assert rg.lo <= b <= rg.hi
        for target in _moves(rg.lo, rg.hi, b):
            moved, _ = make({i: target - b}, {})
            got = moved.solve().objective_value - sol.objective_value
            assert abs(got - (target - b) * sol.dual(con)) <= tol, (i, target, got, sol.dual(con))
    coefs = problem.objective.linexpr.map_ids_to_coefs()
    for j, v in enumerate(variables):
        rg = sol.objective_range(v)
        cv = coefs.get(v.id, 0.0)
        assert rg.lo <= cv <= rg.hi
        for target in _moves(rg.lo, rg.hi, cv):
            moved, _ = make({}, {j: target - cv})
            got = moved.solve().objective_value - sol.objective_value
            assert abs(got - (target - cv) * sol[v]) <= tol, (j, target, got, sol[v])
    return sol


def test_textbook_models_end_to_end():
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    c1, c2, c3 = x <= 4.0, 2 * y <= 12.0, 3 * x + 2 * y <= 18.0
    t1 = dz.Maximize(3 * x + 5 * y).subject_to([c1, c2, c3]).solve(ranging=True)
    assert abs(t1.objective_value - 36.0) <= 1e-12
    _near(_pair(t1.objective_range(x)), (0.0, 7.5))
    _near(_pair(t1.objective_range(y)), (2.0, INF))
    _near(_pair(t1.rhs_range(c1)), (2.0, INF))
    _near(_pair(t1.rhs_range(c2)), (6.0, 18.0))
    _near(_pair(t1.rhs_range(c3)), (12.0, 24.0))
    assert abs(t1.dual(c2) - 1.5) <= 1e-12 and t1.certificate.source == "fresh"  # ranging implies duals
    with pytest.raises(KeyError):
        t1.rhs_range(x <= 9.0)
    with pytest.raises(KeyError):
        t1.objective_range(dz.Variable.nonneg())
    with pytest.raises(RuntimeError, match=r"solve\(ranging=True\)"):
        dz.Maximize(3 * x + 5 * y).subject_to([c1, c2, c3]).solve(duals=True).rhs_range(c1)

    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()

    def t2(bs, cs):
        cons = [x + y >= 4.0 + bs.get(0, 0.0), x + 3 * y >= 6.0 + bs.get(1, 0.0)]
        return dz.Minimize((2.0 + cs.get(0, 0.0)) * x + (3.0 + cs.get(1, 0.0)) * y).subject_to(cons), cons

    assert abs(_resolve_check(t2, [x, y], 1e-12).objective_value - 9.0) <= 1e-12

    x, y = dz.Variable.nonneg(), dz.Variable(lb=0.0, ub=2.0)

    def t3(bs, cs):
        cons = [x + y == 3.0 + bs.get(0, 0.0)]
        return dz.Maximize((1.0 + cs.get(0, 0.0)) * x + (2.0 + cs.get(1, 0.0)) * y).subject_to(cons), cons

    assert abs(_resolve_check(t3, [x, y], 1e-12).objective_value - 5.0) <= 1e-12


# ------------------------------------------------------------------ 2, 3. STRICT is the reference
def _directions(i, m, n, every=1):
    """LP i's request: every `every`-th variable's and every row's own direction, then three
    two-entry directions e_i - e_j of each kind where the LP has two indices to name."""
    rng = np.random.default_rng(5000 + i)
    cost = [{j: 1.0} for j in range(0, n, every)]
    rhs = [{r: 1.0} for r in range(m)]
    for _ in range(3):
        if n >= 2:
            a, b = rng.choice(n, 2, replace=False)
            cost.append({int(a): 1.0, int(b): -1.0})
        if m >= 2:
            a, b = rng.choice(m, 2, replace=False)
            rhs.append({int(a): 1.0, int(b): -1.0})
    return cost, rhs


@functools.lru_cache(maxsize=None)
def _strict_set():
    """The LPs of tests 2 and 3 (those of tests/test_gpu_duals.py) with the oracle's result, their
    directions and, for the optimal ones, the reference ranges: computed once."""
    data = [(kind,) + make_lp(seed, kind, 4, 48) for kind in (1, 2) for seed in range(200)]
    data += [(0,) + make_lp(seed, 0, 4, 48) for seed in range(40)]
    data += [(0,) + _family(3, 0, 128, 200), (0,) + _family(1, 0, 1, 3)]
    out = []
    for i, (kind, a, b, c) in enumerate(data):
        m, ns = a.shape
        sf = ora.stdform_from_dense(a, b, c)
        res = ora.simplex_solve(sf)
        cost, rhs = _directions(i, m, m + ns, every=8 if m == 128 else 1)
        ref = None
        if res.status == "optimal":
            rg = rref.CoreRanging(sf, res)
            ref = ([rg.cost(d) for d in cost], [rg.rhs(d) for d in rhs])
        out.append((kind, a, core.CoreLP.from_inequality_form(a, b, c), res, cost, rhs, ref))
    return out


@functools.lru_cache(maxsize=None)
def _strict_batch():
    items = _strict_set()
    return core.solve_batch([item[2] for item in items], ranging=[(item[4], item[5]) for item in items],
                            log_cap=1 << 12)


def _assert_ranges(lo, hi, lo_var, hi_var, want, what):
    assert_bit_equal(lo, [w.lo for w in want], what + " lo")
    assert_bit_equal(hi, [w.hi for w in want], what + " hi")
    assert np.asarray(lo_var).tolist() == [w.lo_var for w in want], what + " lo_var"
    assert np.asarray(hi_var).tolist() == [w.hi_var for w in want], what + " hi_var"


def _assert_same_duals(got, want, what):
    assert got.source == want.source, what
    assert_bit_equal(got.y, want.y, what + " y")
    assert_bit_equal(got.d, want.d, what + " d")
    assert_bit_equal([got.primal_obj, got.dual_obj, got.primal_infeas, got.dual_infeas, got.z_diff],
                     [want.primal_obj, want.dual_obj, want.primal_infeas, want.dual_infeas, want.z_diff],
                     what + " scalars")


def test_strict_batch_ranging_is_the_reference():
    items, got = _strict_set(), _strict_batch()
    plain = core.solve_batch([item[2] for item in items], duals=True, log_cap=1 << 12)
    optimal, ms, finite = 0, [], 0
    for i, ((kind, a, lp, res, cost, rhs, ref), g, p) in enumerate(zip(items, got, plain)):
        what = f"LP {i} (kind {kind}, {a.shape[0]} x {a.shape[1]})"
        assert_same_run(g, p, what)      # res is what dzg_batch_solve_duals fills
        if ref is None:
            assert g.ranging is None and g.duals is None and p.duals is None, what
            continue
        _assert_same_duals(g.duals, p.duals, what)
        optimal += 1
        ms.append(a.shape[0])
        r = g.ranging
        _assert_ranges(r.cost_lo, r.cost_hi, r.cost_lo_var, r.cost_hi_var, ref[0], what + " cost")
        _assert_ranges(r.rhs_lo, r.rhs_hi, r.rhs_lo_var, r.rhs_hi_var, ref[1], what + " rhs")
        assert (r.cost_lo <= 0.0).all() and (r.cost_hi >= 0.0).all(), what
        assert (r.rhs_lo <= 0.0).all() and (r.rhs_hi >= 0.0).all(), what
        finite += int(np.isfinite(r.cost_lo).sum() + np.isfinite(r.rhs_hi).sum())
    assert optimal >= 100 and min(ms) == 1 and max(ms) == 128, (optimal, ms)
    assert finite >= 1000


def test_non_optimal_lps_get_nan_ranges():
    # the C contract underneath `ranging is None`: NaN ranges and -1 for an LP that did not end OPTIMAL
    items = _strict_set()
    i = next(k for k, item in enumerate(items) if item[3].status != "optimal")
    kind, a, lp, res, cost, rhs, ref = items[i]
    buf = _ffi.RangingBuffers(cost, rhs)
    buf.lo[0][:] = 7.0
    buf.lo_var[1][:] = 7
    req, out = _ffi.RangingReq(), _ffi.Ranging()
    buf.fill(req, out)
    c_lp, keep = core._c_lp(lp)
    r = _ffi.Result()
    rc = _ffi.lib().dzg_batch_solve_ranging(C.byref(c_lp), C.c_int64(1), None, C.c_int64(0), C.byref(req),
                                            C.byref(r), None, C.byref(out))
    assert rc == 0 and _ffi.status_str(r.status) == res.status
    for side in (0, 1):
        lo, hi, lo_var, hi_var = buf.side(side)
        assert np.isnan(lo).all() and np.isnan(hi).all()
        assert (lo_var == -1).all() and (hi_var == -1).all()


def test_strict_handle_equals_the_batch():
    items, batch = _strict_set(), _strict_batch()
    optimal = [i for i, item in enumerate(items) if item[6] is not None]
    for i in optimal[::10]:
        kind, a, lp, res, cost, rhs, ref = items[i]
        what = f"LP {i} (kind {kind}, {a.shape[0]} x {a.shape[1]})"
        with core.Solver(lp, numerics=core.STRICT) as s:
            assert s.run(0) == "optimal", what
            r = s.ranging(cost, rhs)
        g = batch[i].ranging
        for name in ("cost_lo", "cost_hi", "rhs_lo", "rhs_hi"):
            assert_bit_equal(getattr(r, name), getattr(g, name), f"{what} {name}")
        for name in ("cost_lo_var", "cost_hi_var", "rhs_lo_var", "rhs_hi_var"):
            assert getattr(r, name).tolist() == getattr(g, name).tolist(), f"{what} {name}"
        _assert_same_duals(r.duals, batch[i].duals, what)
    assert len(optimal[::10]) >= 10
    # above the batch limit, inside AUTO's STRICT range: against the reference
    a, b, c = _family(5, 0, 150, 260)
    sf = ora.stdform_from_dense(a, b, c)
    res = ora.simplex_solve(sf)
    assert res.status == "optimal"
    rng = np.random.default_rng(9)
    cost = [{int(j): 1.0} for j in rng.choice(410, 13, replace=False)]
    rhs = [{int(r): 1.0} for r in rng.choice(150, 13, replace=False)]
    for _ in range(3):
        i, j = rng.choice(410, 2, replace=False)
        cost.append({int(i): 1.0, int(j): -1.0})
        i, j = rng.choice(150, 2, replace=False)
        rhs.append({int(i): 1.0, int(j): -1.0})
    rg = rref.CoreRanging(sf, res)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c)) as s:
        assert s.run(0) == "optimal"
        before = s.result(log=False)
        r = s.ranging(cost, rhs)
        after = s.result(log=False)
    assert before.numerics == "strict" and before.basis.tolist() == res.basis.tolist()
    _same_state(before, after, "150 x 260: result() around ranging()")
    _assert_ranges(r.cost_lo, r.cost_hi, r.cost_lo_var, r.cost_hi_var, [rg.cost(d) for d in cost], "150 x 260 cost")
    _assert_ranges(r.rhs_lo, r.rhs_hi, r.rhs_lo_var, r.rhs_hi_var, [rg.rhs(d) for d in rhs], "150 x 260 rhs")
    # a solver that has not ended optimal has no ranges
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), numerics=core.STRICT) as s:
        s.run(3)
        with pytest.raises(_ffi.DantzigAmdError, match="OPTIMAL"):
            s.ranging(cost, rhs)


# ------------------------------------------------------------------ 4. FAST against long double
def _same_state(r0, r1, what):
    assert r0.basis.tolist() == r1.basis.tolist() and r0.nonbasis.tolist() == r1.nonbasis.tolist(), what
    assert r0.iterations == r1.iterations and r0.status == r1.status, what
    for name in ("x", "xbar", "z", "zbar"):
        assert_bit_equal(getattr(r0, name), getattr(r1, name), f"{what} {name}")
    assert_bit_equal([r0.objective], [r1.objective], what + " objective")


def _endpoint_error(got_lo, got_hi, want, skip, what):
    """max |t - t^| / max(1, |t^|) over the finite endpoints of the directions not skipped; infinite
    and finite must agree exactly."""
    worst = 0.0
    for i, w in enumerate(want):
        if skip[i]:
            continue
        for g, t in ((got_lo[i], w.lo), (got_hi[i], w.hi)):
            assert np.isfinite(g) == np.isfinite(t), (what, i, g, t)
            if np.isfinite(t):
                worst = max(worst, abs(g - t) / max(1.0, abs(t)))
            else:
                assert g == t, (what, i, g, t)
    return worst


@pytest.mark.parametrize("m,ns", [(97, 161), (601, 1203)])
def test_fast_ranging_against_long_double(m, ns):
    a, b, c = _family(21, 0, m, ns)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    n = m + ns
    with core.Solver(lp, numerics=core.FAST, refactor_interval=-1) as s:
        assert s.run(0) == "optimal"
        before = s.result(log=False)
        rng = np.random.default_rng(m)
        basic_struct = [int(j) for j in before.basis if j < ns]
        assert len(basic_struct) == before.dense_columns
        cost = [{j: 1.0} for j in basic_struct]
        cost += [{int(j): 1.0} for j in rng.choice(before.nonbasis, 32, replace=False)]
        rhs = [{r: 1.0} for r in range(m)]
        for _ in range(16):
            i, j = rng.choice(n, 2, replace=False)
            cost.append({int(i): 1.0, int(j): -1.0})
            i, j = rng.choice(m, 2, replace=False)
            rhs.append({int(i): 1.0, int(j): -1.0})
        r = s.ranging(cost, rhs)
        after = s.result(log=False)
        again = s.ranging(cost, rhs)
        du = s.duals()
    _same_state(before, after, f"{m} x {ns}: result() around ranging()")
    for name in ("cost_lo", "cost_hi", "rhs_lo", "rhs_hi"):
        assert_bit_equal(getattr(r, name), getattr(again, name), f"second call {name}")
    for name in ("cost_lo_var", "cost_hi_var", "rhs_lo_var", "rhs_hi_var"):
        assert getattr(r, name).tolist() == getattr(again, name).tolist(), f"second call {name}"
    _assert_same_duals(r.duals, du, "the duals of ranging() and of duals()")
    assert (r.cost_lo <= 0.0).all() and (r.cost_hi >= 0.0).all()
    assert (r.rhs_lo <= 0.0).all() and (r.rhs_hi >= 0.0).all()

    # long-double endpoints of the returned basis by the same rule: the device's own carried x, the
    # long-double d; numpy's plain double solve of the same basis is the yardstick
    ex = sc.exact_state(a, ns, lp, before.basis, before.nonbasis)
    codes = sc.var_codes(n, ns)
    bm = sc.columns(a, m, codes[before.basis])
    nm = sc.columns(a, m, codes[before.nonbasis])
    unit_rows = np.where(codes[before.nonbasis] < 0, -1 - codes[before.nonbasis], -1)
    want_c, want_r, near_c, near_r = rref.ranges_from_inverse(
        rref.refined_inverse(bm), nm, unit_rows, before.basis, before.nonbasis, before.x, ex.z, cost, rhs)
    call = np.asarray(lp.c, dtype=np.float64)
    inv_np = np.linalg.solve(bm, np.eye(m))
    d_np = nm.T @ np.linalg.solve(bm.T, call[before.basis]) - call[before.nonbasis]
    np_c, np_r, _, _ = rref.ranges_from_inverse(inv_np, nm, unit_rows, before.basis, before.nonbasis,
                                                before.x, d_np, cost, rhs)
    skipped = int(np.sum(near_c) + np.sum(near_r))
    assert skipped <= 0.02 * (len(cost) + len(rhs)), (skipped, len(cost), len(rhs))
    err_c = _endpoint_error(r.cost_lo, r.cost_hi, want_c, near_c, "cost")
    err_r = _endpoint_error(r.rhs_lo, r.rhs_hi, want_r, near_r, "rhs")
    yard_c = _endpoint_error([w.lo for w in np_c], [w.hi for w in np_c], want_c, near_c, "numpy cost")
    yard_r = _endpoint_error([w.lo for w in np_r], [w.hi for w in np_r], want_r, near_r, "numpy rhs")
    tol_c, tol_r = max(C_DUALS * yard_c, 1e-13), max(C_DUALS * yard_r, 1e-13)
    ratio_c = err_c / max(yard_c, 1e-13 / C_DUALS)
    ratio_r = err_r / max(yard_r, 1e-13 / C_DUALS)
    print(f"\n{m}x{ns}: k = {before.dense_columns}, {len(cost)} cost + {len(rhs)} rhs directions, "
          f"{skipped} skipped (a delta within a factor 2 of pivot_tol): cost error {err_c:.3e} "
          f"(ratio {ratio_c:.3f}), rhs error {err_r:.3e} (ratio {ratio_r:.3f})")
    assert err_c <= tol_c, (err_c, tol_c)
    assert err_r <= tol_r, (err_r, tol_r)


# ------------------------------------------------------------------ 5. edges
def test_slack_optimum_missing_workspace_and_csc():
    # c <= 0 with b >= 0: the slack basis is optimal, k = 0
    a, _, c = _family(22, 0, 40, 60)
    c = -np.abs(c)
    lp = core.CoreLP.from_inequality_form(a, np.ones(40), c)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=-1) as s:
        assert s.run(0) == "optimal"
        res, r = s.result(log=False), s.ranging([{j: 1.0} for j in range(60)], None)
    assert res.iterations == 0 and res.dense_columns == 0
    # structural j is nonbasic with delta = -1: t in (-inf, d_j];  row i's slack is basic at position
    # i with delta = +1: t in [-x_i, +inf)
    assert (r.cost_lo == -INF).all() and (r.cost_lo_var == -1).all()
    assert_bit_equal(r.cost_hi, r.duals.d[:60], "cost hi = d_j")
    assert r.cost_hi_var.tolist() == list(range(60))
    assert (r.rhs_hi == INF).all() and (r.rhs_hi_var == -1).all()
    assert_bit_equal(r.rhs_lo, -res.x, "rhs lo = -x_i")
    assert r.rhs_lo_var.tolist() == res.basis.tolist()
    # without the refactorisation workspace a FAST handle cannot recompute anything
    a, b, c = _family(23, 0, 30, 50)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), numerics=core.FAST, refactor_interval=0) as s:
        assert s.run(0) == "optimal"
        with pytest.raises(_ffi.DantzigAmdError, match="refactor_interval"):
            s.ranging()
        buf = _ffi.RangingBuffers([{0: 1.0}], [{0: 1.0}])
        req, out = _ffi.RangingReq(), _ffi.Ranging()
        buf.fill(req, out)
        assert _ffi.lib().dzg_solver_ranging(s._h, C.byref(req), None, C.byref(out)) == _ffi.E_ARG
        assert "refactor_interval" in _ffi.lib().dzg_last_error().decode()
        assert _ffi.lib().dzg_solver_ranging(s._h, None, None, C.byref(out)) == _ffi.E_ARG
        assert _ffi.lib().dzg_solver_ranging(s._h, C.byref(req), None, None) == _ffi.E_ARG
    # CSC storage: no ranging, and no carried stand-in
    m, ns = 200, 400
    col_ptr, row_idx, val, b, c = core.gen_sparse_lp(7, m, ns, 8)
    with core.Solver(core.CoreLP.from_csc(m, col_ptr, row_idx, val, b, c), numerics=core.FAST) as s:
        assert s.run(0) == "optimal"
        assert _ffi.lib().dzg_solver_ranging(s._h, C.byref(req), None, C.byref(out)) == _ffi.E_ARG
        assert "ranging is not supported" in _ffi.lib().dzg_last_error().decode()
        with pytest.raises(NotImplementedError, match="not supported"):
            s.ranging([{0: 1.0}], [{0: 1.0}])
        assert s.duals().source == "carried"  # (what duals() still gives there)


# ------------------------------------------------------------------ 6. solve_many(ranging=True)
def _rebuild(vs, p, b_shift=None, c_shift=None):
    """The model p with one constraint's b or one variable's objective coefficient moved."""
    cons = []
    for i, con in enumerate(p.constraints):
        rows = con.rust_inequalities()
        t = b_shift[1] if b_shift and b_shift[0] == i else 0.0
        # the rows as lowered: linexpr <= b; the user's b moves by t, a negated row's by -t
        cons.append(Constraint(inequalities=[rust.PyInequality(linexpr=row._linexpr, b=row._b + sign * t)
                                                for row, sign in zip(rows, con._signs)], signs=list(con._signs)))
    objective = p.objective
    if c_shift:
        objective = (objective + c_shift[1] * vs[c_shift[0]]).to_affexpr()
    return type(p)(objective).subject_to(cons)


def _midpoint_step(end, at):
    """The step from `at` to the midpoint of [at, end], cut towards zero to a multiple of 2^-16.  The
    re-solve check holds at every point inside a range; the cut keeps the moved data short.  The
    reference's algorithm has no anti-cycling rule, and ties that a last-bit perturbation splits make
    it stall: with b = -1.4999999999999998 (half of a lower end computed as -2.9999999999999996) one
    of these models runs into the iteration limit on the CPU oracle as well, with b = -1.5 it takes
    three pivots."""
    return float(np.trunc((end - at) / 2 * 65536.0) / 65536.0)


def test_solve_many_with_ranging_equals_one_solve_per_model():
    rng = np.random.default_rng(78)
    items = [_random_problem(rng, int(rng.integers(0, 12))) for _ in range(24)]
    got = dz.solve_many([p for _, p in items], ranging=True, return_exceptions=True)
    plain = dz.solve_many([p for _, p in items], return_exceptions=True)
    kinds, checks, dropped = set(), [], 0
    for i, ((vs, p), g, q) in enumerate(zip(items, got, plain)):
        assert type(g) is type(q), (i, g, q)
        try:
            w = p.solve(ranging=True)
        except Exception as e:  # noqa: BLE001
            assert type(g) is type(e) and f"(model {i})" in str(g), (i, g, e)
            kinds.add(type(e).__name__)
            continue
        kinds.add("optimal")
        assert_bit_equal([g.objective_value, q.objective_value], [w.objective_value] * 2, f"model {i}")
        assert_bit_equal([g[v] for v in vs], [w[v] for v in vs], f"model {i} values")
        assert_bit_equal([g.dual(con) for con in p.constraints], [w.dual(con) for con in p.constraints],
                         f"model {i} duals")
        used = [v for v in vs if v.id in g._solution.ranging.var_lo]
        for name, ours, theirs in (("rhs", [g.rhs_range(con) for con in p.constraints],
                                    [w.rhs_range(con) for con in p.constraints]),
                                   ("objective", [g.objective_range(v) for v in used],
                                    [w.objective_range(v) for v in used])):
            assert_bit_equal([r.lo for r in ours], [r.lo for r in theirs], f"model {i} {name} lo")
            assert_bit_equal([r.hi for r in ours], [r.hi for r in theirs], f"model {i} {name} hi")
        # inside every range the same basis stays optimal: the optimal value moves along the slope
        tol = 1e-9 * max(1.0, abs(g.objective_value))
        coefs = p.objective.linexpr.map_ids_to_coefs()
        first = {}
        for ci, con in enumerate(p.constraints):
            if first.setdefault(id(con), ci) != ci:
                continue  # (a constraint listed twice moves both of its copies: not this check)
            rg, bval = g.rhs_range(con), con._signs[0] * con.rust_inequalities()[0]._b
            assert rg.lo <= bval <= rg.hi, (i, ci, rg, bval)
            for end in (rg.lo, rg.hi):
                t = _midpoint_step(end, bval) if np.isfinite(end) else 0.0
                dropped += int(np.isfinite(end) and end != bval and t == 0.0)
                if t != 0.0:
                    checks.append((_rebuild(vs, p, b_shift=(ci, t)), g.objective_value, t * g.dual(con), tol,
                                   (i, "b", ci, t)))
        for vi, v in enumerate(vs):
            if v not in used:
                continue
            rg, cval = g.objective_range(v), coefs.get(v.id, 0.0)
            assert rg.lo <= cval <= rg.hi, (i, vi, rg, cval)
            for end in (rg.lo, rg.hi):
                t = _midpoint_step(end, cval) if np.isfinite(end) else 0.0
                dropped += int(np.isfinite(end) and end != cval and t == 0.0)
                if t != 0.0:
                    checks.append((_rebuild(vs, p, c_shift=(vi, t)), g.objective_value, t * g[v], tol,
                                   (i, "c", vi, t)))
    assert "optimal" in kinds and len(kinds) >= 2, kinds
    # every finite side of nonzero width is checked: none is so narrow that its cut step is 0 (a side
    # of width 0 has its midpoint at the current value, where there is nothing to re-solve)
    assert dropped == 0, dropped
    assert len(checks) >= 20
    saved = dict(rust._options)
    rust.set_options(**{**saved, "max_iter": 100000})  # (a moved model that cycled would say so at once)
    try:
        moved = dz.solve_many([c[0] for c in checks], return_exceptions=True)
    finally:
        rust.set_options(**saved)
    for (_, base, slope, tol, what), sol in zip(checks, moved):
        assert not isinstance(sol, Exception), (what, sol)
        assert abs((sol.objective_value - base) - slope) <= tol, (what, sol.objective_value, base, slope)
