"""Re-optimisation from the current basis on the GPU (csrc/k_restart.hip, dzg_solver_reoptimize,
core.Solver.reoptimize, Optimize.session).

STRICT: the restart state is the CPU oracle's lu_solve / neg_t_dot bit for bit, and the pivots that
follow are the oracle's from that state.  FAST: the restart state is held to C_RESTART against the
state the basis defines for the changed LP in long double (tests/reopt_check.py), at the kernels'
edges: odd and even k, k = 0, both iteration forms, the 64-lane instantiation.  Inside the ranges of
Solver.ranging() nothing pivots and the objective moves by the duals; beyond them the run ends at an
optimum that passes the independent certificate; the statuses follow the data through infeasible
and unbounded steps; duals and drift speak about the new LP; the call is reproducible."""
import functools

import numpy as np
import pytest

from dantzig_amd import _ffi, core
from dantzig_amd import rust as rs
from oracle import oracle as ora
from tests import duals_reference as dref
from tests import reopt_check as rc
from tests import state_check as sc
from tests.duals_helpers import assert_bit_equal
from tests.optimality import certificate
from tests.test_reopt_host import CHANGES, _kat
from tests.test_surface import build_problem

pytestmark = pytest.mark.gpu

FAST_OPTS = dict(numerics=core.FAST, refactor_interval=-1)


@functools.lru_cache(maxsize=None)
def _g1(seed, m, ns):
    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    return np.ascontiguousarray(a), b, c


def _full(c, m):
    return np.concatenate([c, np.zeros(m)])


def _kat_lp(name):
    """A KAT model lowered to a CoreLP: bound rows, split free variables, var_col not the benchmark's."""
    _, problem = build_problem(_kat(name))
    arrays, _ = rs.lower(problem._core_objective().to_rust_affexpr(), list(problem.yield_rust_inequalities()))
    f = rs.standard_form(arrays)
    return f, core.CoreLP(a=f.a, c=f.c, basis=f.basis, nonbasis=f.nonbasis, x=f.x, z=f.z, var_col=f.var_col,
                          constant=f.constant)


# ------------------------------------------------------------------ 1, 2. STRICT: the oracle's bits
def _strict_restart_and_continuation(lp, a, ns, var_col, b2, c2, what):
    m = lp.m
    codes = sc.var_codes(lp.n, ns, var_col)
    with core.Solver(lp, numerics=core.STRICT) as s:
        assert s.run(0) == "optimal", what
        r0 = s.result()
        s.reoptimize(b=b2, c=c2)
        r1 = s.result()
        assert (r1.status, r1.iterations) == ("running", r0.iterations), what
        assert r1.basis.tolist() == r0.basis.tolist() and r1.nonbasis.tolist() == r0.nonbasis.tolist(), what
        # 1. the restart state
        bmat = sc.columns(a, m, codes[r1.basis])
        assert_bit_equal(r1.x, ora.lu_solve(bmat, b2), what + " x")
        sf = sc.stdform(a, ns, c2, r1, var_col)
        sf.constant = float(lp.constant)
        assert_bit_equal(r1.z, dref.core_duals(sf, r1).d[r1.nonbasis], what + " z")
        assert (r1.xbar == 1.0).all() and (r1.zbar == 1.0).all(), what
        # 2. the continuation: the oracle from that state
        want = ora.simplex_solve(sf, xbar=r1.xbar, zbar=r1.zbar)
        status = s.run(0)
        r2 = s.result()
    new = r2.pivots[r0.iterations:]
    print(f"{what}: {r0.iterations} pivots cold, {len(new)} after the change, {status}")
    assert status == want.status and r2.iterations == r0.iterations + want.iterations, what
    assert [p[:3] for p in new] == [tuple(int(v) for v in p[:3]) for p in want.pivots], what
    assert_bit_equal([p[3] for p in new], [p[3] for p in want.pivots], what + " mu")
    assert_bit_equal([r2.objective], [want.objective], what + " objective")
    assert r2.basis.tolist() == want.basis.tolist(), what
    return len(new)


def test_strict_restart_state_and_continuation_are_the_oracles():
    m, ns = 24, 40
    a, b, c = _g1(31, m, ns)
    b2, c2 = rc.moved(1, b, c)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    moved = _strict_restart_and_continuation(lp, a, ns, None, b2, _full(c2, m), "G1 24x40")
    assert moved > 0, "the change does not leave the range: the continuation tests nothing"


def test_strict_restart_on_a_model_with_bound_rows():
    f, lp = _kat_lp("non_standard_variables")
    # bound rows below the user rows, the free variable split in two: var_col comes from the builder
    assert f.m == 7 and f.n_struct == 6 and len(f.var_col) == f.n
    rng = np.random.default_rng(5)
    b2 = f.x + 0.5 * rng.random(f.m)
    c2 = f.c - np.where(f.var_col >= 0, 0.5 * rng.random(f.n), 0.0)
    _strict_restart_and_continuation(lp, f.a, f.n_struct, f.var_col, b2, c2, "KAT non_standard_variables")


# ------------------------------------------------------------------ 3. FAST: the restart state
def _fast_restart_drift(a, b, c, seed, what, stop_at=None, **opts):
    """reoptimize(b', c') on a FAST solver stopped after `stop_at` pivots (None: at the optimum, 0:
    before any run): (result after the call, D's parts)."""
    m, ns = a.shape
    b2, c2 = rc.moved(seed, b, c)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), **FAST_OPTS, **opts) as s:
        if stop_at is None:
            assert s.run(0) == "optimal", what
        elif stop_at > 0:
            assert s.run(stop_at) == "iter_limit", what
        before = s.result(log=False)
        s.reoptimize(b=b2, c=_full(c2, m))
        r = s.result(log=False)
    assert (r.status, r.iterations) == ("running", before.iterations), what
    assert r.basis.tolist() == before.basis.tolist() and r.dense_columns == before.dense_columns, what
    assert (r.xbar == 1.0).all() and (r.zbar == 1.0).all(), what
    assert r.state_drift == 0.0, what
    ex = sc.exact_state(a, ns, rc.slack_start(a, b2, c2), r.basis, r.nonbasis)
    d = rc.restart_drift(ex, r)
    print(f"{what}: k = {r.dense_columns}, D = {d['D']:.3e} (x {d['x']:.3e}, z {d['z']:.3e}), "
          f"helper error {max(ex.err['x'], ex.err['z']):.1e}")
    assert max(ex.err["x"], ex.err["z"]) * 1e2 <= rc.C_RESTART, (what, ex.err)
    assert d["D"] <= rc.C_RESTART, (what, d)
    return r, d


def _stops_with_odd_and_even_k(a, b, c):
    """Pivot counts at which a FAST solve of the LP holds an odd and an even k > 0."""
    found = {}
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), **FAST_OPTS) as s:
        for p in range(1, 60):
            if s.run(1) != "iter_limit":
                break
            k = s.result(log=False).dense_columns
            if k > 0:
                found.setdefault(k % 2, p)
            if len(found) == 2:
                break
    assert len(found) == 2, found
    return found[1], found[0]


def test_fast_restart_state_at_odd_even_and_zero_k():
    a, b, c = _g1(41, 37, 53)
    odd, even = _stops_with_odd_and_even_k(a, b, c)
    r, _ = _fast_restart_drift(a, b, c, 2, "37x53 odd k", stop_at=odd)
    assert r.dense_columns % 2 == 1
    r, _ = _fast_restart_drift(a, b, c, 3, "37x53 even k", stop_at=even)
    assert r.dense_columns % 2 == 0 and r.dense_columns > 0
    r, d = _fast_restart_drift(a, b, c, 4, "37x53 slack basis", stop_at=0)
    assert r.dense_columns == 0 and r.iterations == 0
    # the basis is all slack: x = b' and z = -c', exactly
    b2, c2 = rc.moved(4, b, c)
    assert_bit_equal(r.x, b2, "x = b'")
    assert_bit_equal(r.z, -c2, "z = -c'")


@pytest.mark.parametrize("seven", [0, 1], ids=["three launches", "seven launches"])
def test_fast_restart_state_at_the_optimum_300x500(seven):
    a, b, c = _g1(42, 300, 500)
    r, _ = _fast_restart_drift(a, b, c, 5, f"300x500 seven_launches={seven}", seven_launches=seven)
    assert 0 < r.dense_columns <= 512


def test_fast_restart_state_with_the_64_lane_rows_640x1280():
    a, b, c = _g1(43, 640, 1280)
    r, _ = _fast_restart_drift(a, b, c, 6, "640x1280")
    assert r.dense_columns > 512, "the 64-lane instantiation of k_restart_x did not run"


# ------------------------------------------------------------------ 4. inside the range nothing pivots
@pytest.mark.parametrize("numerics,m,ns", [(core.FAST, 300, 500), (core.STRICT, 24, 40)], ids=["fast", "strict"])
def test_inside_the_range_nothing_pivots(numerics, m, ns):
    a, b, c = _g1(44, m, ns)
    cf = _full(c, m)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), numerics=numerics, refactor_interval=-1) as s:
        assert s.run(0) == "optimal"
        rg = s.ranging()
        r0 = s.result(log=False)
        old = r0.objective
        tol = 1e-9 * max(1.0, abs(old))
        rows = [i for i in range(m) if np.isfinite(rg.rhs_hi[i]) and abs(rg.rhs_hi[i]) > 1e-6]
        cols = [j for j in range(m + ns) if np.isfinite(rg.cost_hi[j]) and abs(rg.cost_hi[j]) > 1e-6]
        assert len(rows) >= 4 and len(cols) >= 4, (len(rows), len(cols))
        value = np.zeros(m + ns)
        value[r0.basis] = r0.x
        for i in rows[:4]:
            t = 0.5 * rg.rhs_hi[i]
            b2 = b.copy()
            b2[i] += t
            s.reoptimize(b=b2, c=cf)
            assert s.run(0) == "optimal"
            r = s.result(log=False)
            assert r.iterations == r0.iterations and r.basis.tolist() == r0.basis.tolist(), ("row", i, t)
            assert abs(r.objective - (old + t * rg.duals.y[i])) <= tol, ("row", i, t, r.objective, old)
        for j in cols[:4]:
            t = 0.5 * rg.cost_hi[j]
            c2 = cf.copy()
            c2[j] += t
            s.reoptimize(b=b, c=c2)
            assert s.run(0) == "optimal"
            r = s.result(log=False)
            assert r.iterations == r0.iterations and r.basis.tolist() == r0.basis.tolist(), ("variable", j, t)
            assert abs(r.objective - (old + t * value[j])) <= tol, ("variable", j, t, r.objective, old)


# ------------------------------------------------------------------ 5, 7. beyond the range it re-solves
@pytest.mark.parametrize("single", [False, True], ids=["all rows", "one row"])
@pytest.mark.parametrize("numerics,m,ns", [(core.FAST, 300, 500), (core.STRICT, 24, 40)], ids=["fast", "strict"])
def test_beyond_the_range_it_resolves_and_post_solve_follows(numerics, m, ns, single):
    a, b, c = _g1(45, m, ns)
    b2, c2 = rc.moved(7, b, c, rows=[m // 2] if single else None, cols=[ns // 3] if single else None)
    opts = dict(numerics=numerics, refactor_interval=-1)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), **opts) as s:
        assert s.run(0) == "optimal"
        cold_pivots = s.result(log=False).iterations
        s.reoptimize(b=b2, c=_full(c2, m))
        assert s.run(0) == "optimal"
        r = s.result(log=False)
        cert = certificate(a, b2, c2, r.basis)
        scale = max(1.0, abs(cert["primal_obj"]))
        print(f"{m}x{ns} {'one row' if single else 'all rows'}: {cold_pivots} pivots cold, "
              f"{r.iterations - cold_pivots} after the change")
        assert cert["primal_infeas"] <= 1e-9 and cert["dual_infeas"] <= 1e-9, cert
        assert abs(cert["primal_obj"] - cert["dual_obj"]) <= 1e-9 * scale, cert
        assert abs(r.objective - cert["primal_obj"]) <= 1e-9 * scale, (r.objective, cert)
        # 7. duals, and the drift measurement, speak about the new LP
        du = s.duals()
        assert abs(du.primal_obj - du.dual_obj) <= 1e-9 * scale, (du.primal_obj, du.dual_obj)
        with core.Solver(core.CoreLP.from_inequality_form(a, b2, c2), **opts) as cold:
            assert cold.run(0) == "optimal"
            assert abs(cold.duals().dual_obj - du.dual_obj) <= 1e-9 * scale
        if numerics == core.FAST:
            s.refactor()
            assert s.result(log=False).state_drift == 0.0


# ------------------------------------------------------------------ 6. other ends
@pytest.mark.parametrize("numerics", [core.STRICT, core.FAST], ids=["strict", "fast"])
def test_statuses_follow_the_data(numerics):
    opts = dict(numerics=numerics, refactor_interval=-1)
    # x1 + 2 x2 <= 4, 3 x1 + x2 >= 1: feasible -> x1 + 2 x2 <= 1, 3 x1 + x2 >= 6: infeasible -> back
    a = np.array([[1.0, 2.0], [-3.0, -1.0]])
    b, c = np.array([4.0, -1.0]), np.array([-1.0, -0.5])
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), **opts) as s:
        assert s.run(0) == "optimal"
        s.reoptimize(b=np.array([1.0, -6.0]))
        assert s.run(0) == "infeasible"
        ray = s.ray()
        assert ray.kind == "farkas" and ray.proven
        s.reoptimize(b=b)
        assert s.run(0) == "optimal"
        r = s.result(log=False)
        cert = certificate(a, b, c, r.basis)
        assert cert["primal_infeas"] <= 1e-9 and cert["dual_infeas"] <= 1e-9
        assert abs(r.objective + 1.0 / 3.0) <= 1e-9 and abs(cert["primal_obj"] + 1.0 / 3.0) <= 1e-9
    # x1 - x2 <= 2, x2 - x1 <= 3: bounded for c = (1, -2), unbounded along (1, 1) for c = (1, 1)
    a = np.array([[1.0, -1.0], [-1.0, 1.0]])
    b, c = np.array([2.0, 3.0]), np.array([1.0, -2.0])
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), **opts) as s:
        assert s.run(0) == "optimal"
        s.reoptimize(c=_full(np.array([1.0, 1.0]), 2))
        assert s.run(0) == "unbounded"
        ray = s.ray()
        assert ray.kind == "primal" and ray.proven
        s.reoptimize(c=_full(c, 2), constant=0.25)
        assert s.run(0) == "optimal"
        r = s.result(log=False)
        cert = certificate(a, b, c, r.basis)
        assert cert["primal_infeas"] <= 1e-9 and cert["dual_infeas"] <= 1e-9
        assert abs(r.objective - 2.25) <= 1e-9 and abs(cert["primal_obj"] - 2.0) <= 1e-9


# ------------------------------------------------------------------ 8. determinism and refusals
def test_two_solvers_through_the_same_sequence_leave_the_same_bits():
    a, b, c = _g1(46, 300, 500)
    m = a.shape[0]
    b2, c2 = rc.moved(8, b, c)
    runs = []
    for _ in range(2):
        with core.Solver(core.CoreLP.from_inequality_form(a, b, c), **FAST_OPTS) as s:
            assert s.run(70) == "iter_limit"
            s.reoptimize(b=b2, c=_full(c2, m))
            mid = s.result()
            s.reoptimize(b=b2, c=_full(c2, m))   # the same data on the same state: the same bits
            again = s.result()
            assert s.run(0) == "optimal"
            runs.append((mid, again, s.result()))
    for name in ("x", "xbar", "z", "zbar"):
        assert_bit_equal(getattr(runs[0][0], name), getattr(runs[0][1], name), "repeated call " + name)
        assert_bit_equal(getattr(runs[0][0], name), getattr(runs[1][0], name), "restart " + name)
        assert_bit_equal(getattr(runs[0][2], name), getattr(runs[1][2], name), "final " + name)
    assert runs[0][2].pivots == runs[1][2].pivots and runs[0][2].objective == runs[1][2].objective


def test_refusals():
    a, b, c = _g1(47, 37, 53)
    m, ns = a.shape
    lp = core.CoreLP.from_inequality_form(a, b, c)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=0) as s:
        with pytest.raises(_ffi.DantzigAmdError, match="refactor_interval"):
            s.reoptimize(b=b)
    with core.Solver(lp, **FAST_OPTS) as s:
        with pytest.raises(ValueError):
            s.reoptimize(b=b[:-1])
        with pytest.raises(ValueError):
            s.reoptimize(c=c)            # ns entries: the objective has one per variable, slacks included
        with pytest.raises(ValueError):
            s.reoptimize()
        bad = b.copy()
        bad[5] = np.nan
        with pytest.raises(_ffi.DantzigAmdError, match=r"rhs\[5\]"):
            s.reoptimize(b=bad)
        assert s.run(0) == "optimal"     # the refused calls changed nothing
        want = core.solve(lp, **FAST_OPTS)
        assert s.result().pivots == want.pivots
    col_ptr, row_idx, val, bs, cs = core.gen_sparse_lp(seed=3, m=40, n_struct=60, per_col=4)
    with core.Solver(core.CoreLP.from_csc(40, col_ptr, row_idx, val, bs, cs), **FAST_OPTS) as s:
        with pytest.raises(NotImplementedError, match="reoptimize is not supported"):
            s.reoptimize(b=bs)


# ------------------------------------------------------------------ 9. the session
def _satisfied(session, sol, ns):
    """Every row of the session's current model and every bound, to 1e-9."""
    by_id = {v.id: sol[v] for v in ns.values()}
    for ineq in session._inequalities():
        lhs = sum(coef * by_id[v.id] for coef, v in zip(ineq._linexpr.coefs, ineq._linexpr.vars))
        assert lhs <= ineq._b + 1e-9, (lhs, ineq._b)
    for v in ns.values():
        assert v.lb is None or sol[v] >= v.lb - 1e-9
        assert v.ub is None or sol[v] <= v.ub + 1e-9


@pytest.mark.parametrize("numerics", [core.AUTO, core.FAST], ids=["auto", "fast"])
@pytest.mark.parametrize("name", ["readme_quick_start", "non_standard_variables"])
def test_session_follows_rewritten_models(name, numerics):
    _, new_b, written, objective = next(ch for ch in CHANGES if ch[0] == name)
    k = _kat(name)
    ns, problem = build_problem(k)
    env = dict(ns)
    steps = [({}, k["constraints"], k["objective"]),
             (dict(rhs={problem.constraints[i]: v for i, v in new_b.items()}), written, k["objective"]),
             (dict(objective=eval(objective, {"__builtins__": {}}, env)), written, objective)]
    with problem.session(numerics=numerics) as session:
        for change, cons, obj in steps:
            sol = session.solve(**change)
            want = build_problem(dict(k, constraints=cons, objective=obj))[1].solve()
            scale = max(1.0, abs(want.objective_value))
            assert abs(sol.objective_value - want.objective_value) <= 1e-9 * scale, (name, obj, cons)
            _satisfied(session, sol, ns)
        assert len(session.pivots) == 3 and all(p >= 0 for p in session.pivots)
        print(f"{name}: pivots per solve {session.pivots}")


def test_session_survives_infeasible_and_unbounded_steps():
    import dantzig_amd as dz

    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    lo, hi = x + y >= 1, x + y <= 4
    with dz.Maximize(x + 0.5 * y).subject_to([lo, hi]).session() as session:
        assert abs(session.solve().objective_value - 4.0) <= 1e-9
        with pytest.raises(dz.exceptions.InfeasibleError):
            session.solve(rhs={lo: 5.0})
        assert abs(session.solve(rhs={lo: 2.0}).objective_value - 4.0) <= 1e-9
        assert abs(session.solve(rhs={hi: 6.0}).objective_value - 6.0) <= 1e-9
        assert abs(session.solve(objective=-x - y).objective_value + 2.0) <= 1e-9
    u, v = dz.Variable.nonneg(), dz.Variable.nonneg()
    with dz.Minimize(u + v).subject_to(u - v <= 2).session() as session:
        assert abs(session.solve().objective_value) <= 1e-9
        with pytest.raises(dz.exceptions.UnboundedError):
            session.solve(objective=u - 2 * v)
        assert abs(session.solve(objective=2 * u + v + 1).objective_value - 1.0) <= 1e-9
