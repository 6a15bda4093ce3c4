"""Rows and columns added to a live LP on the GPU (csrc/k_extend.hip, dzg_solver_extend,
core.Solver.extend, Session.add_constraints).

The matrix the device holds afterwards is core.extended_lp's bit for bit (column-major and the
row-major copy), at shapes that keep and grow both leading dimensions.  STRICT: the restart state is
the CPU oracle's lu_solve / neg_t_dot on the extended basis bit for bit and the pivots that follow are
the oracle's from that state.  FAST: the restart state is held to reopt_check.C_RESTART against the
state the extended basis defines in long double.  The run that follows ends at the optimum of a cold
solve of the extended LP with a basis that passes the independent certificate, over several rounds
too; the other verdicts come with proven rays; refused calls change nothing; a session follows the
model written with the added constraint.  The data is tests/extend_check.py's."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from dantzig_amd import _ffi, core
from oracle import oracle as ora
from tests import duals_reference as dref
from tests import extend_check as ec
from tests import reopt_check as rc
from tests import state_check as sc
from tests.duals_helpers import assert_bit_equal, bits
from tests.test_gpu_reopt import _kat_lp
from tests.test_reopt_host import _kat
from tests.test_surface import build_problem

pytestmark = pytest.mark.gpu

FAST_OPTS = dict(numerics=core.FAST, refactor_interval=-1)
STRICT_OPTS = dict(numerics=core.STRICT)
TOL = 1e-9


def _base_lp(seed, m, ns):
    return core.CoreLP.from_inequality_form(*ec.base(seed, m, ns))


def _optimum(s, lp):
    """(result, x* by structural column, y* by row) of a solver that has just ended optimal."""
    r = s.result()
    return r, ec.structural_values(lp, r), s.duals().y


@functools.lru_cache(maxsize=None)
def _base_optimum(seed, m, ns, fast):
    """x*, y* of the base LP, computed once per shape and numerics and never written to."""
    lp = _base_lp(seed, m, ns)
    with core.Solver(lp, **(FAST_OPTS if fast else STRICT_OPTS)) as s:
        assert s.run(0) == "optimal"
        _, xs, ys = _optimum(s, lp)
    xs.setflags(write=False)
    ys.setflags(write=False)
    return xs, ys


def _extended_positions(before, lp, p, r):
    return (list(before.basis) + list(range(lp.n + r, lp.n + r + p)),
            list(before.nonbasis) + list(range(lp.n, lp.n + r)))


# ------------------------------------------------------------------ 1. the matrix on the device
def _assert_same_bits(got, want, what):
    """Bit for bit with the sign of zero included: a -0.0 that reached the device as -0.0 is a failure."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, what
    same = bits(got) == bits(want)
    assert same.all(), f"{what}: {np.count_nonzero(~same)} of {same.size} values differ"


SHAPES = [(1, 1, 1, 0), (3, 5, 1, 1), (15, 17, 2, 0), (16, 16, 1, 3), (17, 33, 31, 2), (64, 64, 64, 0),
          (65, 130, 1, 0), (300, 500, 5, 3)]


@pytest.mark.parametrize("m,ns,p,r", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_the_matrix_on_the_device_is_the_extended_lps(m, ns, p, r):
    rng = np.random.default_rng(1000 * m + ns)
    a, b, c = rng.uniform(-1, 1, (m, ns)), rng.uniform(-1, 1, m), rng.uniform(-1, 1, ns)
    rows, cols = rng.uniform(-1, 1, (p, ns)), rng.uniform(-1, 1, (m + p, r))
    rows[p // 2, ns // 2] = -0.0
    if r:
        cols[(m + p) // 2, r // 2] = -0.0
    kw = dict(rows=rows, rhs=rng.uniform(-1, 1, p))
    if r:
        kw.update(cols=cols, c_cols=rng.uniform(-1, 1, r))
    lp = core.CoreLP.from_inequality_form(a, b, c)
    ext = core.extended_lp(lp, **kw)
    assert not np.signbit(ext.a[ext.a == 0.0]).any()
    copies = 0
    for opts in (FAST_OPTS, STRICT_OPTS):
        with core.Solver(lp, **opts) as s:
            assert s.dims() == (m, m + ns, ns)
            _assert_same_bits(s.debug_matrix(), a, "the base matrix")
            s.extend(**kw)                                   # before any run
            assert s.dims() == (m + p, m + ns + p + r, ns + r)
            _assert_same_bits(s.debug_matrix(), ext.a, f"a' {opts}")
            res = s.result()
            at = s.debug_matrix_rows()
            assert (at is not None) == bool(res.price_rows_copy), opts
            if at is not None:
                copies += 1
                _assert_same_bits(at, ext.a, f"the row-major copy {opts}")
            assert (res.status, res.iterations) == ("running", 0)
            assert res.basis.tolist() == ext.basis.tolist() and res.nonbasis.tolist() == ext.nonbasis.tolist()
            assert np.array_equal(res.x, ext.x) and np.array_equal(res.z, ext.z), opts   # x = rhs', z = -c'
            assert (res.xbar == 1.0).all() and (res.zbar == 1.0).all()
    if m >= 16:
        assert copies >= 1, "no solver kept the row-major copy: it was not checked"


# ------------------------------------------------------------------ 2. STRICT: the oracle's bits
def _strict_extend_and_continuation(lp, p, r, seed, what):
    with core.Solver(lp, **STRICT_OPTS) as s:
        assert s.run(0) == "optimal", what
        r0, xs, ys = _optimum(s, lp)
        kw = ec.draw(lp, xs, ys, p, r, seed)
        ext = core.extended_lp(lp, **kw)
        s.extend(**kw)
        r1 = s.result()
        assert (r1.status, r1.iterations) == ("running", r0.iterations) and r1.pivots == r0.pivots, what
        basis, nonbasis = _extended_positions(r0, lp, p, r)
        assert r1.basis.tolist() == basis and r1.nonbasis.tolist() == nonbasis, what
        # the restart state
        codes = ec.codes_of(ext)
        bmat = sc.columns(ext.a, ext.m, codes[r1.basis])
        assert_bit_equal(r1.x, ora.lu_solve(bmat, ext.x), what + " x")
        sf = sc.stdform(ext.a, ext.n_struct, ext.c, r1, ext.var_col)
        sf.constant = float(lp.constant)
        assert_bit_equal(r1.z, dref.core_duals(sf, r1).d[r1.nonbasis], what + " z")
        assert (r1.xbar == 1.0).all() and (r1.zbar == 1.0).all(), what
        # the continuation: the oracle from that state
        want = ora.simplex_solve(sf, xbar=r1.xbar, zbar=r1.zbar)
        assert want.status == "optimal" and want.iterations >= 1, (what, want.status, want.iterations)
        status = s.run(0)
        r2 = s.result()
    new = r2.pivots[r0.iterations:]
    print(f"{what}: {r0.iterations} pivots cold, {len(new)} after the extension, {status}")
    assert status == want.status and r2.iterations == r0.iterations + want.iterations, what
    assert r2.pivots[:r0.iterations] == r0.pivots, what
    assert [q[:3] for q in new] == [tuple(int(v) for v in q[:3]) for q in want.pivots], what
    assert_bit_equal([q[3] for q in new], [q[3] for q in want.pivots], what + " mu")
    assert_bit_equal([r2.objective], [want.objective], what + " objective")
    assert r2.basis.tolist() == want.basis.tolist(), what


@pytest.mark.parametrize("p,r,seed", [(1, 0, 1), (3, 0, 2), (0, 2, 4), (2, 2, 5)])
def test_strict_restart_state_and_continuation_are_the_oracles(p, r, seed):
    _strict_extend_and_continuation(_base_lp(31, 24, 40), p, r, seed, f"G1 24x40 +{p} rows +{r} columns")


def test_strict_extend_on_a_model_with_bound_rows():
    f, lp = _kat_lp("non_standard_variables")
    assert f.m == 7 and f.n_struct == 6 and len(f.var_col) == f.n   # var_col comes from the builder
    _strict_extend_and_continuation(lp, 1, 1, 1, "KAT non_standard_variables +1 row +1 column")


# ------------------------------------------------------------------ 3. FAST: the restart state
def _fast_extend_drift(base, p, r, seed, what, stop_at=None, **opts):
    """extend() on a FAST solver stopped after `stop_at` pivots (None: at the optimum, 0: before any
    run) by the recipe's rows and columns: (result after the call, D's parts)."""
    lp = _base_lp(*base)
    xs, ys = _base_optimum(*base, True)
    kw = ec.draw(lp, xs, ys, p, r, seed)
    ext = core.extended_lp(lp, **kw)
    with core.Solver(lp, **FAST_OPTS, **opts) as s:
        if stop_at is None:
            assert s.run(0) == "optimal", what
        elif stop_at > 0:
            assert s.run(stop_at) == "iter_limit", what
        before = s.result()
        s.extend(**kw)
        res = s.result()
    assert (res.status, res.iterations) == ("running", before.iterations) and res.pivots == before.pivots, what
    basis, nonbasis = _extended_positions(before, lp, p, r)
    assert res.basis.tolist() == basis and res.nonbasis.tolist() == nonbasis, what
    assert res.dense_columns == before.dense_columns, what
    assert (res.xbar == 1.0).all() and (res.zbar == 1.0).all(), what
    assert res.state_drift == 0.0, what
    ex = sc.exact_state(ext.a, ext.n_struct, ext, res.basis, res.nonbasis, ext.var_col)
    d = rc.restart_drift(ex, res)
    print(f"{what}: k = {res.dense_columns}, D = {d['D']:.3e} (x {d['x']:.3e}, z {d['z']:.3e}), "
          f"helper error {max(ex.err['x'], ex.err['z']):.1e}")
    assert max(ex.err["x"], ex.err["z"]) * 1e2 <= rc.C_RESTART, (what, ex.err)
    assert d["D"] <= rc.C_RESTART, (what, d)
    return res, ext


def test_fast_restart_state_at_odd_even_and_zero_k():
    from tests.test_gpu_reopt import _stops_with_odd_and_even_k

    base = (41, 37, 53)
    odd, even = _stops_with_odd_and_even_k(*ec.base(*base))
    res, _ = _fast_extend_drift(base, 2, 2, 5, "37x53 +2+2 odd k", stop_at=odd)
    assert res.dense_columns % 2 == 1
    res, _ = _fast_extend_drift(base, 2, 2, 5, "37x53 +2+2 even k", stop_at=even)
    assert res.dense_columns % 2 == 0 and res.dense_columns > 0
    res, ext = _fast_extend_drift(base, 2, 2, 5, "37x53 +2+2 slack basis", stop_at=0)
    assert res.dense_columns == 0 and res.iterations == 0
    assert np.array_equal(res.x, ext.x) and np.array_equal(res.z, ext.z)   # x = rhs', z = -c', exactly


@pytest.mark.parametrize("seven", [0, 1], ids=["three launches", "seven launches"])
def test_fast_restart_state_at_the_optimum_300x500(seven):
    res, _ = _fast_extend_drift((42, 300, 500), 5, 3, 6, f"300x500 +5+3 seven_launches={seven}",
                                seven_launches=seven)
    assert 0 < res.dense_columns <= 512


def test_fast_restart_state_with_the_64_lane_rows_640x1280():
    """Without extend's refinement step this basis shows D = 3.544e-12, above C_RESTART (and 3.535e-12
    for reoptimize with the base LP's own data, no extension at all: DESIGN.md 7i); with it 1.8e-15."""
    res, _ = _fast_extend_drift(ec.LARGE, 17, 0, 8, "640x1280 +17")
    assert res.dense_columns > 512, "the 64-lane instantiation of k_restart_x did not run"


# ------------------------------------------------------------------ 4. the optimum of a cold solve
def _matches_cold(s, ext, opts, before_iterations, what, need_pivot=True):
    """The solver has just run on `ext`: optimal, at least one pivot since (need_pivot), the objective
    of a cold solve of `ext`, a final basis that passes the certificate, duals of the extended sizes."""
    res = s.result(log=False)
    cold = core.solve(ext, log=False, **opts)
    assert cold.status == "optimal" and res.status == "optimal", (what, cold.status, res.status)
    assert res.iterations > before_iterations or not need_pivot, (what, "the continuation took no pivot")
    scale = max(1.0, abs(cold.objective))
    assert abs(res.objective - cold.objective) <= TOL * scale, (what, res.objective, cold.objective)
    cert = ec.check_certificate(ext, res, TOL)
    du = s.duals()
    assert du.y.shape == (ext.m,) and du.d.shape == (ext.n,), what
    assert np.abs(du.y - cert["y"]).max() <= TOL * max(1.0, np.abs(cert["y"]).max()), what
    assert abs(du.primal_obj - du.dual_obj) <= TOL * scale, what
    print(f"{what}: {before_iterations} pivots before, {res.iterations - before_iterations} after, "
          f"{cold.iterations} cold")
    return res


@pytest.mark.parametrize("p,r,seed", ec.RECIPE)
@pytest.mark.parametrize("fast", [False, True], ids=["strict 24x40", "fast 300x500"])
def test_extend_and_run_reach_the_cold_optimum(fast, p, r, seed):
    base, opts = ((42, 300, 500), FAST_OPTS) if fast else ((31, 24, 40), STRICT_OPTS)
    lp = _base_lp(*base)
    with core.Solver(lp, **opts) as s:
        assert s.run(0) == "optimal"
        r0, xs, ys = _optimum(s, lp)
        kw = ec.draw(lp, xs, ys, p, r, seed)
        ext = core.extended_lp(lp, **kw)
        s.extend(**kw)
        assert s.run(0) == "optimal"
        _matches_cold(s, ext, opts, r0.iterations, f"{base[1]}x{base[2]} +{p}+{r}")


# ------------------------------------------------------------------ 5. rounds
ROUNDS = [(2, 2, 5), (3, 0, 2), (0, 2, 4)]


@pytest.mark.parametrize("fast", [False, True], ids=["strict 24x40", "fast 300x500"])
def test_three_rounds_then_a_new_right_hand_side(fast):
    base, opts = ((42, 300, 500), FAST_OPTS) if fast else ((31, 24, 40), STRICT_OPTS)
    finals = []
    for handle in range(2):
        lp = _base_lp(*base)
        with core.Solver(lp, **opts) as s:
            assert s.run(0) == "optimal"
            for k, (p, r, seed) in enumerate(ROUNDS):
                r0, xs, ys = _optimum(s, lp)
                kw = ec.draw(lp, xs, ys, p, r, seed)
                ext = core.extended_lp(lp, **kw)
                s.extend(**kw)
                assert s.run(0) == "optimal"
                if handle == 0:
                    _matches_cold(s, ext, opts, r0.iterations, f"round {k} {ext.m}x{ext.n_struct}")
                lp = ext
            assert s.dims() == (lp.m, lp.n, lp.n_struct)
            # reoptimize takes m' entries afterwards and runs to the cold optimum of that change
            b2 = lp.x + np.random.default_rng(9).random(lp.m)
            with pytest.raises(ValueError):
                s.reoptimize(b=b2[:base[1]])
            before = s.result(log=False).iterations
            s.reoptimize(b=b2)
            assert s.run(0) == "optimal"
            moved = dataclasses.replace(lp, x=b2)
            if handle == 0:
                _matches_cold(s, moved, opts, before, "the new right-hand side", need_pivot=False)
            finals.append(s.result())
    for name in ("x", "xbar", "z", "zbar"):
        assert_bit_equal(getattr(finals[0], name), getattr(finals[1], name), "two handles " + name)
    assert finals[0].pivots == finals[1].pivots and finals[0].objective == finals[1].objective
    assert finals[0].basis.tolist() == finals[1].basis.tolist()


# ------------------------------------------------------------------ 6. the other verdicts
@pytest.mark.parametrize("fast", [False, True], ids=["strict 24x40", "fast 37x53"])
def test_the_other_verdicts_come_with_proven_rays(fast):
    base, opts = ((41, 37, 53), FAST_OPTS) if fast else ((31, 24, 40), STRICT_OPTS)
    lp = _base_lp(*base)
    m, ns = lp.m, lp.n_struct
    rng = np.random.default_rng(12)
    with core.Solver(lp, **opts) as s:
        assert s.run(0) == "optimal"
        s.extend(rows=rng.uniform(0.5, 1.5, (1, ns)), rhs=[-1.0])          # g . x <= -1 with g > 0, x >= 0
        assert s.run(0) == "infeasible"
        ray = s.ray()
        assert ray.kind == "farkas" and ray.proven and ray.y.shape == (m + 1,) and ray.d.shape == (lp.n + 1,)
    with core.Solver(lp, **opts) as s:
        assert s.run(0) == "optimal"
        s.extend(cols=-rng.uniform(0.0, 1.0, (m, 1)), c_cols=[1.0])        # gains for ever, uses nothing
        assert s.run(0) == "unbounded"
        ray = s.ray()
        assert ray.kind == "primal" and ray.proven and ray.d.shape == (lp.n + 1,)


# ------------------------------------------------------------------ 7. refusals
def test_refusals_change_nothing():
    a, b, c = ec.base(41, 37, 53)
    m, ns = a.shape
    lp = core.CoreLP.from_inequality_form(a, b, c)
    rows, rhs = np.random.default_rng(13).random((2, ns)), np.ones(2)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=0) as s:
        with pytest.raises(_ffi.DantzigAmdError, match="refactor_interval"):
            s.extend(rows=rows, rhs=rhs)
        assert s._lp is lp and s.dims() == (m, m + ns, ns)
    with core.Solver(lp, **FAST_OPTS) as s:
        bad = rows.copy()
        bad[1, 2] = np.nan
        with pytest.raises(_ffi.DantzigAmdError, match=rf"rows\[{ns + 2}\]"):
            s.extend(rows=bad, rhs=rhs)
        with pytest.raises(_ffi.DantzigAmdError, match=r"rhs\[1\]"):
            s.extend(rows=rows, rhs=[1.0, np.inf])
        with pytest.raises(_ffi.DantzigAmdError, match=r"c_cols\[0\]"):
            s.extend(cols=np.ones((m, 1)), c_cols=[np.nan])
        ext = _ffi.Extend(0, 0, None, ns, None, None, m, None)
        assert _ffi.lib().dzg_solver_extend(s._h, C.byref(ext)) == _ffi.E_ARG      # p == r == 0
        ext = _ffi.Extend(-1, 0, None, ns, None, None, m, None)
        assert _ffi.lib().dzg_solver_extend(s._h, C.byref(ext)) == _ffi.E_ARG      # a negative count
        ext = _ffi.Extend(2, 0, _ffi.ptr(rows), ns - 1, _ffi.ptr(rhs), None, m, None)
        assert _ffi.lib().dzg_solver_extend(s._h, C.byref(ext)) == _ffi.E_ARG      # ld_rows too small
        ext = _ffi.Extend(2, 0, None, ns, _ffi.ptr(rhs), None, m, None)
        assert _ffi.lib().dzg_solver_extend(s._h, C.byref(ext)) == _ffi.E_ARG      # rows is NULL
        assert s._lp is lp and s.dims() == (m, m + ns, ns)
        assert s.run(0) == "optimal"     # the refused calls changed nothing
        want = core.solve(lp, **FAST_OPTS)
        assert s.result().pivots == want.pivots
    col_ptr, row_idx, val, bs, cs = core.gen_sparse_lp(seed=3, m=40, n_struct=60, per_col=4)
    with core.Solver(core.CoreLP.from_csc(40, col_ptr, row_idx, val, bs, cs), **FAST_OPTS) as s:
        with pytest.raises(NotImplementedError, match="extend is not supported"):
            s.extend(rows=np.ones((1, 60)), rhs=[1.0])
        one, r1 = np.ones((1, 60)), np.ones(1)
        ext = _ffi.Extend(1, 0, _ffi.ptr(one), 60, _ffi.ptr(r1), None, 41, None)
        with pytest.raises(NotImplementedError, match="extend is not supported on CSC storage or sharded"):
            _ffi.check_extend(_ffi.lib().dzg_solver_extend(s._h, C.byref(ext)), "dzg_solver_extend")


# ------------------------------------------------------------------ 8. the session
def _satisfied(session, sol, ns):
    """Every row of the session's current model, the added constraints included, and every bound, to 1e-9."""
    by_id = {v.id: sol[v] for v in ns.values()}
    rows = [(ineq._linexpr, ineq._b) for ineq in session._inequalities()]
    for con in session._added:
        new_b = session._rhs.get(id(con))
        for ineq, sign in zip(con.rust_inequalities(), con._signs):
            rows.append((ineq._linexpr, ineq._b if new_b is None else sign * new_b))
    for linexpr, b in rows:
        lhs = sum(coef * by_id[v.id] for coef, v in zip(linexpr.coefs, linexpr.vars))
        assert lhs <= b + 1e-9, (lhs, b)
    for v in ns.values():
        assert v.lb is None or sol[v] >= v.lb - 1e-9
        assert v.ub is None or sol[v] <= v.ub + 1e-9
    return len(rows)


@pytest.mark.parametrize("numerics", [core.AUTO, core.FAST], ids=["auto", "fast"])
@pytest.mark.parametrize("name", ["readme_quick_start", "non_standard_variables"])
def test_session_follows_the_model_written_with_the_added_constraint(name, numerics):
    text, new_b, text_new_b = ec.ADDED[name]
    k = _kat(name)
    ns, problem = build_problem(k)
    con = eval(text, {"__builtins__": {}}, dict(ns))
    with problem.session(numerics=numerics) as session:
        first = session.solve()
        want = problem.solve()
        assert abs(first.objective_value - want.objective_value) <= TOL * max(1.0, abs(want.objective_value))
        # the cut is violated by the first solution
        ineq = con.rust_inequalities()[0]
        lhs = sum(coef * first[next(v for v in ns.values() if v.id == var.id)]
                  for coef, var in zip(ineq._linexpr.coefs, ineq._linexpr.vars))
        assert lhs > ineq._b + 1e-6, (lhs, ineq._b)
        session.add_constraints(con)
        base_rows = len(session._inequalities())
        for change, written in (({}, text), (dict(rhs={con: new_b}), text_new_b)):
            sol = session.solve(**change)
            want = build_problem(dict(k, constraints=k["constraints"] + [written]))[1].solve()
            scale = max(1.0, abs(want.objective_value))
            assert abs(sol.objective_value - want.objective_value) <= TOL * scale, (name, written)
            assert abs(want.objective_value - first.objective_value) > 1e-6, (name, "the cut changes nothing")
            assert _satisfied(session, sol, ns) == base_rows + 1
        assert len(session.pivots) == 3 and all(q >= 0 for q in session.pivots) and session.pivots[1] >= 1
        assert session._solver.dims()[0] == session._form.m + 1
        print(f"{name}: pivots per solve {session.pivots}")
