"""Rows and columns removed from a live LP on the GPU (csrc/k_remove.hip, dzg_solver_remove,
core.Solver.remove, Session.remove_constraints).

The matrix the device holds afterwards is core.reduced_lp's bit for bit (column-major and the row-major
copy), at shapes that keep and lower the leading dimension.  At an optimum everything removable()
offers goes and the run that follows takes no pivot: STRICT with the CPU oracle's lu_solve /
core_duals on the reduced basis bit for bit, FAST held to reopt_check.C_RESTART against the state the
reduced basis defines in long double.  The loop it is for -- extend by cuts, run, purge the slack
ones, extend, run -- ends at the cold optimum of the accumulated LP; refused calls change nothing; a
session follows the model written without the removed constraint.  The data is
tests/remove_check.py's and tests/extend_check.py's."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from dantzig_amd import _ffi, core
from oracle import oracle as ora
from tests import duals_reference as dref
from tests import extend_check as ec
from tests import remove_check as rmc
from tests import reopt_check as rc
from tests import state_check as sc
from tests.duals_helpers import assert_bit_equal, bits
from tests.test_reopt_host import _kat
from tests.test_surface import build_problem

pytestmark = pytest.mark.gpu

FAST_OPTS = dict(numerics=core.FAST, refactor_interval=-1)
STRICT_OPTS = dict(numerics=core.STRICT)
TOL = 1e-9


def _base_lp(seed, m, ns):
    return core.CoreLP.from_inequality_form(*ec.base(seed, m, ns))


def _assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, what
    same = bits(got) == bits(want)
    assert same.all(), f"{what}: {np.count_nonzero(~same)} of {same.size} values differ"


def _surviving(before, var_map):
    """(basis, nonbasis, x, z) of `before` without what var_map dropped, renumbered, in order."""
    kb, kn = var_map[before.basis] >= 0, var_map[before.nonbasis] >= 0
    return (var_map[before.basis[kb]].tolist(), var_map[before.nonbasis[kn]].tolist(), before.x[kb],
            before.z[kn])


def _removed(s, lp, rows, cols, what):
    """s.remove(rows, cols) on a solver that holds `lp` (in its slack start): (the reduced LP in its
    slack start, result before, result after), the maps, the sizes and the lists checked."""
    before = s.result()
    red, var_map, row_map = core.reduced_lp(lp, rows=rows, cols=cols)   # (everything is free at a slack start)
    got_var, got_row = s.remove(rows=rows or None, cols=cols or None)
    assert got_var.tolist() == var_map.tolist() and got_row.tolist() == row_map.tolist(), what
    assert s.dims() == (red.m, red.n, red.n_struct), what
    res = s.result()
    basis, nonbasis, _, _ = _surviving(before, var_map)
    assert res.basis.tolist() == basis and res.nonbasis.tolist() == nonbasis, what
    assert (res.status, res.iterations) == ("running", before.iterations) and res.pivots == before.pivots, what
    assert (res.xbar == 1.0).all() and (res.zbar == 1.0).all(), what
    return red, before, res


# ------------------------------------------------------------------ 1. the matrix on the device
_copies = []


@pytest.mark.parametrize("m,ns,rows,cols", rmc.MATRIX_CASES,
                         ids=[f"{m}x{ns}-{len(r)}-{len(c)}" for m, ns, r, c in rmc.MATRIX_CASES])
def test_the_matrix_on_the_device_is_the_reduced_lps(m, ns, rows, cols):
    lp = rmc.random_lp(m, ns)
    for opts in ((FAST_OPTS,) if m > 2048 else (FAST_OPTS, STRICT_OPTS)):
        with core.Solver(lp, **opts) as s:
            free_rows, free_cols = s.removable()
            assert free_rows.all() and free_cols.all(), opts          # the slack start
            red, _, res = _removed(s, lp, rows, cols, f"{m}x{ns} {opts}")   # before any run
            assert red.a.shape == (m - len(rows), ns - len(cols))
            _assert_same_bits(s.debug_matrix(), red.a, f"a' {opts}")
            at = s.debug_matrix_rows()
            assert (at is not None) == bool(res.price_rows_copy), opts
            if at is not None:
                _copies.append((m, ns))
                _assert_same_bits(at, red.a, f"the row-major copy {opts}")
            assert res.basis.tolist() == red.basis.tolist() and res.nonbasis.tolist() == red.nonbasis.tolist()
            assert np.array_equal(res.x, red.x) and np.array_equal(res.z, red.z), opts   # x = rhs', z = -c'
            assert np.array_equal(red.x, lp.x[np.setdiff1d(np.arange(m), rows)])
            free_rows, free_cols = s.removable()
            assert free_rows.shape == (red.m,) and free_cols.shape == (red.n_struct,) and free_rows.all()


def test_some_matrix_case_kept_the_row_major_copy():
    """(runs after the cases above) the copy the row-wise pricing pass reads was checked at least once"""
    if not _copies:     # this test on its own: one case that keeps the copy
        test_the_matrix_on_the_device_is_the_reduced_lps(*rmc.MATRIX_CASES[4])
    assert _copies, "no solver kept the row-major copy: it was not checked"


# ------------------------------------------------------------------ 2, 3. at the optimum
def _remove_at_the_optimum(base, opts, what):
    """Everything removable() offers goes at the optimum of a base LP; returns what the checks of
    either numerics need.  The continuation: 0 pivots, the same objective, the certificate."""
    lp = _base_lp(*base)
    out = {}
    s = core.Solver(lp, **opts)
    assert s.run(0) == "optimal", what
    r0 = s.result()
    row_mask, col_mask = s.removable()
    want_rows, want_cols = rmc.free_masks(rmc.at_basis(lp, r0))
    assert row_mask.tolist() == want_rows.tolist() and col_mask.tolist() == want_cols.tolist(), what
    at_least = rmc.FREE_AT_LEAST[base]
    assert row_mask.sum() >= at_least[0] and col_mask.sum() >= at_least[1], (what, row_mask.sum(), col_mask.sum())
    rows, cols = np.flatnonzero(row_mask).tolist(), np.flatnonzero(col_mask).tolist()
    red, before, res = _removed(s, lp, rows, cols, what)
    out.update(s=s, lp=lp, red=red, r0=r0, r1=res, rows=rows, cols=cols)
    return out


def _continuation(o, opts, what):
    s, red, r0, r1 = o["s"], o["red"], o["r0"], o["r1"]
    assert s.run(0) == "optimal", what
    r2 = s.result()
    assert r2.iterations == r0.iterations and r2.pivots == r0.pivots, (what, "the continuation took a pivot")
    scale = max(1.0, abs(r0.objective))
    assert abs(r2.objective - r0.objective) <= TOL * scale, (what, r2.objective, r0.objective)
    cert = ec.check_certificate(red, r2, TOL)
    du = s.duals()
    assert du.y.shape == (red.m,) and du.d.shape == (red.n,), what
    assert np.abs(du.y - cert["y"]).max() <= TOL * max(1.0, np.abs(cert["y"]).max()), what
    print(f"{what}: {len(o['rows'])} rows and {len(o['cols'])} columns removed, {red.m}x{red.n_struct} left, "
          f"{r2.iterations - r0.iterations} new pivots")
    return r2


@pytest.mark.parametrize("base", ec.BASES[:2], ids=["24x40", "37x53"])
def test_strict_removal_at_the_optimum_is_the_oracles_state_and_takes_no_pivot(base):
    what = f"strict {base[1]}x{base[2]}"
    o = _remove_at_the_optimum(base, STRICT_OPTS, what)
    with o["s"] as s:
        red, r1 = o["red"], o["r1"]
        codes = ec.codes_of(red)
        assert_bit_equal(r1.x, ora.lu_solve(sc.columns(red.a, red.m, codes[r1.basis]), red.x), what + " x")
        sf = sc.stdform(red.a, red.n_struct, red.c, r1, red.var_col)
        sf.constant = float(red.constant)
        assert_bit_equal(r1.z, dref.core_duals(sf, r1).d[r1.nonbasis], what + " z")
        _continuation(o, STRICT_OPTS, what)
        # reoptimize takes m' entries afterwards and ends at the cold optimum of that change
        b2 = red.x + np.random.default_rng(9).random(red.m)
        with pytest.raises(ValueError):
            s.reoptimize(b=b2[:-1])
        s.reoptimize(b=b2)
        assert s.run(0) == "optimal"
        moved = dataclasses.replace(red, x=b2)
        cold = core.solve(moved, log=False, **STRICT_OPTS)
        got = s.result(log=False)
        assert cold.status == "optimal"
        assert abs(got.objective - cold.objective) <= TOL * max(1.0, abs(cold.objective)), what
        ec.check_certificate(moved, got, TOL)


@pytest.mark.parametrize("base", ec.BASES[1:], ids=["37x53", "300x500"])
def test_fast_removal_at_the_optimum_restart_state_and_no_pivot(base):
    what = f"fast {base[1]}x{base[2]}"
    finals = []
    for handle in range(2):
        o = _remove_at_the_optimum(base, FAST_OPTS, what)
        with o["s"]:
            red, r1 = o["red"], o["r1"]
            if handle == 0:
                assert r1.state_drift == 0.0, what
                ex = sc.exact_state(red.a, red.n_struct, red, r1.basis, r1.nonbasis, red.var_col)
                d = rc.restart_drift(ex, r1)
                print(f"{what}: k = {r1.dense_columns}, D = {d['D']:.3e} (x {d['x']:.3e}, z {d['z']:.3e}), "
                      f"helper error {max(ex.err['x'], ex.err['z']):.1e}")
                assert max(ex.err["x"], ex.err["z"]) * 1e2 <= rc.C_RESTART, (what, ex.err)
                assert d["D"] <= rc.C_RESTART, (what, d)
            finals.append((r1, _continuation(o, FAST_OPTS, what)))
    for k in range(2):
        for name in ("x", "xbar", "z", "zbar"):
            assert_bit_equal(getattr(finals[0][k], name), getattr(finals[1][k], name), f"two handles {name}")
        assert finals[0][k].basis.tolist() == finals[1][k].basis.tolist()
        assert finals[0][k].objective == finals[1][k].objective


# ------------------------------------------------------------------ 4. the loop it is for
@pytest.mark.parametrize("fast", [False, True], ids=["strict 24x40", "fast 300x500"])
def test_extend_run_purge_extend_run_reaches_the_cold_optimum(fast):
    base, opts = ((42, 300, 500), FAST_OPTS) if fast else ((31, 24, 40), STRICT_OPTS)
    what = f"{base[1]}x{base[2]}"
    lp = _base_lp(*base)                      # the accumulated LP, in its slack start
    with core.Solver(lp, **opts) as s:
        assert s.run(0) == "optimal"
        r = s.result()
        # round 1: five cuts
        kw = ec.draw(lp, ec.structural_values(lp, r), s.duals().y, 5, 0, 8)
        m0, ns0 = lp.m, lp.n_struct
        lp = core.extended_lp(lp, **kw)
        s.extend(**kw)
        assert s.run(0) == "optimal"
        r = s.result()
        # the purge: the cuts that went slack
        row_mask, _ = s.removable()
        slack_cuts = [i for i in range(m0, m0 + 5) if row_mask[i]]
        print(f"{what}: {len(slack_cuts)} of 5 cuts are slack")
        assert len(slack_cuts) >= 1, (what, "no cut went slack")
        before = r.iterations
        var_map, row_map = s.remove(rows=slack_cuts)
        lp, want_var, want_row = core.reduced_lp(lp, rows=slack_cuts)
        assert var_map.tolist() == want_var.tolist() and row_map.tolist() == want_row.tolist()
        assert s.dims() == (lp.m, lp.n, lp.n_struct) == (m0 + 5 - len(slack_cuts), lp.n, ns0)
        assert s.run(0) == "optimal"
        r = s.result()
        assert r.iterations == before, (what, "the purge cost pivots")
        # round 2 on the purged LP: three cuts and three columns
        kw = ec.draw(lp, ec.structural_values(lp, r), s.duals().y, 3, 3, 9)
        lp = core.extended_lp(lp, **kw)
        s.extend(**kw)
        assert s.run(0) == "optimal"
        res = s.result(log=False)
        assert res.iterations > before, (what, "the second round took no pivot")
        cold = core.solve(lp, log=False, **opts)
        assert cold.status == "optimal"
        assert abs(res.objective - cold.objective) <= TOL * max(1.0, abs(cold.objective)), (what, res.objective)
        ec.check_certificate(lp, res, TOL)
        # the columns of the second round that ended nonbasic go too, at no cost
        col_mask = s.removable()[1]
        idle = [j for j in range(lp.n_struct - 3, lp.n_struct) if col_mask[j]]
        print(f"{what}: {len(idle)} of 3 new columns ended nonbasic")
        if idle:
            s.remove(cols=idle)
            lp2, _, _ = core.reduced_lp(lp, cols=idle)
            assert s.dims() == (lp2.m, lp2.n, lp2.n_struct)
            assert s.run(0) == "optimal"
            last = s.result(log=False)
            assert last.iterations == res.iterations
            assert abs(last.objective - cold.objective) <= TOL * max(1.0, abs(cold.objective))
            ec.check_certificate(lp2, last, TOL)


# ------------------------------------------------------------------ 5. refusals
def test_refusals_change_nothing():
    lp = _base_lp(41, 37, 53)
    m, ns = lp.m, lp.n_struct
    lib = _ffi.lib()

    def refused(s, rows, cols, match):
        r, c = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        var_map, row_map = np.full(lp.n, 7, np.int64), np.full(m, 7, np.int64)
        rem = _ffi.Remove(len(r), _ffi.ptr(r) if len(r) else None, len(c), _ffi.ptr(c) if len(c) else None)
        assert lib.dzg_solver_remove(s._h, C.byref(rem), _ffi.ptr(var_map), _ffi.ptr(row_map)) == _ffi.E_ARG
        assert match in lib.dzg_last_error().decode(), lib.dzg_last_error()
        assert (var_map == 7).all() and (row_map == 7).all()               # the maps are not written

    with core.Solver(lp, numerics=core.FAST, refactor_interval=0) as s:
        with pytest.raises(_ffi.DantzigAmdError, match="refactor_interval"):
            s.remove(rows=[0])
        assert s._lp is lp and s.dims() == (m, m + ns, ns)
    want = core.solve(lp, **FAST_OPTS)
    with core.Solver(lp, **FAST_OPTS) as s:
        assert s.run(0) == "optimal"
        row_mask, col_mask = s.removable()
        binding, basic = int(np.flatnonzero(~row_mask)[0]), int(np.flatnonzero(~col_mask)[0])
        free = int(np.flatnonzero(row_mask)[0])
        with pytest.raises(ValueError, match=f"row {binding} is binding"):
            s.remove(rows=[binding])
        with pytest.raises(ValueError, match=f"column {basic} is basic"):
            s.remove(cols=[basic])
        with pytest.raises(ValueError, match="listed twice"):
            s.remove(rows=[free, free])
        # the C call itself
        refused(s, [free, binding], [], f"row {binding} is binding")
        refused(s, [free], [basic], f"column {basic} is basic")
        refused(s, [free, free], [], "listed twice")
        refused(s, [m], [], "out of range")
        refused(s, [], [-1], "out of range")
        refused(s, [], [], "nothing to remove")
        refused(s, list(range(m)), [], "must stay")
        rem = _ffi.Remove(-1, None, 0, None)
        assert lib.dzg_solver_remove(s._h, C.byref(rem), None, None) == _ffi.E_ARG      # a negative count
        rem = _ffi.Remove(1, None, 0, None)
        assert lib.dzg_solver_remove(s._h, C.byref(rem), None, None) == _ffi.E_ARG      # rows is NULL
        assert s._lp is lp and s.dims() == (m, m + ns, ns)
        assert s.run(0) == "optimal"     # the refused calls changed nothing: an untouched handle's pivots
        assert s.result().pivots == want.pivots
    col_ptr, row_idx, val, bs, cs = core.gen_sparse_lp(seed=3, m=40, n_struct=60, per_col=4)
    with core.Solver(core.CoreLP.from_csc(40, col_ptr, row_idx, val, bs, cs), **FAST_OPTS) as s:
        with pytest.raises(NotImplementedError, match="remove is not supported"):
            s.remove(rows=[0])
        one = np.zeros(1, np.int64)
        rem = _ffi.Remove(1, _ffi.ptr(one), 0, None)
        with pytest.raises(NotImplementedError, match="remove is not supported on CSC storage or sharded"):
            _ffi.check_extend(lib.dzg_solver_remove(s._h, C.byref(rem), None, None), "dzg_solver_remove")


# ------------------------------------------------------------------ 6. the session
def _same_solution(got, want, ns, what):
    scale = max(1.0, abs(want.objective_value))
    assert abs(got.objective_value - want.objective_value) <= TOL * scale, (what, got.objective_value)
    for name, v in ns.items():
        assert abs(got[v] - want[v]) <= 1e-9 * max(1.0, abs(want[v])), (what, name, got[v], want[v])


@pytest.mark.parametrize("numerics", [core.AUTO, core.FAST], ids=["auto", "fast"])
@pytest.mark.parametrize("name", sorted(rmc.LOOSENED))
def test_session_drops_a_slack_added_constraint_on_the_live_solver(name, numerics):
    ns, problem = build_problem(_kat(name))
    con = eval(rmc.LOOSENED[name], {"__builtins__": {}}, dict(ns))
    want = problem.solve()
    with problem.session(numerics=numerics) as session:
        _same_solution(session.solve(), want, ns, name)
        session.add_constraints(con)
        _same_solution(session.solve(), want, ns, name + " with the slack constraint")
        held = session._solver.dims()
        assert held[0] == session._form.m + 1
        assert session.remove_constraints(con) is session
        _same_solution(session.solve(), want, ns, name + " without it again")
        assert session.rebuilds == 0 and session._solver.dims() == (held[0] - 1, held[1] - 1, held[2])
        session.add_constraints(con)                       # and it may come back
        _same_solution(session.solve(), want, ns, name + " added again")
        assert session._solver.dims() == held
    print(f"{name}: pivots per solve {session.pivots}")


@pytest.mark.parametrize("name", ["readme_quick_start", "non_standard_variables"])
def test_session_rebuilds_for_a_binding_constraint(name):
    ns, problem = build_problem(_kat(name))
    con = eval(ec.ADDED[name][0], {"__builtins__": {}}, dict(ns))
    want = problem.solve()
    with problem.session() as session:
        session.solve()
        session.add_constraints(con)
        cut = session.solve()
        assert abs(cut.objective_value - want.objective_value) > 1e-6, (name, "the cut changes nothing")
        session.remove_constraints(con)
        _same_solution(session.solve(), want, ns, name)
        assert session.rebuilds == 1 and session._solver.dims()[0] == session._form.m
        # an original constraint of the model: a rebuild too, and the model written without it
        first = problem.constraints[0]
        session.remove_constraints(first)
        k = _kat(name)
        try:
            less = build_problem(dict(k, constraints=k["constraints"][1:]))[1].solve()
        except Exception as exc:                            # (unbounded without it)
            with pytest.raises(type(exc)):
                session.solve()
        else:
            got = session.solve()
            assert abs(got.objective_value - less.objective_value) <= TOL * max(1.0, abs(less.objective_value))
        assert session.rebuilds == 2
    print(f"{name}: pivots per solve {session.pivots}")


def test_session_equality_constraint_goes_by_whichever_path_applies():
    name = "inventory_balance"
    ns, problem = build_problem(_kat(name))
    con = eval(ec.ADDED[name][0], {"__builtins__": {}}, dict(ns))
    want = problem.solve()
    with problem.session() as session:
        session.solve()
        session.add_constraints(con)
        cut = session.solve()
        assert abs(cut.objective_value - want.objective_value) > 1e-6
        assert session._solver.dims()[0] == session._form.m + 2          # an == is two rows
        free = session._solver.removable()[0][session._form.m:]
        session.remove_constraints(con)
        got = session.solve()
        scale = max(1.0, abs(want.objective_value))
        assert abs(got.objective_value - want.objective_value) <= TOL * scale
        assert session.rebuilds == (0 if free.all() else 1)
        assert session._solver.dims()[0] == session._form.m
    print(f"{name}: both rows free: {bool(free.all())}, pivots per solve {session.pivots}")
