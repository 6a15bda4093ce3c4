"""Rows and columns added to a live LP (dzg_solver_extend, core.Solver.extend, core.extended_lp,
Session.add_constraints), the parts that need no GPU: the entry points and their mirror, the argument
checks that run before any device work, the numbering rule on the host, the session's rows for an added
constraint against the library's builder on the model written with that constraint, and the recipe of
tests/extend_check.py against HiGHS on the small shapes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi, core
from dantzig_amd import rust as rs
from tests import extend_check as ec
from tests.test_reopt_host import _form, _kat
from tests.test_surface import build_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dzg_solver_extend", "dzg_solver_dims", "dzg_debug_matrix", "dzg_debug_matrix_rows"]


# ------------------------------------------------------------------ the C entry points
def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "dantzig_amd.h")).read()
    assert "int dzg_solver_extend(dzg_solver *s, const dzg_extend *ext);" in text
    assert "int dzg_solver_dims(const dzg_solver *s, int64_t *m, int64_t *n, int64_t *n_struct);" in text
    assert "#define DZG_ABI_VERSION 4" in text
    for name in NEW:
        assert name in text and name in _ffi.EXPORTS and hasattr(_ffi.lib(), name), name
    assert _ffi.lib().dzg_abi_version() == 4


def test_mirror_layout_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dantzig_amd.h"', 'int main(void) {',
             'printf("dzg_extend %zu\\n", sizeof(dzg_extend));']
    for field, _ in _ffi.Extend._fields_:
        lines.append(f'printf("dzg_extend.{field} %zu\\n", offsetof(dzg_extend, {field}));')
    lines += ['return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["dzg_extend"]) == C.sizeof(_ffi.Extend) == 64
    assert [f for f, _ in _ffi.Extend._fields_] == ["n_rows", "n_cols", "rows", "ld_rows", "rhs", "cols",
                                                   "ld_cols", "c_cols"]
    for field, _ in _ffi.Extend._fields_:
        assert int(got[f"dzg_extend.{field}"]) == getattr(_ffi.Extend, field).offset, field


def test_null_arguments_are_argument_errors_on_the_host():
    lib = _ffi.lib()
    ext = _ffi.Extend(1, 0, None, 1, None, None, 1, None)
    assert lib.dzg_solver_extend(None, C.byref(ext)) == _ffi.E_ARG
    assert lib.dzg_solver_extend(None, None) == _ffi.E_ARG
    assert b"NULL" in lib.dzg_last_error()
    m = C.c_int64(0)
    assert lib.dzg_solver_dims(None, C.byref(m), None, None) == _ffi.E_ARG
    with pytest.raises(_ffi.DantzigAmdError):
        _ffi.check_extend(lib.dzg_solver_extend(None, None), "dzg_solver_extend")


def test_check_extend_maps_the_unsupported_routes():
    class _Lib:
        @staticmethod
        def dzg_last_error():
            return b"extend is not supported on CSC storage or sharded solvers"

        @staticmethod
        def dzg_status_str(code):
            return b"invalid_argument"
    real = _ffi._lib
    _ffi.lib()
    try:
        _ffi._lib = _Lib()
        with pytest.raises(NotImplementedError, match="extend is not supported"):
            _ffi.check_extend(_ffi.E_ARG, "dzg_solver_extend")
    finally:
        _ffi._lib = real


def test_solver_has_extend_with_a_docstring():
    assert "dzg_solver_extend" in core.Solver.extend.__doc__


# ------------------------------------------------------------------ the numbering rule, on the host
def _blocks(rng, m, ns, p, r):
    rows, cols = rng.uniform(-1, 1, (p, ns)), rng.uniform(-1, 1, (m + p, r))
    if p and ns:
        rows[p // 2, ns // 2] = -0.0
    if r:
        cols[(m + p) // 2, r // 2] = -0.0
    return rows, rng.uniform(-1, 1, p), cols, rng.uniform(-1, 1, r)


@pytest.mark.parametrize("explicit", [False, True], ids=["benchmark convention", "explicit var_col"])
def test_extended_lp_follows_the_numbering_rule(explicit):
    m, ns, p, r = 5, 7, 3, 2
    rng = np.random.default_rng(11)
    a, b, c = rng.uniform(-1, 1, (m, ns)), rng.uniform(0, 1, m), rng.uniform(-1, 1, ns)
    lp = core.CoreLP.from_inequality_form(a, b, c, constant=0.5)
    if explicit:  # the same LP with its variables renumbered: slacks first
        perm = np.concatenate([ns + np.arange(m), np.arange(ns)])          # new variable -> old variable
        inv = np.argsort(perm)
        lp = core.CoreLP(a=a, c=lp.c[perm], basis=inv[lp.basis], nonbasis=inv[lp.nonbasis], x=lp.x, z=lp.z,
                         var_col=ec.codes_of(lp)[perm], constant=0.5)
    n, old_codes = lp.n, ec.codes_of(lp)
    rows, rhs, cols, c_cols = _blocks(rng, m, ns, p, r)
    got = core.extended_lp(lp, rows=rows, rhs=rhs, cols=cols, c_cols=c_cols)
    assert (got.m, got.n, got.n_struct) == (m + p, n + p + r, ns + r) and got.constant == 0.5
    # the blocks of a', -0.0 read as +0.0
    assert got.a.shape == (m + p, ns + r)
    assert got.a[:m, :ns].tobytes() == np.ascontiguousarray(a).tobytes()
    assert np.array_equal(got.a[m:, :ns], rows) and np.array_equal(got.a[:, ns:], cols)
    assert not np.signbit(got.a[got.a == 0.0]).any()
    assert np.signbit(rows).sum() > np.signbit(got.a[m:, :ns]).sum()      # (the planted -0.0 was there)
    # no existing index changes; the new structural variables, then the new slacks
    assert got.var_col[:n].tolist() == old_codes.tolist()
    assert got.var_col[n:n + r].tolist() == list(range(ns, ns + r))
    assert got.var_col[n + r:].tolist() == [-1 - (m + i) for i in range(p)]
    assert got.c[:n].tobytes() == f64bytes(lp.c) and got.c[n:n + r].tolist() == c_cols.tolist()
    assert (got.c[n + r:] == 0.0).all()
    # positions: the old ones keep their variables, the new slacks and the new variables follow
    assert got.basis.tolist() == list(lp.basis) + list(range(n + r, n + r + p))
    assert got.nonbasis.tolist() == list(lp.nonbasis) + list(range(n, n + r))
    # the slack start of the extended LP
    assert got.x.tolist() == list(b) + list(rhs) and got.z.tolist() == list(lp.z) + list(-c_cols)
    assert got.xbar is None and got.zbar is None
    a2, b2, c2 = ec.inequality_form(got)
    assert np.array_equal(b2, np.concatenate([b, rhs])) and np.array_equal(c2, np.concatenate([c, c_cols]))
    # rows only, columns only
    only_rows = core.extended_lp(lp, rows=rows, rhs=rhs)
    assert (only_rows.m, only_rows.n, only_rows.n_struct) == (m + p, n + p, ns)
    only_cols = core.extended_lp(lp, cols=cols[:m], c_cols=c_cols)
    assert (only_cols.m, only_cols.n, only_cols.n_struct) == (m, n + r, ns + r)
    # two extensions in a row number like one after the other
    twice = core.extended_lp(only_rows, cols=cols, c_cols=c_cols)
    assert twice.var_col[n:n + p].tolist() == [-1 - (m + i) for i in range(p)]
    assert twice.var_col[n + p:].tolist() == list(range(ns, ns + r))
    assert np.array_equal(twice.a, got.a)


def f64bytes(v):
    return np.ascontiguousarray(v, dtype=np.float64).tobytes()


def test_extend_shape_errors_come_before_the_ffi():
    m, ns = 4, 6
    rng = np.random.default_rng(3)
    lp = core.CoreLP.from_inequality_form(rng.random((m, ns)), rng.random(m), rng.random(ns))
    s = core.Solver.__new__(core.Solver)   # a stub: no device, no handle
    s._lp, s._h = lp, None
    bad = [dict(),
           dict(rows=np.zeros((1, ns))),                                   # rows without rhs
           dict(rhs=np.zeros(1)),
           dict(cols=np.zeros((m, 1))),                                    # cols without c_cols
           dict(rows=np.zeros((1, ns - 1)), rhs=np.zeros(1)),
           dict(rows=np.zeros((2, ns)), rhs=np.zeros(1)),
           dict(rows=np.zeros(ns), rhs=np.zeros(1)),
           dict(cols=np.zeros((m + 1, 1)), c_cols=np.zeros(1)),
           dict(rows=np.zeros((1, ns)), rhs=np.zeros(1), cols=np.zeros((m, 1)), c_cols=np.zeros(1)),
           dict(cols=np.zeros((m, 2)), c_cols=np.zeros(1)),
           dict(rows=np.zeros((0, ns)), rhs=np.zeros(0))]
    for kw in bad:
        with pytest.raises(ValueError, match="extend"):
            s.extend(**kw)
        with pytest.raises(ValueError, match="extend"):
            core.extended_lp(lp, **kw)
    assert s._lp is lp
    col_ptr, row_idx, val, bs, cs = core.gen_sparse_lp(seed=3, m=8, n_struct=12, per_col=2)
    with pytest.raises(NotImplementedError, match="extend is not supported"):
        core.extended_lp(core.CoreLP.from_csc(8, col_ptr, row_idx, val, bs, cs), rows=np.zeros((1, 12)),
                         rhs=np.zeros(1))


# ------------------------------------------------------------------ the session, without a device
@pytest.mark.parametrize("name", sorted(ec.ADDED))
def test_session_row_equals_the_builder_on_the_model_written_with_the_constraint(name):
    text, new_b, text_new_b = ec.ADDED[name]
    k = _kat(name)
    ns, problem = build_problem(k)
    env = dict(ns)
    first = _form(problem)
    order = rs.lower(problem._core_objective().to_rust_affexpr(), list(problem.yield_rust_inequalities()))[1]
    session = problem.session()
    # (as if a solver were live: the constraint waits for the next solve instead of joining the model)
    session._solver, session._form, session._order = object(), first, order
    try:
        con = eval(text, {"__builtins__": {}}, env)
        assert session.add_constraints(con) is session
        assert session._added == [con] and session._constraints == problem.constraints
        for written, change in ((text, None), (text_new_b, {con: new_b})):
            if change:
                session._change(None, change)
            rows = session._rows_of(con, first, order)
            want = _form(build_problem(dict(k, constraints=k["constraints"] + [written]))[1])
            assert (want.m, want.n_struct) == (first.m + len(rows), first.n_struct), name
            assert want.pos_var.tolist() == first.pos_var.tolist(), name
            assert want.var_col[want.var_col >= 0].tolist() == first.var_col[first.var_col >= 0].tolist(), name
            at = len(list(problem.yield_rust_inequalities()))   # the builder lists the user rows first
            for j, (row, b) in enumerate(rows):
                assert row.tobytes() == np.ascontiguousarray(want.a[at + j]).tobytes(), (name, written, j)
                assert np.float64(b).tobytes() == np.float64(want.x[at + j]).tobytes(), (name, written, j)
        assert len(rows) == (2 if "==" in text else 1)
    finally:
        session._solver = None


def test_a_repeated_variable_keeps_its_last_coefficient():
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    problem = dz.Maximize(x + y).subject_to(x + y <= 4)
    session = problem.session()
    first = _form(problem)
    order = session._lowered()[2]
    con = x + 2 * y <= 3
    ineq = con.rust_inequalities()[0]
    twice = rs.PyLinExpr.__new__(rs.PyLinExpr)   # x listed twice, as a hand-built expression may
    twice.coefs, twice.vars, twice._slot = [5.0] + list(ineq._linexpr.coefs), [ineq._linexpr.vars[0]] + list(ineq._linexpr.vars), {}

    class _Con:
        _signs = [1.0]

        @staticmethod
        def rust_inequalities():
            return [rs.PyInequality(linexpr=twice, b=3.0)]
    (row, b), = session._rows_of(_Con, first, order)
    arrays, _ = rs.lower(problem._core_objective().to_rust_affexpr(),
                         list(problem.yield_rust_inequalities()) + _Con.rust_inequalities())
    want = rs.standard_form(arrays)
    assert row.tobytes() == np.ascontiguousarray(want.a[1]).tobytes() and b == want.x[1] == 3.0


def test_add_constraints_value_errors():
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    base = x + 2 * y <= 4
    for live in (False, True):
        problem = dz.Maximize(x + y).subject_to(base)
        session = problem.session()
        if live:
            session._solver, session._form, session._order = object(), _form(problem), session._lowered()[2]
        try:
            w = dz.Variable.nonneg()
            with pytest.raises(ValueError, match="not seen"):
                session.add_constraints(x + w <= 1)
            k = dz.Variable(lb=0.0, ub=5.0, integer=True)
            with pytest.raises(ValueError, match="integer"):
                session.add_constraints(x + k <= 1)
            with pytest.raises(ValueError, match="already part"):
                session.add_constraints(base)
            good = x - y <= 1
            with pytest.raises(ValueError, match="already part"):
                session.add_constraints([good, good])
            with pytest.raises(ValueError, match="not seen"):
                session.add_constraints([good, x + w <= 1])            # all or nothing
            assert session._added == [] and session._constraints == [base]
            with pytest.raises(TypeError):
                session.add_constraints("x <= 1")
            session.add_constraints([good])
            with pytest.raises(ValueError, match="already part"):
                session.add_constraints(good)
            assert (session._added if live else session._constraints[1:]) == [good]
        finally:
            session._solver = None
    # an objective over an unseen variable is still refused once a solver exists
    problem = dz.Maximize(x + y).subject_to(base)
    session = problem.session()
    session._solver, session._form, session._order = object(), _form(problem), session._lowered()[2]
    session.add_constraints(x - y <= 1)
    with pytest.raises(ValueError, match="changes the standard form"):
        session.solve(objective=x + y + dz.Variable.nonneg())
    session._solver = None


# ------------------------------------------------------------------ the recipe, against HiGHS
@pytest.mark.parametrize("seed,m,ns", ec.BASES[:2], ids=["24x40", "37x53"])
def test_recipe_cases_stay_optimal_and_move_the_optimum(seed, m, ns):
    a, b, c = ec.base(seed, m, ns)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    status, obj, x_star, y_star = ec.highs(lp)
    assert status == 0
    for p, r, s in ec.RECIPE:
        kw = ec.draw(lp, x_star, y_star, p, r, s)
        if p:
            assert (kw["rows"] @ x_star > kw["rhs"]).all(), (p, r, s)        # the cuts are violated at x*
        if r:
            y_ext = np.concatenate([y_star, np.zeros(p)])
            assert np.allclose(kw["cols"].T @ y_ext - kw["c_cols"], -0.5)    # the columns price out
        status2, obj2, _, _ = ec.highs(core.extended_lp(lp, **kw))
        assert status2 == 0, (p, r, s, status2)
        assert abs(obj2 - obj) > 1e-6 * max(1.0, abs(obj)), (p, r, s, obj, obj2)
        assert (obj2 < obj) if r == 0 else True, (p, r, s)
