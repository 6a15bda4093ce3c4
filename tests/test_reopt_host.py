"""Re-optimisation from the current basis (dzg_solver_reoptimize, core.Solver.reoptimize,
Optimize.session), the parts that need no GPU: the entry point and its mirror, the argument checks
that run before any device work, the session's pure-Python rebuilding of a changed model against the
library's builder on a model written with the new numbers, and the control of the constant the GPU
test holds the FAST restart state to."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi, core
from dantzig_amd import rust as rs
from oracle import oracle as ora
from tests import reopt_check as rc
from tests import state_check as sc
from tests.test_surface import PY_KATS, build_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the C entry point
def test_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "dantzig_amd.h")).read()
    assert "int dzg_solver_reoptimize(dzg_solver *s, const dzg_reopt *chg);" in text
    assert "#define DZG_ABI_VERSION 4" in text
    assert "dzg_solver_reoptimize" in _ffi.EXPORTS
    assert hasattr(_ffi.lib(), "dzg_solver_reoptimize")
    assert _ffi.lib().dzg_abi_version() == 4


def test_mirror_layout_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dantzig_amd.h"', 'int main(void) {',
             'printf("dzg_reopt %zu\\n", sizeof(dzg_reopt));']
    for field, _ in _ffi.Reopt._fields_:
        lines.append(f'printf("dzg_reopt.{field} %zu\\n", offsetof(dzg_reopt, {field}));')
    lines += ['return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["dzg_reopt"]) == C.sizeof(_ffi.Reopt) == 32
    assert [f for f, _ in _ffi.Reopt._fields_] == ["rhs", "c", "constant", "set_constant", "reserved"]
    for field, _ in _ffi.Reopt._fields_:
        assert int(got[f"dzg_reopt.{field}"]) == getattr(_ffi.Reopt, field).offset, field


def test_null_and_empty_changes_are_argument_errors_on_the_host():
    lib = _ffi.lib()
    chg = _ffi.Reopt(None, None, 0.0, 0, 0)
    assert lib.dzg_solver_reoptimize(None, C.byref(chg)) == _ffi.E_ARG
    assert lib.dzg_solver_reoptimize(None, None) == _ffi.E_ARG
    assert b"NULL" in lib.dzg_last_error()
    with pytest.raises(_ffi.DantzigAmdError):
        _ffi.check_reopt(lib.dzg_solver_reoptimize(None, None), "dzg_solver_reoptimize")


def test_check_reopt_maps_the_unsupported_routes():
    class _Lib:
        @staticmethod
        def dzg_last_error():
            return b"reoptimize is not supported on CSC storage or sharded solvers"

        @staticmethod
        def dzg_status_str(code):
            return b"invalid_argument"
    real = _ffi._lib
    _ffi.lib()
    try:
        _ffi._lib = _Lib()
        with pytest.raises(NotImplementedError, match="reoptimize is not supported"):
            _ffi.check_reopt(_ffi.E_ARG, "dzg_solver_reoptimize")
    finally:
        _ffi._lib = real


def test_solver_has_reoptimize_with_a_docstring():
    assert "dzg_solver_reoptimize" in core.Solver.reoptimize.__doc__


# ------------------------------------------------------------------ the session, without a device
def test_session_solve_without_gpu_fails_loudly():
    if _ffi.lib().dzg_device_count() > 0:
        pytest.skip("a GPU is visible")
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    session = dz.Maximize(x + y).subject_to(x + 2 * y <= 4).session()
    with pytest.raises(_ffi.DantzigAmdError):
        session.solve()


def test_session_refuses_integer_models_and_unknown_constraints():
    x, k = dz.Variable.nonneg(), dz.Variable(lb=0.0, ub=5.0, integer=True)
    with pytest.raises(ValueError, match="integer"):
        dz.Maximize(x + k).subject_to(x + k <= 3.5).session()
    con = x <= 4
    session = dz.Maximize(x).subject_to(con).session()
    with pytest.raises(KeyError):
        session._change(None, {x <= 5: 1.0})
    with pytest.raises(TypeError):
        session._change(None, {con: "1"})


# Changed models, as (name of the KAT, {index of the constraint: new b of its normal form}, the
# constraints written with the new numbers, the new objective or None).  ==, >=, <=, bounded, free
# and non-positive variables, a constraint with variables on both sides.
CHANGES = [
    ("problem_2", {1: 2.5, 2: 4.0}, ["y <= 5", "x >= y + 2.5", "y == 4.0"], "3 * x - 1.5 * y + 4"),
    ("non_standard_variables", {0: 3.5, 2: -0.75}, ["y == 3.5", "-3.0 <= x <= 3.0", "z >= -0.75"],
     "2 * x + y + 0.5 * z"),
    ("inventory_balance", {0: 60.0, 2: 110.0, 5: -90.0},
     ["x_1 >= 60", "x_2 + z_1 >= 75", "x_3 + z_2 >= 110", "z_1 == x_1 - 50", "z_2 == x_2 + z_1 - 75",
      "z_3 == x_3 + z_2 - 90"], None),
    ("readme_quick_start", {0: 2.0}, ["x + y + z == 2"], "x + 2 * y - 3 * z"),
    ("problem_3", {0: 0.0}, ["x + y + z <= 0"], None),
]


def _kat(name):
    return next(k for k in PY_KATS if k["name"] == name)


def _form(problem):
    arrays, _ = rs.lower(problem._core_objective().to_rust_affexpr(), list(problem.yield_rust_inequalities()))
    return rs.standard_form(arrays)


def _assert_same_form(got, want, what):
    assert (got.m, got.n, got.n_struct) == (want.m, want.n, want.n_struct), what
    for name in ("a", "var_col", "c", "basis", "nonbasis", "x", "z", "pos_var", "neg_var"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, g, w)
    assert np.float64(got.constant).tobytes() == np.float64(want.constant).tobytes(), what


@pytest.mark.parametrize("name,new_b,written,objective", CHANGES, ids=[c[0] for c in CHANGES])
def test_session_lowering_equals_the_builder_on_the_written_model(name, new_b, written, objective):
    k = _kat(name)
    ns, problem = build_problem(k)
    session = problem.session()
    new_objective = None if objective is None else eval(objective, {"__builtins__": {}}, dict(ns))
    session._change(new_objective, {problem.constraints[i]: b for i, b in new_b.items()})
    got = rs.standard_form(session._lowered()[1])
    ns2, written_problem = build_problem(dict(k, constraints=written, objective=objective or k["objective"]))
    want = _form(written_problem)
    _assert_same_form(got, want, name)
    # ... and only b, c and the constant moved: the live solver can take the change
    first = _form(build_problem(k)[1])
    assert got.same_shape_as(first), name
    assert got.x.tobytes() != first.x.tobytes(), name


def test_session_rhs_speaks_about_the_normal_form_b():
    """The b a session takes is the b Solution.rhs_range reports: signs[0] * the first row's b."""
    k = _kat("inventory_balance")
    _, problem = build_problem(k)
    con = problem.constraints[3]  # z_1 == x_1 - 50
    assert con._signs[0] * con.rust_inequalities()[0]._b == -50.0
    session = problem.session()
    session._change(None, {con: -45.0})
    rows = session._inequalities()
    first = sum(len(c.rust_inequalities()) for c in problem.constraints[:3])
    assert (rows[first]._b, rows[first + 1]._b) == (-45.0, 45.0)
    assert rows[first]._linexpr is con.rust_inequalities()[0]._linexpr


def test_an_objective_over_an_unseen_variable_changes_the_standard_form():
    k = _kat("problem_2")
    ns, problem = build_problem(k)
    session = problem.session()
    first = rs.standard_form(session._lowered()[1])
    w = dz.Variable.nonneg()
    session._change(2 * ns["x"] - 2 * ns["y"] + w, None)
    assert not rs.standard_form(session._lowered()[1]).same_shape_as(first)
    # through solve(): refused before the device is asked for anything once a solver exists
    session2 = problem.session()
    session2._solver, session2._form, session2._order = object(), first, session2._lowered()[2]
    with pytest.raises(ValueError, match="changes the standard form"):
        session2.solve(objective=2 * ns["x"] - 2 * ns["y"] + w)
    assert session2._objective is problem.objective  # the refused change is not kept
    session2._solver = None


# ------------------------------------------------------------------ the constant of the FAST restart state
def test_restart_constant_rejects_one_entry_off_by_1e_10():
    """C_RESTART accepts the exact restart state rounded to double and rejects it with a relative error
    of 1e-10 planted in one entry of x or of z."""
    assert rc.C_RESTART is not None and rc.C_RESTART_OBSERVED, "C_RESTART has not been measured"
    assert rc.C_RESTART == pytest.approx(10 * max(rc.C_RESTART_OBSERVED.values()), rel=0.25)
    for seed, m, ns in ((11, 37, 53), (12, 24, 40)):
        a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
        a = np.ascontiguousarray(a)
        res = ora.simplex_solve(ora.stdform_from_dense(a, b, c))
        assert res.status == "optimal"
        b2, c2 = rc.moved(seed, b, c)
        ex = sc.exact_state(a, ns, rc.slack_start(a, b2, c2), res.basis, res.nonbasis)
        good = ex.rounded()
        assert rc.restart_drift(ex, good)["D"] <= 1e-3 * rc.C_RESTART
        for name in ("x", "z"):
            bad = {key: np.array(val, copy=True) for key, val in good.items()}
            i = int(np.argmax(np.abs(bad[name])))
            assert abs(bad[name][i]) >= 1.0, (seed, name)
            bad[name][i] *= 1.0 + 1e-10
            assert rc.restart_drift(ex, bad)["D"] > rc.C_RESTART, (seed, name, rc.restart_drift(ex, bad))
