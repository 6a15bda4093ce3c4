"""Sensitivity ranging, the parts that need no GPU: struct layouts, the reference of
tests/ranging_reference.py against long-double numpy, argument checks that precede any device work,
and the Python surface (Solution.rhs_range / objective_range)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi, core, optimize, rust
from oracle import oracle as ora
from tests import duals_reference as dref
from tests import ranging_reference as rref
from tests.lp_families import make_lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _c_model(model: dict):
    """dzg_model of a JSON-style model; returns (struct, arrays to keep alive)."""
    vs, cons = model["vars"], model.get("constraints", [])
    ot = model["objective"]["terms"]
    k = dict(
        has_lb=np.array([v.get("lb") is not None for v in vs] + [0], dtype=np.int32),
        has_ub=np.array([v.get("ub") is not None for v in vs] + [0], dtype=np.int32),
        lb=np.array([v["lb"] if v.get("lb") is not None else 0.0 for v in vs] + [0.0]),
        ub=np.array([v["ub"] if v.get("ub") is not None else 0.0 for v in vs] + [0.0]),
        obj_var=np.array([t[0] for t in ot] + [0], dtype=np.int64),
        obj_coef=np.array([t[1] for t in ot] + [0.0]),
        con_ptr=np.array(np.concatenate([[0], np.cumsum([len(c["terms"]) for c in cons])]), dtype=np.int64),
        con_var=np.array([t[0] for c in cons for t in c["terms"]] + [0], dtype=np.int64),
        con_coef=np.array([t[1] for c in cons for t in c["terms"]] + [0.0]),
        con_b=np.array([c["b"] for c in cons] + [0.0]))
    p = _ffi.ptr
    md = _ffi.Model(len(vs), p(k["has_lb"]), p(k["has_ub"]), p(k["lb"]), p(k["ub"]), len(ot),
                    p(k["obj_var"]), p(k["obj_coef"]), float(model["objective"].get("constant", 0.0)),
                    len(cons), p(k["con_ptr"]), p(k["con_var"]), p(k["con_coef"]), p(k["con_b"]))
    return md, k


def test_struct_layouts_match_the_header(tmp_path):
    structs = {"dzg_ranging_req": _ffi.RangingReq, "dzg_ranging": _ffi.Ranging,
               "dzg_model_ranging_req": _ffi.ModelRangingReq}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dantzig_amd.h"', 'int main(void) {']
    for cname, mirror in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for field, _ in mirror._fields_:
            lines.append(f'printf("{cname}.{field} %zu\\n", offsetof({cname}, {field}));')
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, mirror in structs.items():
        assert int(got[cname]) == C.sizeof(mirror), cname
        for field, _ in mirror._fields_:
            assert int(got[f"{cname}.{field}"]) == getattr(mirror, field).offset, f"{cname}.{field}"


def test_abi_version_stays_4_and_the_new_names_are_exported():
    lib = _ffi.lib()
    assert lib.dzg_abi_version() == 4
    for name in ("dzg_solver_ranging", "dzg_batch_solve_ranging", "dzg_model_solve_ranging",
                 "dzg_model_solve_batch_ranging"):
        assert name in _ffi.EXPORTS and hasattr(lib, name)


# ------------------------------------------------------------------ the reference itself
def test_textbook_reference_values():
    # T1: max 3x + 5y, x <= 4, 2y <= 12, 3x + 2y <= 18: the classic allowable increases / decreases
    sf, res, ref = dref.solve_model_duals(dref.T1)
    rg = rref.CoreRanging(sf, res, ref)
    # variables of the standard form: x+ x- y+ y-, then the slacks in the order they were first seen
    cx = rg.cost({0: 1.0, 1: -1.0})
    cy = rg.cost({2: 1.0, 3: -1.0})
    assert abs(cx.lo + 3.0) <= 1e-12 and abs(cx.hi - 4.5) <= 1e-12       # 3 + t in [0, 7.5]
    assert abs(cy.lo + 3.0) <= 1e-12 and cy.hi == INF                     # 5 + t in [2, inf)
    rows = [rg.rhs({i: 1.0}) for i in range(3)]
    assert abs(rows[0].lo + 2.0) <= 1e-12 and rows[0].hi == INF           # 4 + t in [2, inf)
    assert abs(rows[1].lo + 6.0) <= 1e-12 and abs(rows[1].hi - 6.0) <= 1e-12    # 12 + t in [6, 18]
    assert abs(rows[2].lo + 6.0) <= 1e-12 and abs(rows[2].hi - 6.0) <= 1e-12    # 18 + t in [12, 24]
    for r in [cx, cy] + rows:
        assert r.lo <= 0.0 <= r.hi
        assert (r.lo_var >= 0) == np.isfinite(r.lo) and (r.hi_var >= 0) == np.isfinite(r.hi)


def _optimal_lps(count):
    out, seed = [], 0
    while len(out) < count:
        a, b, c = make_lp(seed, seed % 3, 4, 24)
        sf = ora.stdform_from_dense(a, b, c)
        res = ora.simplex_solve(sf)
        if res.status == "optimal":
            out.append((seed, a, sf, res))
        seed += 1
    return out


def _close(got, want, what):
    assert np.isfinite(got) == np.isfinite(want), (what, got, want)
    if np.isfinite(want):
        assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (what, got, want)
    else:
        assert got == want, (what, got, want)


def test_reference_agrees_with_long_double_numpy():
    checked = 0
    for seed, a, sf, res in _optimal_lps(20):
        m, ns = a.shape
        n = m + ns
        full = np.concatenate([a, np.eye(m)], axis=1)
        duals = dref.core_duals(sf, res)
        rg = rref.CoreRanging(sf, res, duals)
        rng = np.random.default_rng(1000 + seed)
        cost_dirs = [{j: 1.0} for j in range(n)]
        rhs_dirs = [{i: 1.0} for i in range(m)]
        for _ in range(3):
            i, j = rng.choice(n, 2, replace=False)
            cost_dirs.append({int(i): 1.0, int(j): -1.0})
            if m >= 2:
                i, j = rng.choice(m, 2, replace=False)
                rhs_dirs.append({int(i): 1.0, int(j): -1.0})
        want_c, want_r = rref.long_double_ranges(full[:, res.basis], full[:, res.nonbasis], res.basis,
                                                 res.nonbasis, res.x, duals.d[res.nonbasis], cost_dirs, rhs_dirs)
        for d, w in zip(cost_dirs, want_c):
            g = rg.cost(d)
            _close(g.lo, w.lo, (seed, "cost lo", d))
            _close(g.hi, w.hi, (seed, "cost hi", d))
            assert g.lo <= 0.0 <= g.hi
            checked += 1
        for d, w in zip(rhs_dirs, want_r):
            g = rg.rhs(d)
            _close(g.lo, w.lo, (seed, "rhs lo", d))
            _close(g.hi, w.hi, (seed, "rhs hi", d))
            assert g.lo <= 0.0 <= g.hi
            checked += 1
    assert checked >= 400


def test_first_position_wins_a_tie():
    r = rref.ratio_rule([2.0, 1.0, 2.0, 0.0], [1.0, 0.5, -1.0, 1e-10], [7, 8, 9, 10], 1e-9)
    assert (r.lo, r.lo_var, r.hi, r.hi_var) == (-2.0, 7, 2.0, 9)
    none = rref.ratio_rule([1.0], [1e-10], [3], 1e-9)
    assert (none.lo, none.hi, none.lo_var, none.hi_var) == (-INF, INF, -1, -1)


# ------------------------------------------------------------------ argument checks
def _tiny_lp():
    """max x st x <= 1 as a dzg_lp: m = 1, n = 2."""
    keep = dict(a=np.array([1.0]), c=np.array([1.0, 0.0]), basis=np.array([1], dtype=np.int64),
                nonbasis=np.array([0], dtype=np.int64), x=np.array([1.0]), z=np.array([-1.0]))
    lp = _ffi.Lp()
    lp.m, lp.n, lp.n_struct, lp.lda = 1, 2, 1, 1
    lp.a, lp.c = _ffi.ptr(keep["a"]), _ffi.ptr(keep["c"])
    lp.basis, lp.nonbasis = _ffi.ptr(keep["basis"]), _ffi.ptr(keep["nonbasis"])
    lp.x, lp.z = _ffi.ptr(keep["x"]), _ffi.ptr(keep["z"])
    return lp, keep


def _req(cost_ptr=(0,), cost_idx=(), cost_val=(), rhs_ptr=(0,), rhs_idx=(), rhs_val=(), tol=0.0):
    keep = [_ffi.i64(list(cost_ptr)), _ffi.i64(list(cost_idx) + [0]), _ffi.f64(list(cost_val) + [0.0]),
            _ffi.i64(list(rhs_ptr)), _ffi.i64(list(rhs_idx) + [0]), _ffi.f64(list(rhs_val) + [0.0])]
    r = _ffi.RangingReq()
    r.ncost, r.nrhs, r.pivot_tol = len(cost_ptr) - 1, len(rhs_ptr) - 1, tol
    r.cost_ptr, r.cost_idx, r.cost_val = (_ffi.ptr(k) for k in keep[:3])
    r.rhs_ptr, r.rhs_idx, r.rhs_val = (_ffi.ptr(k) for k in keep[3:])
    return r, keep


def _batch(lp, req, res=None, rg=None):
    res = _ffi.Result() if res is None else res
    rg = _ffi.Ranging() if rg is None else rg
    return _ffi.lib().dzg_batch_solve_ranging(C.byref(lp), C.c_int64(1), None, C.c_int64(0),
                                              C.byref(req) if req is not None else None, C.byref(res), None,
                                              C.byref(rg) if rg is not False else None)


def test_argument_errors_come_before_any_device_work():
    lib, E_ARG = _ffi.lib(), _ffi.E_ARG
    good, keep_good = _req((0, 1), (0,), (1.0,), (0, 1), (0,), (1.0,))
    out = _ffi.Ranging()
    # NULL pointers
    assert lib.dzg_solver_ranging(None, C.byref(good), None, C.byref(out)) == E_ARG
    lp, keep_lp = _tiny_lp()
    assert _batch(lp, None) == E_ARG
    assert _batch(lp, good, rg=False) == E_ARG
    assert lib.dzg_batch_solve_ranging(None, C.c_int64(1), None, C.c_int64(0), C.byref(good), None, None,
                                       C.byref(out)) == E_ARG
    assert lib.dzg_batch_solve_ranging(None, C.c_int64(-1), None, C.c_int64(0), None, None, None, None) == E_ARG
    no_ptr, k0 = _req((0, 1), (0,), (1.0,))
    no_ptr.cost_ptr = None
    assert _batch(lp, no_ptr) == E_ARG and "cost_ptr" in lib.dzg_last_error().decode()
    no_idx, k1 = _req(rhs_ptr=(0, 1), rhs_idx=(0,), rhs_val=(1.0,))
    no_idx.rhs_idx = None
    assert _batch(lp, no_idx) == E_ARG
    # pivot_tol
    for tol in (-1e-9, float("nan")):
        bad, k2 = _req((0, 1), (0,), (1.0,), tol=tol)
        assert _batch(lp, bad) == E_ARG and "pivot_tol" in lib.dzg_last_error().decode()
    # duplicate indices in one direction (the same index in two directions is fine)
    dup, k3 = _req((0, 2), (1, 1), (1.0, -1.0))
    assert _batch(lp, dup) == E_ARG and "repeated" in lib.dzg_last_error().decode()
    # out of range: a variable >= n, a row >= m, a negative index, a pointer array that decreases
    for bad, k4 in (_req((0, 1), (2,), (1.0,)), _req(rhs_ptr=(0, 1), rhs_idx=(1,), rhs_val=(1.0,)),
                    _req((0, 1), (-1,), (1.0,)), _req((0, 2, 1), (0, 1), (1.0, 1.0))):
        assert _batch(lp, bad) == E_ARG, lib.dzg_last_error().decode()
    # the model level: NULLs, a variable that appears nowhere, a row out of range, a repeated row
    md, keep_md = _c_model(dref.T1)
    mres, mdu, con = _ffi.ModelResult(), _ffi.ModelDuals(), np.zeros(3)
    mdu.con_dual = _ffi.ptr(con)

    def mreq(var=(), row_ptr=(0,), row_idx=(), row_coef=(), tol=0.0):
        keep = [_ffi.i64(list(var) + [0]), _ffi.i64(list(row_ptr)), _ffi.i64(list(row_idx) + [0]),
                _ffi.f64(list(row_coef) + [0.0])]
        r = _ffi.ModelRangingReq()
        r.nvar, r.nrow, r.pivot_tol = len(var), len(row_ptr) - 1, tol
        r.var, r.row_ptr, r.row_idx, r.row_coef = (_ffi.ptr(k) for k in keep)
        return r, keep

    def model_call(md_, req):
        return lib.dzg_model_solve_ranging(C.byref(md_), None, C.byref(req), C.byref(mres), C.byref(mdu),
                                           C.byref(out))

    ok, k5 = mreq((0, 1), (0, 1), (2,), (1.0,))
    assert lib.dzg_model_solve_ranging(C.byref(md), None, None, C.byref(mres), C.byref(mdu), C.byref(out)) == E_ARG
    assert lib.dzg_model_solve_ranging(C.byref(md), None, C.byref(ok), C.byref(mres), None, C.byref(out)) == E_ARG
    assert lib.dzg_model_solve_ranging(C.byref(md), None, C.byref(ok), C.byref(mres), C.byref(mdu), None) == E_ARG
    for bad, k6 in (mreq((2,)), mreq((-1,)), mreq((), (0, 1), (3,), (1.0,)), mreq((), (0, 2), (1, 1), (1.0, -1.0)),
                    mreq((0,), tol=-1.0)):
        assert model_call(md, bad) == E_ARG, lib.dzg_last_error().decode()
    # a user variable that appears nowhere in the model
    lonely = dict(dref.T1, vars=[dref.NN, dref.NN, dref.NN])
    lmd, keep_l = _c_model(lonely)
    nowhere, k7 = mreq((2,))
    assert model_call(lmd, nowhere) == E_ARG and "appears nowhere" in lib.dzg_last_error().decode()
    assert lib.dzg_model_solve_batch_ranging(C.byref(lmd), C.c_int64(1), None, C.byref(nowhere), C.byref(mres),
                                             C.byref(mdu), C.byref(out)) == E_ARG
    assert lib.dzg_model_solve_batch_ranging(C.byref(md), C.c_int64(1), None, None, C.byref(mres),
                                             C.byref(mdu), C.byref(out)) == E_ARG


def test_device_entry_points_fail_loudly_without_gpu():
    if _ffi.lib().dzg_device_count() > 0:
        pytest.skip("a GPU is visible")
    lib = _ffi.lib()
    lp, keep_lp = _tiny_lp()
    good, keep_good = _req((0, 1), (0,), (1.0,), (0, 1), (0,), (1.0,))
    assert _batch(lp, good) == _ffi.E_DEVICE
    md, keep_md = _c_model(dref.T1)
    mres, mdu, con, out = _ffi.ModelResult(), _ffi.ModelDuals(), np.zeros(3), _ffi.Ranging()
    mdu.con_dual = _ffi.ptr(con)
    var = _ffi.i64([0, 1])
    req = _ffi.ModelRangingReq()
    req.nvar, req.var = 2, _ffi.ptr(var)
    assert lib.dzg_model_solve_ranging(C.byref(md), None, C.byref(req), C.byref(mres), C.byref(mdu),
                                       C.byref(out)) == _ffi.E_DEVICE
    assert lib.dzg_model_solve_batch_ranging(C.byref(md), C.c_int64(1), None, C.byref(req), C.byref(mres),
                                             C.byref(mdu), C.byref(out)) == _ffi.E_DEVICE
    x = dz.Variable.nonneg()
    with pytest.raises(_ffi.DantzigAmdError, match="no HIP device"):
        dz.Maximize(x).subject_to(x <= 1.0).solve(ranging=True)
    with pytest.raises(_ffi.DantzigAmdError):
        core.solve_batch([core.CoreLP.from_inequality_form(np.ones((1, 1)), np.ones(1), np.ones(1))],
                         ranging=True)


# ------------------------------------------------------------------ the Python surface
def _hand_made(order, var_lo, var_hi, group_lo, group_hi):
    ids = [v.to_rust_variable().id for v in order]
    ranging = rust.PyRanging(var_lo=dict(zip(ids, var_lo)), var_hi=dict(zip(ids, var_hi)),
                             var_lo_var={i: -1 for i in ids}, var_hi_var={i: -1 for i in ids},
                             group_lo=list(group_lo), group_hi=list(group_hi),
                             group_lo_var=[-1] * len(group_lo), group_hi_var=[-1] * len(group_lo))
    sol = rust.PySolution(1.0, {})
    sol.ranging = ranging
    return sol


def test_surface_senses_and_errors():
    x, y, w = dz.Variable.nonneg(), dz.Variable.nonneg(), dz.Variable.nonneg()
    le, ge, eq = x + y <= 4.0, x - y >= 1.0, x + 2 * y == 3.0
    stranger = x <= 9.0
    objective = (3 * x - 2 * y).to_affexpr()
    for sense in ("maximize", "minimize"):
        sol = optimize.Solution(solution=_hand_made([x, y], [-1.0, -INF], [0.5, 2.0], [-1.0, -2.0, -INF],
                                                    [3.0, INF, 0.25]),
                                sense=sense, constraints=[le, ge, eq], objective=objective)
        # t is the change of the constraint's own b, whatever its form and the sense
        assert sol.rhs_range(le) == optimize.Range(3.0, 7.0)
        assert sol.rhs_range(ge) == optimize.Range(-1.0, INF)
        assert sol.rhs_range(eq) == optimize.Range(-INF, 3.25)
        if sense == "maximize":
            assert sol.objective_range(x) == optimize.Range(2.0, 3.5)
            assert sol.objective_range(y) == optimize.Range(-INF, 0.0)
        else:  # the core's coefficient is the negated one: negate and swap
            assert sol.objective_range(x) == optimize.Range(2.5, 4.0)
            assert sol.objective_range(y) == optimize.Range(-4.0, INF)
        with pytest.raises(KeyError):
            sol.rhs_range(stranger)
        with pytest.raises(KeyError):
            sol.objective_range(w)
    plain = optimize.Solution(solution=rust.PySolution(1.0, {}), sense="maximize", constraints=[le])
    for call in (lambda: plain.rhs_range(le), lambda: plain.objective_range(x)):
        with pytest.raises(RuntimeError, match=r"solve\(ranging=True\)"):
            call()


def test_row_groups_follow_the_constraints_signs():
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    le, ge, eq = x + y <= 4.0, x - y >= 1.0, x + 2 * y == 3.0
    p = dz.Maximize(x).subject_to([le, ge, eq, le])
    assert p._row_groups() == [[(0, 1.0)], [(1, -1.0)], [(2, 1.0), (3, -1.0)]]


def test_integer_models_have_no_ranges():
    k = dz.Variable.integer(lb=0.0, ub=3.0)
    with pytest.raises(ValueError, match="integer"):
        dz.Maximize(k).subject_to(k <= 2.5).solve(ranging=True)
    with pytest.raises(ValueError, match="integer"):
        optimize.solve_many([dz.Maximize(k).subject_to(k <= 2.5)], ranging=True)


def test_unsupported_route_is_not_implemented(monkeypatch):
    class FakeLib:
        def dzg_last_error(self):
            return b"ranging is not supported on CSC storage or sharded solvers"

        def dzg_status_str(self, code):
            return b"bad_argument"

    monkeypatch.setattr(_ffi, "lib", lambda: FakeLib())
    with pytest.raises(NotImplementedError, match="not supported"):
        _ffi.check_ranging(_ffi.E_ARG, "dzg_solver_ranging")
    assert _ffi.check_ranging(0, "dzg_solver_ranging") == 0
