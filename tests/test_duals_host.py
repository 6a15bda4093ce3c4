"""Dual values and reduced costs, the parts that need no GPU: struct layouts, the host-only map from
the standard form's dual vector to the user's model (dzg_model_map_duals) against
tests/duals_reference.py, argument checks that precede any device work, and the signs of the
Python surface (Solution.dual / reduced_cost / certificate)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi, optimize, rust
from oracle import oracle as ora
from tests import duals_reference as dref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _map(model: dict, y):
    md, keep = _c_model(model)
    nv, nc = len(model["vars"]), len(model.get("constraints", []))
    out = dict(con=np.full(max(nc, 1), np.nan), rc=np.full(max(nv, 1), np.nan),
               lb=np.full(max(nv, 1), np.nan), ub=np.full(max(nv, 1), np.nan))
    du = _ffi.ModelDuals()
    du.con_dual, du.var_rc, du.lb_dual, du.ub_dual = (_ffi.ptr(out[k]) for k in ("con", "rc", "lb", "ub"))
    y = np.ascontiguousarray(y, dtype=np.float64)
    rc = _ffi.lib().dzg_model_map_duals(C.byref(md), _ffi.ptr(y), C.c_int64(len(y)), C.byref(du))
    return rc, out["con"][:nc], out["rc"][:nv], out["lb"][:nv], out["ub"][:nv]


def test_struct_layouts_match_the_header(tmp_path):
    structs = {"dzg_duals": _ffi.Duals, "dzg_model_duals": _ffi.ModelDuals}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dantzig_amd.h"', 'int main(void) {']
    for cname, mirror in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for field, _ in mirror._fields_:
            lines.append(f'printf("{cname}.{field} %zu\\n", offsetof({cname}, {field}));')
    lines += ['printf("FRESH %d\\n", DZG_DUALS_FRESH);', 'printf("CARRIED %d\\n", DZG_DUALS_CARRIED);',
              'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, mirror in structs.items():
        assert int(got[cname]) == C.sizeof(mirror), cname
        for field, _ in mirror._fields_:
            assert int(got[f"{cname}.{field}"]) == getattr(mirror, field).offset, f"{cname}.{field}"
    assert (int(got["FRESH"]), int(got["CARRIED"])) == (_ffi.DUALS_FRESH, _ffi.DUALS_CARRIED) == (1, 2)


def test_abi_version_stays_4_and_the_new_names_are_exported():
    lib = _ffi.lib()
    assert lib.dzg_abi_version() == 4
    for name in ("dzg_solver_duals", "dzg_batch_solve_duals", "dzg_model_solve_duals",
                 "dzg_model_solve_batch_duals", "dzg_model_map_duals"):
        assert name in _ffi.EXPORTS and hasattr(lib, name)


def _models():
    with open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")) as f:
        kats = json.load(f)["solver"]
    out = [(k["name"], k["model"]) for k in kats if k["expect"]["status"] == "optimal"]
    return out + [(name, model) for name, (model, _) in dref.TEXTBOOK.items()]


@pytest.mark.parametrize("name,model", _models(), ids=[n for n, _ in _models()])
def test_map_duals_agrees_with_the_reference(name, model):
    sf, res, ref = dref.solve_model_duals(model)
    assert res.status == "optimal"
    want = dref.model_duals(model, ref.y)
    rc, con, var_rc, lb, ub = _map(model, ref.y)
    assert rc == 0
    for got, exp, what in ((con, want.con_dual, "con_dual"), (lb, want.lb_dual, "lb_dual"),
                           (ub, want.ub_dual, "ub_dual")):
        assert got.tobytes() == exp.tobytes(), (name, what, got, exp)
    assert np.abs(var_rc - want.var_rc).max(initial=0.0) <= 1e-12, (name, var_rc, want.var_rc)
    # the certificate the reference composes: strong duality and feasibility of both sides
    assert abs(ref.dual_obj - res.objective) <= 1e-12 * max(1.0, abs(res.objective))
    assert ref.primal_infeas <= 1e-12 and ref.dual_infeas <= 1e-12 and ref.z_diff <= 1e-12


def test_textbook_values():
    # T1: max 3x + 5y, x <= 4, 2y <= 12, 3x + 2y <= 18
    sf, res, ref = dref.solve_model_duals(dref.T1)
    assert res.objective == 36.0
    rc, con, var_rc, lb, ub = _map(dref.T1, ref.y)
    assert np.abs(con - [0.0, 1.5, 1.0]).max() <= 1e-12 and np.abs(var_rc).max() <= 1e-12
    # T2 (core sense: the negated minimisation): user's duals (1.5, 0.5) are the core's y here
    sf, res, ref = dref.solve_model_duals(dref.T2)
    assert res.objective == -9.0
    rc, con, var_rc, lb, ub = _map(dref.T2, ref.y)
    assert np.abs(con - [1.5, 0.5]).max() <= 1e-12
    # T3: max x + 2y, x + y == 3, 0 <= y <= 2
    sf, res, ref = dref.solve_model_duals(dref.T3)
    assert res.objective == 5.0
    rc, con, var_rc, lb, ub = _map(dref.T3, ref.y)
    assert abs((con[0] - con[1]) - 1.0) <= 1e-12
    assert abs(var_rc[1] - 1.0) <= 1e-12 and abs(ub[1] - 1.0) <= 1e-12 and abs(var_rc[0]) <= 1e-12


def test_argument_errors_come_before_any_device_work():
    lib = _ffi.lib()
    E_ARG = _ffi.E_ARG
    du, mdu, res, mres = _ffi.Duals(), _ffi.ModelDuals(), _ffi.Result(), _ffi.ModelResult()
    assert lib.dzg_solver_duals(None, C.byref(du)) == E_ARG
    assert lib.dzg_batch_solve_duals(None, C.c_int64(-1), None, C.c_int64(0), None, None) == E_ARG
    assert lib.dzg_model_solve_batch_duals(None, C.c_int64(-1), None, None, None) == E_ARG
    md, keep = _c_model(dref.T1)
    con = np.zeros(3)
    mdu.con_dual = _ffi.ptr(con)
    assert lib.dzg_model_solve_duals(C.byref(md), None, C.byref(mres), None) == E_ARG
    assert lib.dzg_model_solve_duals(C.byref(md), None, None, C.byref(mdu)) == E_ARG
    assert lib.dzg_model_solve_batch_duals(C.byref(md), C.c_int64(1), None, C.byref(mres), None) == E_ARG
    # a model the validator rejects: a term that names a variable out of range
    bad = json.loads(json.dumps(dref.T1))
    bad["constraints"][0]["terms"][0][0] = 7
    bmd, bkeep = _c_model(bad)
    assert lib.dzg_model_solve_duals(C.byref(bmd), None, C.byref(mres), C.byref(mdu)) == E_ARG
    assert lib.dzg_model_solve_batch_duals(C.byref(bmd), C.c_int64(1), None, C.byref(mres), C.byref(mdu)) == E_ARG
    y = np.zeros(5)
    assert lib.dzg_model_map_duals(C.byref(bmd), _ffi.ptr(y), C.c_int64(5), C.byref(mdu)) == E_ARG
    assert lib.dzg_model_map_duals(C.byref(md), _ffi.ptr(y), C.c_int64(4), C.byref(mdu)) == E_ARG  # m is 5
    assert lib.dzg_model_map_duals(C.byref(md), _ffi.ptr(y), C.c_int64(5), None) == E_ARG
    assert lib.dzg_model_map_duals(C.byref(md), _ffi.ptr(y), C.c_int64(5), C.byref(mdu)) == 0
    # a batch whose LP is malformed, and one without an output array
    lp = _ffi.Lp()
    lp.m, lp.n, lp.n_struct = 2, 1, 0
    assert lib.dzg_batch_solve_duals(C.byref(lp), C.c_int64(1), None, C.c_int64(0), C.byref(res),
                                     C.byref(du)) == E_ARG
    assert lib.dzg_batch_solve_duals(C.byref(lp), C.c_int64(1), None, C.c_int64(0), C.byref(res), None) == E_ARG


def test_device_entry_points_fail_loudly_without_gpu():
    if _ffi.lib().dzg_device_count() > 0:
        pytest.skip("a GPU is visible")
    md, keep = _c_model(dref.T1)
    mres, mdu = _ffi.ModelResult(), _ffi.ModelDuals()
    con = np.zeros(3)
    mdu.con_dual = _ffi.ptr(con)
    assert _ffi.lib().dzg_model_solve_duals(C.byref(md), None, C.byref(mres), C.byref(mdu)) == _ffi.E_DEVICE
    assert _ffi.lib().dzg_model_solve_batch_duals(C.byref(md), C.c_int64(1), None, C.byref(mres),
                                                  C.byref(mdu)) == _ffi.E_DEVICE


# ------------------------------------------------------------------ the Python surface's signs
def _hand_made(con_dual, var_rc, primal, dual, order):
    duals = rust.PyDuals(source="fresh", con_dual=list(con_dual),
                         var_rc={v.to_rust_variable().id: r for v, r in zip(order, var_rc)},
                         lb_dual={}, ub_dual={}, primal_objective=primal, dual_objective=dual,
                         primal_infeasibility=0.0, dual_infeasibility=0.0, z_diff=0.25)
    return rust.PySolution(primal, {}, duals=duals)


def test_surface_signs():
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    le, ge, eq = x + y <= 4.0, x - y >= 1.0, x + 2 * y == 3.0
    stranger = x <= 9.0
    rows = [0.5, 2.0, 7.0, 3.0]  # le; ge (negated row); eq (as written, negated)
    for sense, flip in (("maximize", 1.0), ("minimize", -1.0)):
        sol = optimize.Solution(solution=_hand_made(rows, [1.25, -0.5], 10.0, 9.0, [x, y]), sense=sense,
                                constraints=[le, ge, eq])
        assert sol.dual(le) == flip * 0.5
        assert sol.dual(ge) == flip * -2.0
        assert sol.dual(eq) == flip * (7.0 - 3.0)
        assert sol.reduced_cost(x) == flip * 1.25 and sol.reduced_cost(y) == flip * -0.5
        cert = sol.certificate
        assert cert.source == "fresh" and cert.z_diff == 0.25
        assert (cert.primal_objective, cert.dual_objective, cert.gap) == (flip * 10.0, flip * 9.0, flip * 1.0)
        assert cert.primal_infeasibility == 0.0 and cert.dual_infeasibility == 0.0
        with pytest.raises(KeyError):
            sol.dual(stranger)
    plain = optimize.Solution(solution=rust.PySolution(1.0, {}), sense="maximize")
    for call in (lambda: plain.dual(le), lambda: plain.reduced_cost(x), lambda: plain.certificate):
        with pytest.raises(RuntimeError, match=r"solve\(duals=True\)"):
            call()


def test_integer_models_have_no_duals():
    k = dz.Variable.integer(lb=0.0, ub=3.0)
    with pytest.raises(ValueError, match="integer"):
        dz.Maximize(k).subject_to(k <= 2.5).solve(duals=True)
    with pytest.raises(ValueError, match="integer"):
        optimize.solve_many([dz.Maximize(k).subject_to(k <= 2.5)], duals=True)
