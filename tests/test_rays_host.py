"""Unboundedness and infeasibility rays, the parts that need no GPU: the reference
(tests/rays_reference.py) over the integer families with the verdicts it can and cannot prove, the
map to the user's model on random small models (dzg_model_map_ray against the reference, and the
properties a proven ray must have there), struct layouts, argument checks that precede any device
work, and the Python surface."""
import ctypes as C
import functools
import inspect
import os
import subprocess

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi, core, optimize, rust
from oracle import oracle as ora
from tests import rays_reference as rref
from tests.duals_helpers import assert_bit_equal, random_problem
from tests.lp_families import make_lp
from tests.rays_helpers import LD, check_model_ray
from tests.test_duals_host import _c_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_DUALS = 32.0  # tests/test_gpu_duals.py


def _metric(v, ref):  # tests/test_gpu_duals.py
    v, ref = np.asarray(v, dtype=LD), np.asarray(ref, dtype=LD)
    return float(np.abs(v - ref).max(initial=0.0) / max(LD(1), np.abs(ref).max(initial=0.0)))


# ------------------------------------------------------------------ 1. the reference's rays
# (status, proven) counts over seeds 0..199 of make_lp(seed, kind, 4, 48), and the seeds whose
# UNBOUNDED verdict the ray does not prove
COUNTS = {1: {("unbounded", True): 153, ("unbounded", False): 1, ("infeasible", True): 20},
          2: {("unbounded", True): 32, ("unbounded", False): 8, ("infeasible", False): 13}}
UNPROVEN_UNBOUNDED = {1: [194], 2: [4, 55, 67, 78, 80, 165, 181, 183]}
NAN_SEEDS = {1: [194], 2: [183]}


@functools.lru_cache(maxsize=None)
def integer_family_rays():
    """(kind, seed, a, standard form, oracle result, RefRay or None) for kinds 1 and 2, seeds 0..199,
    computed once (tests/test_gpu_rays.py reads it too)."""
    out = []
    for kind in (1, 2):
        for seed in range(200):
            a, b, c = make_lp(seed, kind, 4, 48)
            sf = ora.stdform_from_dense(a, b, c)
            res = ora.simplex_solve(sf)
            out.append((kind, seed, a, sf, res, rref.core_ray(sf, res)))
    return out


def test_reference_rays_over_the_integer_families():
    counts = {1: {}, 2: {}}
    unproven = {1: [], 2: []}
    worst = 0.0
    for kind, seed, a, sf, res, ray in integer_family_rays():
        if ray is None:
            assert res.status not in ("unbounded", "infeasible")
            continue
        key = (res.status, ray.proven)
        counts[kind][key] = counts[kind].get(key, 0) + 1
        if res.status == "unbounded" and not ray.proven:
            unproven[kind].append(seed)
        if res.status == "unbounded":
            assert np.isnan(ray.violation) == (seed in NAN_SEEDS[kind]), (kind, seed)
        if not ray.proven:
            continue
        # the equalities in long double, against what numpy's double solve of the same system leaves
        m, ns = a.shape
        full = np.concatenate([a, np.eye(m)], axis=1)
        full_ld = full.astype(LD)
        bmat = full[:, res.basis]
        d_np = np.zeros(m + ns)
        if ray.kind == rref.PRIMAL:
            d_np[ray.var] = 1.0
            d_np[res.basis] = -np.linalg.solve(bmat, full[:, ray.var])
            resid = full_ld @ ray.d.astype(LD)
            resid_np = full_ld @ d_np.astype(LD)
        else:
            y_np = np.linalg.solve(bmat.T, np.eye(m)[ray.pos])
            d_np[res.nonbasis] = full[:, res.nonbasis].T @ y_np
            d_np[ray.var] = 1.0
            resid = full_ld.T @ ray.y.astype(LD) - ray.d.astype(LD)
            resid_np = full_ld.T @ y_np.astype(LD) - d_np.astype(LD)
        zero = np.zeros(len(resid))
        err, err_np = _metric(resid, zero), _metric(resid_np, zero)
        tol = max(C_DUALS * err_np, 1e-13)
        worst = max(worst, err / tol)
        assert err <= tol, (kind, seed, err, err_np)
    print(f"\nlargest residual / bound over the proven rays: {worst:.3f}")
    assert counts == COUNTS, counts
    assert unproven == UNPROVEN_UNBOUNDED, unproven


# ------------------------------------------------------------------ 2, 3. the model mapping
N_MODELS = 600


@functools.lru_cache(maxsize=None)
def _model_rays():
    """(JSON model, standard form, RefRay) of the random models that end unbounded or infeasible."""
    rng = np.random.default_rng(2026)
    out = []
    for _ in range(N_MODELS):
        _, problem = random_problem(rng, int(rng.integers(0, 12)))
        model = rref.json_model(problem)
        sf, res, ray = rref.solve_model_ray(model)
        if ray is not None:
            out.append((model, sf, ray))
    return out


def test_proven_rays_hold_in_the_models_terms():
    kinds = {rref.PRIMAL: 0, rref.FARKAS: 0}
    worst = 0.0
    for i, (model, sf, ray) in enumerate(_model_rays()):
        if not ray.proven:
            continue
        kinds[ray.kind] += 1
        mr = rref.model_ray(model, ray.kind, ray.d, ray.y)
        worst = max(worst, check_model_ray(model, ray.kind, mr.var, mr.con, mr.lb, mr.ub, ray.value,
                                           f"model ray {i}"))
    print(f"\nproven rays: {kinds}, largest sign miss {worst:.3e}")
    assert kinds[rref.PRIMAL] >= 100 and kinds[rref.FARKAS] >= 100, kinds


def _map(model: dict, kind: int, d, y):
    md, keep = _c_model(model)
    nv, nc = len(model["vars"]), len(model.get("constraints", []))
    out = dict(var=np.full(max(nv, 1), np.nan), con=np.full(max(nc, 1), np.nan),
               lb=np.full(max(nv, 1), np.nan), ub=np.full(max(nv, 1), np.nan))
    ry = _ffi.ModelRay()
    ry.var, ry.con, ry.lb, ry.ub = (_ffi.ptr(out[k]) for k in ("var", "con", "lb", "ub"))
    d = np.ascontiguousarray(d, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    rc = _ffi.lib().dzg_model_map_ray(C.byref(md), C.c_int32(kind), _ffi.ptr(d), _ffi.ptr(y),
                                      C.c_int64(len(y)), C.c_int64(len(d)), C.byref(ry))
    return rc, out["var"][:nv], out["con"][:nc], out["lb"][:nv], out["ub"][:nv]


def test_map_ray_equals_the_reference_bit_for_bit():
    rays = _model_rays()
    assert len(rays) >= 200
    for i, (model, sf, ray) in enumerate(rays):
        want = rref.model_ray(model, ray.kind, ray.d, ray.y)
        rc, var, con, lb, ub = _map(model, ray.kind, ray.d, ray.y)
        assert rc == 0, i
        for got, exp, what in ((var, want.var, "var"), (con, want.con, "con"), (lb, want.lb, "lb"),
                               (ub, want.ub, "ub")):
            assert_bit_equal(got, exp, f"model ray {i} {what}")


# ------------------------------------------------------------------ 4. ABI
NAMES = ("dzg_solver_ray", "dzg_batch_solve_rays", "dzg_model_solve_rays", "dzg_model_solve_batch_rays",
         "dzg_model_map_ray")


def test_abi_version_stays_4_and_the_new_names_are_exported():
    lib = _ffi.lib()
    assert lib.dzg_abi_version() == 4
    for name in NAMES:
        assert name in _ffi.EXPORTS and hasattr(lib, name)


def test_struct_layouts_match_the_header(tmp_path):
    structs = {"dzg_ray": _ffi.Ray, "dzg_model_ray": _ffi.ModelRay}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dantzig_amd.h"', 'int main(void) {']
    for cname, mirror in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for field, _ in mirror._fields_:
            lines.append(f'printf("{cname}.{field} %zu\\n", offsetof({cname}, {field}));')
    lines += ['printf("PRIMAL %d\\n", DZG_RAY_PRIMAL);', 'printf("FARKAS %d\\n", DZG_RAY_FARKAS);',
              'printf("ABI %d\\n", DZG_ABI_VERSION);', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, mirror in structs.items():
        assert int(got[cname]) == C.sizeof(mirror), cname
        for field, _ in mirror._fields_:
            assert int(got[f"{cname}.{field}"]) == getattr(mirror, field).offset, f"{cname}.{field}"
    assert (int(got["PRIMAL"]), int(got["FARKAS"])) == (_ffi.RAY_PRIMAL, _ffi.RAY_FARKAS) == (1, 2)
    assert int(got["ABI"]) == 4


# max x + y st x - y <= 1: unbounded
T_UNBOUNDED = {"vars": [{"lb": 0.0, "ub": None}] * 2,
               "objective": {"terms": [[0, 1.0], [1, 1.0]], "constant": 0.0},
               "constraints": [{"terms": [[0, 1.0], [1, -1.0]], "b": 1.0}]}


def test_argument_errors_come_before_any_device_work():
    lib = _ffi.lib()
    E_ARG = _ffi.E_ARG
    ry, mry, res, mres = _ffi.Ray(), _ffi.ModelRay(), _ffi.Result(), _ffi.ModelResult()
    assert lib.dzg_solver_ray(None, C.byref(ry)) == E_ARG
    assert lib.dzg_batch_solve_rays(None, C.c_int64(-1), None, C.c_int64(0), None, None, None) == E_ARG
    assert lib.dzg_model_solve_batch_rays(None, C.c_int64(-1), None, None, None, None) == E_ARG
    md, keep = _c_model(T_UNBOUNDED)
    arrays = [np.zeros(2) for _ in range(4)]
    mry.var, mry.con, mry.lb, mry.ub = (_ffi.ptr(a) for a in arrays)
    assert lib.dzg_model_solve_rays(C.byref(md), None, C.byref(mres), None, None) == E_ARG
    assert lib.dzg_model_solve_rays(C.byref(md), None, None, None, C.byref(mry)) == E_ARG
    assert lib.dzg_model_solve_rays(None, None, C.byref(mres), None, C.byref(mry)) == E_ARG
    assert lib.dzg_model_solve_batch_rays(C.byref(md), C.c_int64(1), None, C.byref(mres), None, None) == E_ARG
    assert lib.dzg_model_solve_batch_rays(C.byref(md), C.c_int64(1), None, None, None, C.byref(mry)) == E_ARG
    hollow = _ffi.ModelRay()  # no arrays
    assert lib.dzg_model_solve_rays(C.byref(md), None, C.byref(mres), None, C.byref(hollow)) == E_ARG
    assert lib.dzg_model_solve_batch_rays(C.byref(md), C.c_int64(1), None, C.byref(mres), None,
                                          C.byref(hollow)) == E_ARG
    # dzg_model_map_ray: the standard form has m = 3 rows (one user row, two bounds) and n = 7 variables
    d, y = np.zeros(7), np.zeros(3)
    args = lambda kind, dd, yy, m, n, out: (C.byref(md), C.c_int32(kind), dd, yy, C.c_int64(m),  # noqa: E731
                                            C.c_int64(n), out)
    assert lib.dzg_model_map_ray(*args(1, _ffi.ptr(d), _ffi.ptr(y), 3, 7, C.byref(mry))) == 0
    assert lib.dzg_model_map_ray(*args(1, _ffi.ptr(d), None, 3, 7, C.byref(mry))) == 0  # y optional for PRIMAL
    assert lib.dzg_model_map_ray(*args(2, _ffi.ptr(d), _ffi.ptr(y), 3, 7, C.byref(mry))) == 0
    assert lib.dzg_model_map_ray(*args(2, _ffi.ptr(d), None, 3, 7, C.byref(mry))) == E_ARG
    assert lib.dzg_model_map_ray(*args(0, _ffi.ptr(d), _ffi.ptr(y), 3, 7, C.byref(mry))) == E_ARG
    assert lib.dzg_model_map_ray(*args(1, None, _ffi.ptr(y), 3, 7, C.byref(mry))) == E_ARG
    assert lib.dzg_model_map_ray(*args(1, _ffi.ptr(d), _ffi.ptr(y), 2, 7, C.byref(mry))) == E_ARG
    assert lib.dzg_model_map_ray(*args(1, _ffi.ptr(d), _ffi.ptr(y), 3, 6, C.byref(mry))) == E_ARG
    assert lib.dzg_model_map_ray(*args(1, _ffi.ptr(d), _ffi.ptr(y), 3, 7, None)) == E_ARG
    assert lib.dzg_model_map_ray(*args(1, _ffi.ptr(d), _ffi.ptr(y), 3, 7, C.byref(hollow))) == E_ARG
    # a batch whose LP is malformed, and one without an output array
    lp = _ffi.Lp()
    lp.m, lp.n, lp.n_struct = 2, 1, 0
    assert lib.dzg_batch_solve_rays(C.byref(lp), C.c_int64(1), None, C.c_int64(0), C.byref(res), None,
                                    C.byref(ry)) == E_ARG
    assert lib.dzg_batch_solve_rays(C.byref(lp), C.c_int64(1), None, C.c_int64(0), C.byref(res), None,
                                    None) == E_ARG


def test_device_entry_points_fail_loudly_without_gpu():
    if _ffi.lib().dzg_device_count() > 0:
        pytest.skip("a GPU is visible")
    md, keep = _c_model(T_UNBOUNDED)
    mres, mry = _ffi.ModelResult(), _ffi.ModelRay()
    arrays = [np.zeros(2) for _ in range(4)]
    mry.var, mry.con, mry.lb, mry.ub = (_ffi.ptr(a) for a in arrays)
    assert _ffi.lib().dzg_model_solve_rays(C.byref(md), None, C.byref(mres), None, C.byref(mry)) == _ffi.E_DEVICE
    assert _ffi.lib().dzg_model_solve_batch_rays(C.byref(md), C.c_int64(1), None, C.byref(mres), None,
                                                 C.byref(mry)) == _ffi.E_DEVICE


# ------------------------------------------------------------------ 5. the Python surface
def test_exceptions_carry_no_ray_unless_asked():
    assert dz.exceptions.SolveError().ray is None
    assert dz.exceptions.UnboundedError("x").ray is None and dz.exceptions.InfeasibleError("x").ray is None


def test_rays_is_in_the_signatures():
    for fn in (dz.Maximize.solve, dz.Minimize.solve, dz.solve_many, optimize.solve_many, rust.solve,
               rust.solve_many, core.solve_batch):
        p = inspect.signature(fn).parameters.get("rays")
        assert p is not None and p.default is False, fn
    assert callable(core.Solver.ray)


def test_value_errors_come_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")

    monkeypatch.setattr(_ffi, "require_gpu", no_device)
    monkeypatch.setattr(_ffi, "lib", no_device)
    k = dz.Variable.integer(lb=0.0, ub=3.0)
    x = dz.Variable.nonneg()
    with pytest.raises(ValueError, match="integer"):
        dz.Maximize(k).subject_to(k <= 2.5).solve(rays=True)
    with pytest.raises(ValueError, match="integer"):
        dz.solve_many([dz.Maximize(x).subject_to(x <= 1.0), dz.Maximize(k).subject_to(k <= 2.5)], rays=True)
    with pytest.raises(ValueError, match="ranging"):
        dz.Maximize(x).subject_to(x <= 1.0).solve(rays=True, ranging=True)
    with pytest.raises(ValueError, match="ranging"):
        dz.solve_many([dz.Maximize(x).subject_to(x <= 1.0)], rays=True, ranging=True)
    with pytest.raises(ValueError, match="ranging"):
        rust.solve(*dz.Maximize(x).subject_to(x <= 1.0)._rust_problem(), rays=True, ranging=True)
    with pytest.raises(ValueError, match="ranging"):
        core.solve_batch([], rays=True, ranging=True)


def _hand_made(kind, proven, value, violation, order, var, con, lb=None, ub=None):
    ids = [v.to_rust_variable().id for v in order]
    return rust.PyRay(kind=kind, proven=proven, value=value, violation=violation, mu=0.5,
                      var=dict(zip(ids, var)), con=list(con), lb=dict(zip(ids, lb or [0.0] * len(ids))),
                      ub=dict(zip(ids, ub or [0.0] * len(ids))))


def test_surface_senses_and_signs():
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    le, ge, eq = x + y <= 4.0, x - y >= 1.0, x + 2 * y == 3.0
    stranger = x <= 9.0
    rows = [0.5, 2.0, 7.0, 3.0]  # le; ge (negated row); eq (as written, negated)
    for cls, flip in ((dz.Maximize, 1.0), (dz.Minimize, -1.0)):
        problem = cls(x + y).subject_to([le, ge, eq])
        exc = dz.exceptions.UnboundedError("u")
        exc.ray = _hand_made("primal", True, 2.0, 0.0, [x, y], [1.0, 3.0], rows)
        ray = problem._wrap_ray(exc).ray
        assert isinstance(ray, optimize.PrimalRay) and ray.proven and ray.violation == 0.0
        assert ray.objective_rate == flip * 2.0
        assert (ray.direction(x), ray.direction(y)) == (1.0, 3.0)
        assert ray.direction(dz.Variable.nonneg()) == 0.0
        assert ray.slack_rate(eq) == [7.0, 3.0]
        exc = dz.exceptions.InfeasibleError("i")
        exc.ray = _hand_made("farkas", False, -1.5, 0.25, [x, y], [0.0, 1e-17], rows, lb=[0.0, 2.0],
                             ub=[1.0, 0.0])
        ray = problem._wrap_ray(exc).ray
        assert isinstance(ray, optimize.FarkasRay) and not ray.proven and ray.violation == 0.25
        assert ray.rhs_value == -1.5  # no objective in it: the same under both senses
        assert ray.multiplier(le) == 0.5 and ray.multiplier(ge) == -2.0 and ray.multiplier(eq) == 7.0 - 3.0
        assert ray.bound_multipliers(x) == (0.0, 1.0) and ray.bound_multipliers(y) == (2.0, 0.0)
        assert ray.aggregated(y) == 1e-17
        with pytest.raises(KeyError):
            ray.multiplier(stranger)
        plain = dz.exceptions.InfeasibleError("p")
        assert problem._wrap_ray(plain).ray is None
