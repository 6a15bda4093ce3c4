"""Duals, ranging and rays behind a FAST batch (dzg_batch_solve_post, csrc/k_batch_post.hip), the
parts that need no GPU: tests/batch_post_reference.py -- the float64 restatement of the kernel -- held
to long double with the project's rule (error <= C_DUALS x numpy's double-precision error, floor 1e-13;
ranges through planted.check_ranges with no direction skipped); the planted cases the GPU test enters
through start=(basis, nonbasis): the FAST restart state of every optimal plant is optimal (zero
pivots) and that of every ray plant stops at the planted position before its first pivot; the ABI
(struct size against a compiled C probe, version, exports, argtypes); every new DZG_E_ARG path
returns before device work; the Python keyword checks."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from dantzig_amd import _ffi, core
from tests import batch_post_reference as bpr
from tests import planted as pl
from tests import rays_reference as rref
from tests.rays_helpers import LD, dense_ray_vectors, numpy_solve, refined_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_DEVICE = _ffi.E_ARG, _ffi.E_DEVICE
IDS = ["x".join(map(str, s)) for s in bpr.SHAPES]
RAY_IDS = ["x".join(map(str, s)) for s in bpr.RAY_SHAPES]


def _metric(got, want):
    """tests/test_gpu_duals.py's: max |got - want| / max(1, |want|_inf)."""
    want = np.asarray(want, dtype=LD)
    scale = max(1.0, float(np.max(np.abs(want)))) if want.size else 1.0
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - want))) / scale if want.size else 0.0


# ------------------------------------------------------------------ the reference against long double
@pytest.mark.parametrize("shape", bpr.SHAPES, ids=IDS)
def test_reference_duals_and_ranges_against_long_double(shape):
    m, ns, k = shape
    p = bpr.optimal_plant(shape)
    r = bpr.restart_of(p)
    assert not r.singular
    # the restart state is optimal: the solve takes zero pivots and the post-solve reads this state
    assert bpr.status_of(r.x, np.ones(m), r.z, np.ones(ns)) == ("optimal", -1)
    du = bpr.duals(p.a, p.b, p.cc, 0.0, p.basis, p.nonbasis, r.x, r.z)
    y_hat, d_hat = pl.exact_duals(p.a, p.cc, p.basis, p.nonbasis)
    y_np, d_np = pl.numpy_duals(p.a, p.cc, p.basis, p.nonbasis)
    for got, hat, np_, what in ((du.y, y_hat, y_np, "y"), (du.d[p.nonbasis], d_hat, d_np, "d_N")):
        err, base = _metric(got, hat), _metric(np_, hat)
        print(f"\n{shape} {what}: error {err:.3e}, numpy {base:.3e}")
        assert err <= max(pl.C_DUALS * base, pl.FLOOR), (shape, what, err, base)
    assert (du.d[p.basis] == 0.0).all() and du.primal_infeas == 0.0 and du.dual_infeas == 0.0
    assert du.z_diff <= 1e-12
    assert abs(du.dual_obj - float(p.cc[p.basis] @ r.x)) <= 1e-10 * max(1.0, abs(du.dual_obj))
    cost, rhs = pl.unit_and_pair_directions(m, m, m + ns)
    got_c, got_r = bpr.ranges(p.a, p.basis, p.nonbasis, r.x, du.d, du.w, cost, rhs)
    want = pl.reference_sides(p.a, p.basis, p.nonbasis, r.x, d_hat, cost, rhs)
    yard = pl.reference_sides(p.a, p.basis, p.nonbasis, r.x, d_np, cost, rhs, exact=False)
    for got, w, y, variables, name in ((got_c, want[0], yard[0], p.nonbasis, "cost"), (got_r, want[1], yard[1], p.basis, "rhs")):
        out = pl.check_ranges([g.lo for g in got], [g.hi for g in got], [g.lo_var for g in got],
                              [g.hi_var for g in got], w, y, variables, f"{shape} {name}")
        print(f"{shape} {name}: {out['directions']} directions, error {out['err']:.3e} (ratio {out['ratio']:.3f})")
        assert out["skipped"] == 0, (shape, name)  # the reference alone skips none; the cap stays SKIP_CAP


@pytest.mark.parametrize("kind", pl.RAY_KINDS)
@pytest.mark.parametrize("shape", bpr.RAY_SHAPES, ids=RAY_IDS)
def test_reference_rays_against_long_double(shape, kind):
    m, ns, k = shape
    p = bpr.ray_plant(kind, shape)
    primal = kind.startswith("unbounded")
    r = bpr.restart_of(p)
    assert not r.singular
    # the restart from the planted basis stops at the planted position before its first pivot
    assert bpr.status_of(r.x, np.ones(m), r.z, np.ones(ns)) == ("primal" if primal else "dual", p.pos)
    ray = bpr.ray(p.a, p.b, p.cc, p.basis, p.nonbasis, r.x, np.ones(m), r.z, np.ones(ns), primal)
    assert (ray.pos, ray.var, ray.proven, ray.violation) == (p.pos, p.var, True, 0.0)
    code = rref.PRIMAL if primal else rref.FARKAS
    d_hat, y_hat = dense_ray_vectors(p.a, p.basis, p.nonbasis, code, p.pos, refined_solve)
    d_np, y_np = dense_ray_vectors(p.a, p.basis, p.nonbasis, code, p.pos, numpy_solve)
    for got, hat, np_, what in ((ray.d, d_hat, d_np, "d"), (ray.y, y_hat, y_np, "y")):
        err, base = _metric(got, hat), _metric(np_, hat)
        assert err <= max(pl.C_DUALS * base, pl.FLOOR), (shape, kind, what, err, base)
    value_hat = float(p.cc.astype(LD) @ d_hat) if primal else float(np.asarray(p.b, dtype=LD) @ y_hat)
    assert abs(ray.value - value_hat) <= 1e-9 and abs(abs(value_hat) - 1.0) <= 1e-9


def test_reference_takes_the_permutation_path_for_an_all_slack_basis():
    rng = np.random.default_rng(3)
    a, b, c = rng.uniform(-1, 1, (20, 30)), rng.uniform(0.5, 2, 20), -rng.uniform(0.5, 2, 30)
    basis, nonbasis, cc = np.arange(30, 50), np.arange(30), np.concatenate([c, np.zeros(20)])
    du = bpr.duals(a, b, cc, 0.0, basis, nonbasis, b, -c)
    assert (du.w == np.eye(20)).all() and (du.y == 0.0).all() and du.dual_obj == 0.0
    assert (du.d[nonbasis] == -c).all() and du.z_diff == 0.0


# ------------------------------------------------------------------ ABI
def test_struct_size_against_a_compiled_probe(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dantzig_amd.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %d\\n", sizeof(dzg_batch_post), offsetof(dzg_batch_post, du), '
                   'offsetof(dzg_batch_post, req), offsetof(dzg_batch_post, rg), offsetof(dzg_batch_post, ry), '
                   'DZG_ABI_VERSION);\nreturn 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [32, 0, 8, 16, 24, 4]
    assert C.sizeof(_ffi.BatchPost) == 32
    assert [getattr(_ffi.BatchPost, f).offset for f, _ in _ffi.BatchPost._fields_] == [0, 8, 16, 24]


def test_version_exports_and_argtypes():
    lib = _ffi.lib()
    assert lib.dzg_abi_version() == 4
    with open(os.path.join(ROOT, "include", "dantzig_amd.h")) as f:
        header = f.read()
    assert re.search(r"\bint dzg_batch_solve_post\(const dzg_lp \*lps, const dzg_batch_start \*start, int64_t count,",
                     header)
    assert re.search(r"\bint dzg_batch_resolve_post\(dzg_batch \*b, const int64_t \*which, int64_t nwhich,", header)
    assert len(lib.dzg_batch_resolve_post.argtypes) == 5 and len(lib.dzg_batch_resolve.argtypes) == 4
    for name in ("dzg_batch_solve_post", "dzg_debug_batch_post_ms", "dzg_batch_resolve_post"):
        assert name in _ffi.EXPORTS and hasattr(lib, name)
    assert len(lib.dzg_batch_solve_post.argtypes) == 8
    assert lib.dzg_debug_batch_post_ms.restype is C.c_double
    from dantzig_amd import _build
    assert "k_batch_post.hip" in _build.SOURCES


# ------------------------------------------------------------------ argument checks: C ABI
def _lp(seed=1, m=4, ns=6):
    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    return core.CoreLP.from_inequality_form(a, b, c)


def _call_post(lps, post=(True, None, 0.0, False), starts=None, null_post=False, break_post=None, **opts):
    marshalled = [core._c_lp(lp) for lp in lps]
    count = len(lps)
    c_lps = (_ffi.Lp * max(count, 1))(*[c for c, _ in marshalled])
    res = (_ffi.Result * max(count, 1))()
    pb = core._PostBuffers(lps, *post)
    if break_post:
        break_post(pb)
    c_start = None
    if starts is not None:
        c_start = (_ffi.BatchStart * max(count, 1))()
        keep = []
        for i, s in enumerate(starts):
            if s is not None:
                keep.append([_ffi.i64(v) for v in s])
                c_start[i].basis, c_start[i].nonbasis = _ffi.ptr(keep[-1][0]), _ffi.ptr(keep[-1][1])
    o = _ffi.default_opts(**opts)
    rc = _ffi.lib().dzg_batch_solve_post(c_lps, c_start, C.c_int64(count), C.byref(o), C.c_int64(0), C.c_int64(0),
                                         None if null_post else C.byref(pb.c_post), res)
    return rc, _ffi.lib().dzg_last_error().decode()


def _bad_request(field, value):
    def edit(pb):
        buf = pb.bufs[1]
        if field == "pivot_tol":
            pb.c_req[1].pivot_tol = value
        else:
            arr = buf.cost[1] if field == "cost_idx" else buf.rhs[1]
            arr[:len(value)] = value
    return edit


@pytest.mark.parametrize("numerics", [core.FAST, core.AUTO, core.STRICT])
@pytest.mark.parametrize("what,edit,needle", [
    ("cost index out of range", _bad_request("cost_idx", [10]), "lps[1]"),
    ("rhs index out of range", _bad_request("rhs_idx", [4]), "lps[1]"),
    ("negative index", _bad_request("cost_idx", [-1]), "lps[1]"),
    ("negative pivot_tol", _bad_request("pivot_tol", -1e-9), "lps[1]"),
    ("NaN pivot_tol", _bad_request("pivot_tol", float("nan")), "lps[1]"),
], ids=lambda v: v if isinstance(v, str) and " " in v else None)
def test_a_bad_ranging_request_is_e_arg_and_names_the_lp(what, edit, needle, numerics):
    lps = [_lp(1), _lp(2)]
    rc, msg = _call_post(lps, post=(True, True, 0.0, False), break_post=edit, numerics=numerics)
    assert rc == E_ARG and needle in msg, (what, rc, msg)


def test_a_repeated_index_inside_one_direction_is_e_arg():
    lps = [_lp(1), _lp(2)]
    dirs = [([{0: 1.0}], [{0: 1.0}]), ([{1: 1.0, 2: 1.0}], [{0: 1.0}])]

    def edit(pb):
        pb.bufs[1].cost[1][:2] = [1, 1]
    rc, msg = _call_post(lps, post=(False, dirs, 0.0, False), break_post=edit, numerics=core.FAST)
    assert rc == E_ARG and "lps[1]" in msg, msg


def test_req_and_rg_go_together_and_the_old_checks_stay():
    lps = [_lp(1)]

    def no_rg(pb):
        pb.c_post.rg = None

    def no_req(pb):
        pb.c_post.req = None
    for edit in (no_rg, no_req):
        rc, msg = _call_post(lps, post=(True, True, 0.0, False), break_post=edit)
        assert rc == E_ARG and "req and rg" in msg, msg
    rc, msg = _call_post(lps, starts=[(np.array([0, 0, 6, 7]), np.array([1, 2, 3, 4, 5, 8]))])
    assert rc == E_ARG and "lps[0]" in msg and "not a partition" in msg, msg
    big = core.CoreLP.from_inequality_form(np.ones((129, 2)), np.ones(129), np.ones(2))
    rc, msg = _call_post([lps[0], big])
    assert rc == E_ARG and "lps[1]" in msg and "DZG_BATCH_MAX_ROWS" in msg, msg
    lib = _ffi.lib()
    post = _ffi.BatchPost()
    args = (C.c_int64(0), C.c_int64(0), C.byref(post), None)
    assert lib.dzg_batch_solve_post(None, None, C.c_int64(1), None, *args) == E_ARG
    assert lib.dzg_batch_solve_post(None, None, C.c_int64(-1), None, *args) == E_ARG
    assert lib.dzg_batch_solve_post(None, None, C.c_int64(0), None, *args) == 0
    assert lib.dzg_batch_solve_post(None, None, C.c_int64(0), None, C.c_int64(0), C.c_int64(-1), None, None) == E_ARG


@pytest.mark.skipif(_ffi.lib().dzg_device_count() > 0, reason="a device is present: the call would solve")
@pytest.mark.parametrize("numerics", [core.FAST, core.AUTO, core.STRICT])
def test_good_arguments_reach_the_device(numerics):
    lps = [_lp(1), _lp(2)]
    for kw in (dict(null_post=True), dict(post=(False, None, 0.0, False)), dict(post=(True, True, 0.0, True))):
        rc, msg = _call_post(lps, numerics=numerics, **kw)
        assert rc == E_DEVICE, (kw, rc, msg)


# ------------------------------------------------------------------ argument checks: Python
def test_python_keywords_and_their_checks():
    sig = inspect.signature(core.solve_batch_fast).parameters
    assert (sig["duals"].default, sig["ranging"].default, sig["pivot_tol"].default, sig["rays"].default) == \
        (False, False, 0.0, False)
    lps = [_lp(1), _lp(2)]
    with pytest.raises(ValueError, match="one .* request per LP"):
        core.solve_batch_fast(lps, ranging=[(None, None)])
    with pytest.raises(ValueError, match="pivot_tol"):
        core.solve_batch_fast(lps, ranging=True, pivot_tol=-1.0)
    with pytest.raises(ValueError, match="pivot_tol"):
        core.solve_batch_fast(lps, duals=True, pivot_tol=float("nan"))
    with pytest.raises(ValueError, match="start"):
        core.solve_batch_fast(lps, duals=True, start=[None])
    with pytest.raises(ValueError, match="numerics"):
        core.solve_batch_fast(lps, duals=True, numerics=7)


# ------------------------------------------------------------------ the handle
def test_resolve_post_checks_its_arguments_before_device_work():
    lib = _ffi.lib()
    post = _ffi.BatchPost()
    assert lib.dzg_batch_resolve_post(None, None, C.c_int64(0), C.byref(post), None) == E_ARG
    h = C.c_void_p()
    assert lib.dzg_batch_create(None, C.c_int64(0), None, C.c_int64(0), C.c_int64(0), C.c_int64(0), C.byref(h)) == 0
    try:
        assert lib.dzg_batch_resolve_post(h, None, C.c_int64(0), C.byref(post), None) == 0  # an empty handle
        assert lib.dzg_batch_resolve_post(h, None, C.c_int64(0), None, None) == 0
        one = _ffi.i64([0])
        assert lib.dzg_batch_resolve_post(h, _ffi.ptr(one), C.c_int64(-1), C.byref(post), None) == E_ARG
        res = (_ffi.Result * 1)()
        assert lib.dzg_batch_resolve_post(h, _ffi.ptr(one), C.c_int64(1), C.byref(post), res) == E_ARG
        assert "out of range" in lib.dzg_last_error().decode()
    finally:
        lib.dzg_batch_destroy(h)


def test_batch_solver_keywords_and_their_checks():
    sig = inspect.signature(core.BatchSolver.solve).parameters
    assert [sig[k].default for k in ("which", "log", "duals", "ranging", "pivot_tol", "rays")] == \
        [None, True, False, False, 0.0, False]
    import dantzig_amd as dz
    sig = inspect.signature(dz.SessionBatch.solve).parameters
    assert [sig[k].default for k in ("duals", "ranging", "rays")] == [False, False, False]
    assert "sessions(" in dz.solve_many.__doc__
    with pytest.raises(ValueError, match="fast=True"):
        dz.solve_many([], fast=True, duals=True)
