"""Host side of the batched FAST solver (dzg_batch_solve_fast / dzg_model_solve_batch_fast): the ABI,
the argument checks that run before any device call, and the Python surface.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import dantzig_amd
from dantzig_amd import _ffi, core
from dantzig_amd import rust as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_fast_batch_entry_points():
    with open(os.path.join(ROOT, "include", "dantzig_amd.h")) as f:
        h = f.read()
    assert "int dzg_batch_solve_fast(const dzg_lp *lps, int64_t count, const dzg_opts *opts," in h
    assert "int64_t pivots_per_launch, int64_t refactor_every, dzg_result *res);" in h
    assert "int dzg_model_solve_batch_fast(const dzg_model *models, int64_t count, const dzg_opts *opts," in h
    assert "#define DZG_ABI_VERSION 4" in h  # additions only: no existing struct changes layout


def test_library_exports_the_fast_batch_entry_points():
    lib = _ffi.lib()
    for name in ("dzg_batch_solve_fast", "dzg_model_solve_batch_fast"):
        assert name in _ffi.EXPORTS
        assert hasattr(lib, name)


def _lp(m=3, ns=4, seed=0):
    rng = np.random.default_rng(seed)
    return core.CoreLP.from_inequality_form(rng.uniform(-1, 1, (m, ns)), rng.uniform(0, 1, m),
                                            rng.uniform(-1, 1, ns))


def _call(lps, res=True, ppl=0, refactor_every=0, **opts):
    """dzg_batch_solve_fast on CoreLPs through ctypes; returns (rc, last error)."""
    marshalled = [core._c_lp(lp) for lp in lps]
    arr = (_ffi.Lp * max(len(lps), 1))(*[c for c, _ in marshalled])
    out = (_ffi.Result * max(len(lps), 1))() if res else None
    o = _ffi.default_opts(**opts)
    rc = _ffi.lib().dzg_batch_solve_fast(arr, C.c_int64(len(lps)), C.byref(o), C.c_int64(ppl),
                                         C.c_int64(refactor_every), out)
    return rc, _ffi.lib().dzg_last_error().decode()


def _csc_lp(m=3, ns=4):
    cp = np.arange(ns + 1, dtype=np.int64)
    ri = np.arange(ns, dtype=np.int32) % m
    return core.CoreLP.from_csc(m, cp, ri, np.ones(ns), np.ones(m), np.ones(ns))


@pytest.mark.parametrize("numerics", [_ffi.FAST, _ffi.AUTO])
@pytest.mark.parametrize("case", ["m129", "csc", "res_null", "bad_var_col", "ppl", "refactor_every"])
def test_fast_batch_rejects_malformed_input_on_any_machine(case, numerics):
    good = [_lp(seed=1), _lp(seed=2)]
    res, kw = True, {}
    if case == "m129":
        lps, bad = good + [_lp(m=129, ns=3)], 2
    elif case == "csc":
        lps, bad = [good[0], _csc_lp()], 1
    elif case == "res_null":
        lps, bad, res = good, None, False
    elif case == "ppl":
        lps, bad, kw = good, None, dict(ppl=-1)
    elif case == "refactor_every":
        lps, bad, kw = good, None, dict(refactor_every=-1)
    else:
        lp = _lp(seed=3)
        lp.var_col = np.array([0, 1, 2, 99, -1, -2, -3], dtype=np.int64)  # column 99 does not exist
        lps, bad = [good[0], good[1], lp], 2
    rc, msg = _call(lps, res=res, numerics=numerics, **kw)
    assert rc == _ffi.E_ARG, (rc, msg)
    if bad is not None:
        assert f"lps[{bad}]" in msg


def test_fast_batch_without_a_gpu_is_a_device_error():
    if _ffi.lib().dzg_device_count() > 0:
        pytest.skip("a GPU is visible: the device path is covered by tests/test_gpu_batch_fast.py")
    for numerics in (_ffi.FAST, _ffi.AUTO, _ffi.STRICT):
        rc, msg = _call([_lp(seed=1), _lp(m=0, ns=2, seed=2)], numerics=numerics)
        assert rc == _ffi.E_DEVICE and "no CPU path" in msg


def _arrays(seed):
    x, y = rs.Variable(lb=0.0, ub=None), rs.Variable(lb=None, ub=2.0)
    obj = rs.PyAffExpr(linexpr=rs.PyLinExpr([1.0, float(seed)], [x, y]), constant=0.0)
    con = rs.PyInequality(linexpr=rs.PyLinExpr([1.0, 1.0], [x, y]), b=3.0)
    return (obj, [con]), rs.lower(obj, [con])[0]


def _model_batch(models, res=True):
    keep = [rs._c_model(a) for a in models]
    arr = (_ffi.Model * max(len(keep), 1))(*keep)
    out = (_ffi.ModelResult * max(len(keep), 1))() if res else None
    return _ffi.lib().dzg_model_solve_batch_fast(arr, C.c_int64(len(keep)), None, out)


def test_fast_model_batch_checks_its_arguments():
    assert _model_batch([_arrays(1)[1], _arrays(2)[1]], res=False) == _ffi.E_ARG
    bad = _arrays(3)[1]
    bad["obj_var"] = np.array([0, 7, 0], dtype=np.int64)  # variable 7 of a two-variable model
    assert _model_batch([_arrays(1)[1], bad]) == _ffi.E_ARG
    assert "models[1]" in _ffi.lib().dzg_last_error().decode()
    assert _model_batch([]) == 0


def test_fast_model_batch_without_a_gpu_is_a_device_error():
    if _ffi.lib().dzg_device_count() > 0:
        pytest.skip("a GPU is visible: the device path is covered by tests/test_gpu_batch_fast.py")
    assert _model_batch([_arrays(1)[1], _arrays(2)[1]]) == _ffi.E_DEVICE
    assert "no CPU path" in _ffi.lib().dzg_last_error().decode()


def test_solve_batch_fast_checks_the_whole_batch_before_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was reached")

    lib = _ffi.lib()
    monkeypatch.setattr(_ffi, "lib", lambda: type("L", (), {"dzg_batch_solve_fast": no_device,
                                                            "dzg_batch_solve": no_device,
                                                            "dzg_opts_default": lib.dzg_opts_default,
                                                            "dzg_device_count": no_device})())
    good = _lp()
    for numerics in (core.FAST, core.AUTO):
        with pytest.raises(ValueError, match="129 rows"):
            core.solve_batch_fast([good, _lp(m=129, ns=2)], numerics=numerics)
        with pytest.raises(ValueError, match="CSC"):
            core.solve_batch_fast([good, _csc_lp()], numerics=numerics)
        a, b, c = np.ones((3, 4)), np.ones(3), np.ones(4)
        with pytest.raises(ValueError, match="column-block"):
            core.solve_batch_fast([good, core.CoreLP.from_inequality_block(a[:, :2], b, c, 0, 2)],
                                  numerics=numerics)
        broken = _lp()
        broken.x = np.ones(5)
        with pytest.raises(ValueError, match="do not match"):
            core.solve_batch_fast([good, broken], numerics=numerics)
    with pytest.raises(ValueError, match="numerics"):
        core.solve_batch_fast([good], numerics=7)
    with pytest.raises(ValueError, match="refactor_every"):
        core.solve_batch_fast([good], refactor_every=-1)
    with pytest.raises(ValueError, match="price_kernel"):
        core.solve_batch_fast([good], price_kernel=core.PRICE_SEQ)
    # untouched: the STRICT batch still refuses FAST
    with pytest.raises(ValueError, match="STRICT"):
        core.solve_batch([good], numerics=core.FAST)


def test_solve_many_fast_does_not_combine_with_postsolve_yet():
    x = dantzig_amd.Variable.nonneg()
    p = dantzig_amd.Maximize(x).subject_to([x <= 1.0])
    for kw in (dict(duals=True), dict(ranging=True), dict(rays=True)):
        with pytest.raises(ValueError, match="fast=True"):
            dantzig_amd.solve_many([p], fast=True, **kw)
    pair = _arrays(1)[0]
    for kw in (dict(duals=True), dict(ranging=True), dict(rays=True)):
        with pytest.raises(ValueError, match="fast=True"):
            rs.solve_many([pair], fast=True, **kw)
    with pytest.raises(TypeError, match="Minimize"):
        dantzig_amd.solve_many([object()], fast=True)
