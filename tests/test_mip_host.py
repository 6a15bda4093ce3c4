"""Integer variables without a GPU: the reference branch and bound (tests/mip_reference.py) against
exhaustive enumeration, the dzg_mip_* ABI, every DZG_E_ARG path of dzg_mip_solve, and the Python
surface (integer=, binary(), integer(), .is_integer, routing of LP models)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi
from dantzig_amd import rust as rs
from tests import mip_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_branch_and_bound_equals_enumeration():
    rng = np.random.default_rng(11)
    finished = 0
    for i in range(50):
        md, flags = mr.random_pure_milp(rng)
        got = mr.branch_and_bound(md, flags)
        if got["status"] not in ("optimal", "infeasible"):
            assert got["failed_node"] >= 0  # a node LP hit a reference panic path: the search stops
            continue
        finished += 1
        want = mr.enumerate_optimum(md)
        if want is None:
            assert got["status"] == "infeasible", i
        else:
            assert got["status"] == "optimal", i
            assert abs(got["objective"] - want) <= 1e-9 * max(1.0, abs(want)), (i, got["objective"], want)
            assert all(abs(got["values"][u] - round(got["values"][u])) <= 1e-6 for u in range(len(flags)))
    assert finished >= 40


def test_reference_branch_and_bound_against_scipy_milp():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(12)
    for _ in range(20):
        md, flags = mr.random_pure_milp(rng)
        got = mr.branch_and_bound(md, flags)
        if got["status"] != "optimal":
            continue
        nv = len(md["vars"])
        c = np.zeros(nv)
        for u, k in md["objective"]["terms"]:
            c[u] = -k
        a = np.zeros((len(md["constraints"]), nv))
        for r, con in enumerate(md["constraints"]):
            for u, k in con["terms"]:
                a[r, u] = k
        b = [con["b"] for con in md["constraints"]]
        bounds = opt.Bounds([v["lb"] for v in md["vars"]], [v["ub"] for v in md["vars"]])
        res = opt.milp(c, constraints=opt.LinearConstraint(a, -np.inf, b), integrality=np.ones(nv),
                       bounds=bounds)
        assert res.success
        want = -res.fun + md["objective"]["constant"]
        assert abs(got["objective"] - want) <= 1e-6


def test_reference_branching_rule():
    # most fractional first, ties to the lower index; integral within int_tol
    assert mr.branch_choice([0.5, 1.5, 2.2], [0, 1, 2], 1e-6) == (0, 0.5, False)
    assert mr.branch_choice([1.0, 2.0 + 1e-7], [0, 1], 1e-6) == (-1, 0.0, True)
    assert mr.branch_choice([1.1, 3.4, 0.0], [0, 1, 2], 1e-6) == (1, 3.4, False)


def _header():
    with open(os.path.join(ROOT, "include", "dantzig_amd.h")) as f:
        return f.read()


def test_mip_abi_declared_and_exported():
    h = _header()
    assert "DZG_NODE_LIMIT = 8," in h
    assert "#define DZG_ABI_VERSION 4" in h
    assert ("int dzg_mip_solve(const dzg_model *model, const int32_t *is_integer, const dzg_opts *opts,"
            in h)
    lib = _ffi.lib()
    for name in ("dzg_mip_solve", "dzg_mip_opts_default"):
        assert name in _ffi.EXPORTS and hasattr(lib, name)
    assert _ffi.NODE_LIMIT == 8 and _ffi.status_str(_ffi.NODE_LIMIT) == "node_limit"


def _c_fields(h, name):
    body = re.search(r"typedef struct \{([^{}]*?)\} " + name + ";", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = re.match(r"(\w+\s*\**)\s*(.*)", decl).groups()
        for n in names.split(","):
            fields.append(n.strip().lstrip("*"))
    return fields


@pytest.mark.parametrize("name,cls,size", [("dzg_mip_opts", _ffi.MipOpts, 48),
                                           ("dzg_mip_node", _ffi.MipNode, 56),
                                           ("dzg_mip_result", _ffi.MipResult, 136)])
def test_mip_struct_layouts_match_the_header(name, cls, size):
    assert _c_fields(_header(), name) == [f for f, _ in cls._fields_]
    assert C.sizeof(cls) == size


def test_mip_opts_defaults():
    o = _ffi.default_mip_opts()
    assert (o.node_limit, o.nodes_per_round, o.pivots_per_launch) == (0, 0, 0)
    assert (o.int_tol, o.abs_gap, o.rel_gap) == (1e-6, 1e-9, 0.0)
    with pytest.raises(TypeError):
        _ffi.default_mip_opts(bogus=1)


def _mip_rc(md=True, is_int=True, res=True, log=False, opts=None, **mo):
    arrays = mr.c_arrays({"vars": [{"lb": 0.0, "ub": 3.0}], "objective": {"terms": [[0, 1.0]]},
                          "constraints": [{"terms": [[0, 2.0]], "b": 3.0}]})
    model = rs._c_model(arrays)
    flags = np.array([1, 0], dtype=np.int32)
    r = _ffi.MipResult()
    if log:
        r.log_cap = 4  # no buffer
    o = _ffi.default_opts(**(opts or {}))
    m = _ffi.default_mip_opts(**mo)
    rc = _ffi.lib().dzg_mip_solve(C.byref(model) if md else None, _ffi.ptr(flags) if is_int else None,
                                  C.byref(o), C.byref(m), C.byref(r) if res else None)
    return rc, _ffi.lib().dzg_last_error().decode()


@pytest.mark.parametrize("case", [
    dict(md=False), dict(is_int=False), dict(res=False), dict(log=True),
    dict(int_tol=float("nan")), dict(int_tol=-1e-6), dict(abs_gap=-1.0), dict(rel_gap=float("nan")),
    dict(nodes_per_round=-1), dict(node_limit=-5), dict(pivots_per_launch=-1),
    dict(opts=dict(numerics=_ffi.FAST)),
])
def test_mip_solve_argument_errors_before_any_device_work(case):
    rc, msg = _mip_rc(**case)
    assert rc == _ffi.E_ARG, (rc, msg)
    assert msg.startswith("mip:"), msg


def test_mip_solve_without_a_gpu_is_a_device_error():
    if _ffi.lib().dzg_device_count() > 0:
        pytest.skip("a GPU is visible: the device path is covered by tests/test_gpu_mip.py")
    rc, _ = _mip_rc()
    assert rc == _ffi.E_DEVICE


def test_integer_variables_on_the_surface():
    x = dz.Variable(lb=0.0, ub=4.0, integer=True, name="x")
    b = dz.Variable.binary()
    k = dz.Variable.integer(lb=-2.0, ub=None)
    c = dz.Variable.nonneg()
    assert (x.is_integer, b.is_integer, k.is_integer, c.is_integer) == (True, True, True, False)
    assert (b.lb, b.ub) == (0.0, 1.0) and (k.lb, k.ub) == (-2.0, None)
    assert dz.Variable.integer().lb == 0.0 and dz.Variable.integer().ub is None
    assert repr(x).endswith("integer=True)") and "integer" not in repr(c)
    rv = rs.Variable(lb=None, ub=None, integer=True)
    assert rv.is_integer and repr(rv).endswith("integer=True)")
    assert not rs.Variable(lb=None, ub=None).is_integer
    with pytest.raises(AttributeError):
        x.is_integer = False
    assert issubclass(dz.exceptions.MipLimitWarning, UserWarning)


def test_lp_models_keep_the_lp_path(monkeypatch):
    calls = []
    monkeypatch.setattr(rs, "solve", lambda *a: calls.append("lp") or rs.PySolution(0.0, {}))
    monkeypatch.setattr(rs, "solve_mip", lambda *a, **k: calls.append("mip") or rs.PySolution(0.0, {}))
    x, y = dz.Variable.nonneg(), dz.Variable(lb=0.0, ub=2.0)
    sol = dz.Maximize(x + y).subject_to(x + y <= 3).solve()
    assert calls == ["lp"] and sol.mip is None
    n = dz.Variable.integer()
    dz.Maximize(x + n).subject_to(x + n <= 3).solve()
    assert calls == ["lp", "mip"]


def test_set_mip_options_validates_names():
    rs.set_mip_options(nodes_per_round=7)
    try:
        assert rs._mip_options == {"nodes_per_round": 7}
        with pytest.raises(TypeError):
            rs.set_mip_options(numerics=0)
    finally:
        rs.set_mip_options()
    assert rs._mip_options == {}


@pytest.mark.parametrize("bound", [("ub", float("inf")), ("lb", float("-inf")), ("ub", float("nan"))])
def test_mip_solve_rejects_non_finite_flagged_integer_bounds(bound):
    side, value = bound
    var = {"lb": 0.0, "ub": 3.0}
    var[side] = value
    arrays = mr.c_arrays({"vars": [var, {"lb": 0.0, "ub": float("inf")}],
                          "objective": {"terms": [[0, 1.0], [1, 1.0]]},
                          "constraints": [{"terms": [[0, 2.0], [1, 1.0]], "b": 3.0}]})
    model = rs._c_model(arrays)
    r = _ffi.MipResult()
    flags = np.array([1, 0, 0], dtype=np.int32)  # the continuous variable's +inf ub is not checked
    rc = _ffi.lib().dzg_mip_solve(C.byref(model), _ffi.ptr(flags), None, None, C.byref(r))
    assert rc == _ffi.E_ARG
    assert "integer variable 0" in _ffi.lib().dzg_last_error().decode()
