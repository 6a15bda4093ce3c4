"""Warm-started branch and bound without a GPU: the warm_start option through the C ABI and the
Python surface, and the warm reference search (tests/mip_warm_reference.py) against the cold one
(tests/mip_reference.py): same answers, far fewer LP pivots, and the false optimum a warm start can
produce is caught by the sign check and restarted."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from dantzig_amd import _ffi
from dantzig_amd import rust as rs
from tests import mip_reference as mr
from tests import mip_warm_reference as mw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mip_bench():
    spec = importlib.util.spec_from_file_location("mip_bench", os.path.join(ROOT, "tools", "mip_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _models():
    """tests/test_gpu_mip.py's 40 models: 16 pure, then 24 mixed."""
    rng = np.random.default_rng(2024)
    out = [mr.random_pure_milp(rng) for _ in range(16)]
    out += [mr.random_mixed_milp(rng) for _ in range(24)]
    return out


# ---------------------------------------------------------------- option plumbing
def test_warm_start_option_names():
    assert _ffi.default_mip_opts().warm_start == 0
    assert _ffi.default_mip_opts(warm_start=1).warm_start == 1
    assert _ffi.default_mip_opts(warm_start=True).warm_start == 1
    for name in ("reserved0", "warm", "bogus"):
        with pytest.raises(TypeError):
            _ffi.default_mip_opts(**{name: 1})
    rs.set_mip_options(warm_start=True)
    try:
        assert rs._mip_options == {"warm_start": True}
        with pytest.raises(TypeError):
            rs.set_mip_options(reserved0=1)
        assert rs._mip_options == {"warm_start": True}
    finally:
        rs.set_mip_options()
    assert rs._mip_options == {}
    info = rs.MipInfo(status="optimal")
    assert info.nodes_warm is None and info.nodes_restarted is None
    assert {"nodes_warm", "nodes_restarted"} <= set(rs.MipInfo.__slots__)


def _mip_rc(**mo):
    arrays = mr.c_arrays({"vars": [{"lb": 0.0, "ub": 3.0}], "objective": {"terms": [[0, 1.0]]},
                          "constraints": [{"terms": [[0, 2.0]], "b": 3.0}]})
    model = rs._c_model(arrays)
    flags = np.array([1, 0], dtype=np.int32)
    r = _ffi.MipResult()
    o = _ffi.default_opts()
    m = _ffi.default_mip_opts(**mo)
    rc = _ffi.lib().dzg_mip_solve(C.byref(model), _ffi.ptr(flags), C.byref(o), C.byref(m), C.byref(r))
    return rc, _ffi.lib().dzg_last_error().decode()


@pytest.mark.parametrize("value", [2, -1])
def test_warm_start_out_of_range_is_an_argument_error(value):
    rc, msg = _mip_rc(warm_start=value)
    assert rc == _ffi.E_ARG, (rc, msg)
    assert msg.startswith("mip:") and "warm_start" in msg, msg


def test_struct_sizes_are_unchanged_and_warm_stats_layout():
    assert C.sizeof(_ffi.MipOpts) == 48
    assert C.sizeof(_ffi.MipNode) == 56
    assert C.sizeof(_ffi.MipResult) == 136
    assert _ffi.MipOpts.warm_start.offset == 12 and _ffi.MipOpts.warm_start.size == 4
    assert _ffi.MipOpts.pivots_per_launch.offset == 16
    assert C.sizeof(_ffi.MipWarmStats) == 32
    assert [(f, getattr(_ffi.MipWarmStats, f).offset) for f, _ in _ffi.MipWarmStats._fields_] == [
        ("nodes_warm", 0), ("nodes_restarted", 8), ("warm_iterations", 16), ("restart_iterations", 24)]
    with open(os.path.join(ROOT, "include", "dantzig_amd.h")) as f:
        h = f.read()
    assert "#define DZG_MIP_WARM_TOL 1e-9" in h
    assert "int32_t warm_start;" in h and "reserved0;\n    int64_t pivots_per_launch" not in h
    assert "#define DZG_ABI_VERSION 4" in h
    assert mw.WARM_TOL == 1e-9


def test_last_warm_stats_exists_and_zero_fills():
    lib = _ffi.lib()
    assert "dzg_mip_last_warm_stats" in _ffi.EXPORTS and hasattr(lib, "dzg_mip_last_warm_stats")
    _mip_rc(warm_start=2)  # a call that fails its argument checks leaves zeros too
    out = _ffi.MipWarmStats(7, 7, 7, 7)
    lib.dzg_mip_last_warm_stats(C.byref(out))
    assert (out.nodes_warm, out.nodes_restarted, out.warm_iterations, out.restart_iterations) == (0, 0, 0, 0)
    lib.dzg_mip_last_warm_stats(None)  # NULL is ignored
    s = _ffi.mip_last_warm_stats()
    assert (s.nodes_warm, s.nodes_restarted, s.warm_iterations, s.restart_iterations) == (0, 0, 0, 0)


# ---------------------------------------------------------------- the reference search is right
def test_warm_reference_equals_the_cold_reference():
    optimal = panicked = with_warm = mixed_with_cold_children = 0
    for i, (md, flags) in enumerate(_models()):
        cold = mr.branch_and_bound(md, flags)
        warm = mw.branch_and_bound_warm(md, flags)
        assert warm["status"] == cold["status"], (i, warm["status"], cold["status"])
        assert len(warm["flags"]) == len(warm["log"]) == warm["nodes_solved"] or warm["failed_node"] >= 0
        assert warm["nodes_warm"] == sum(w for w, _ in warm["flags"])
        assert warm["nodes_restarted"] == sum(r for _, r in warm["flags"])
        assert all(w or not r for w, r in warm["flags"]) and warm["flags"][0] == (False, False)
        with_warm += warm["nodes_warm"] > 0
        cold_children = sum(1 for e, (w, _) in zip(warm["log"], warm["flags"]) if e[0] > 0 and not w)
        mixed_with_cold_children += i >= 16 and cold_children > 0
        if cold["status"] != "optimal":
            panicked += cold["status"] == mr.STATUS["panic"]
            continue
        optimal += 1
        diff = abs(warm["objective"] - cold["objective"])
        print(f"model {i}: warm {warm['objective']!r} cold {cold['objective']!r} diff {diff:.3e} "
              f"pivots {warm['lp_iterations']} / {cold['lp_iterations']}")
        assert diff <= 1e-9 * max(1.0, abs(cold["objective"])) + 1e-9, (i, warm["objective"], cold["objective"])
        if i < 16:
            want = mr.enumerate_optimum(md)
            assert abs(warm["objective"] - want) <= 1e-9 * max(1.0, abs(want)), (i, warm["objective"], want)
    assert (optimal, panicked) == (34, 6)
    assert with_warm >= 20 and mixed_with_cold_children >= 20, (with_warm, mixed_with_cold_children)


# ---------------------------------------------------------------- the reason for the feature
def _knapsack_pair(seed, attempts=None):
    md, flags = _mip_bench().knapsack(seed)
    cold = mr.branch_and_bound(md, flags, node_limit=5000)
    warm = mw.branch_and_bound_warm(md, flags, node_limit=5000, attempts=attempts)
    return cold, warm


def _check_pivot_saving(seed):
    cold, warm = _knapsack_pair(seed)
    print(f"knapsack {seed}: pivots cold {cold['lp_iterations']} warm {warm['lp_iterations']}, "
          f"warm nodes {warm['nodes_warm']}, restarted {warm['nodes_restarted']}")
    assert cold["status"] == warm["status"] == "optimal"
    assert abs(warm["objective"] - cold["objective"]) <= 1e-9 * max(1.0, abs(cold["objective"])) + 1e-9
    assert warm["lp_iterations"] * 8 <= cold["lp_iterations"]
    assert warm["nodes_warm"] > 0 and warm["nodes_restarted"] * 50 <= warm["nodes_warm"]
    assert warm["lp_iterations"] >= warm["warm_iterations"] + warm["restart_iterations"]


@pytest.mark.parametrize("seed", [1000, 1003])
def test_warm_search_needs_an_eighth_of_the_pivots(seed):
    _check_pivot_saving(seed)


def test_false_warm_optimum_is_restarted():
    # knapsack 1001: one warm attempt ends OPTIMAL with a carried z at -14.4 (status() looks only
    # at entries whose perturbation is positive); the sign check discards it
    attempts = []
    cold, warm = _knapsack_pair(1001, attempts)
    false_optima = [low for st, low in attempts if st == "optimal" and low < -1.0]
    print("knapsack 1001: false warm optima (min over x, z):", false_optima,
          "pivots cold", cold["lp_iterations"], "warm", warm["lp_iterations"])
    assert len(false_optima) >= 1 and warm["nodes_restarted"] >= len(false_optima)
    assert len(attempts) == warm["nodes_warm"]
    accepted = [low for st, low in attempts if st == "optimal" and low >= -mw.WARM_TOL]
    assert len(accepted) == warm["nodes_warm"] - warm["nodes_restarted"]
    assert cold["status"] == warm["status"] == "optimal"
    assert abs(warm["objective"] - cold["objective"]) <= 1e-9 * max(1.0, abs(cold["objective"])) + 1e-9
    assert warm["lp_iterations"] * 8 <= cold["lp_iterations"]
    assert warm["nodes_restarted"] * 50 <= warm["nodes_warm"]
