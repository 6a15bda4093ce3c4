"""FAST node LPs without a GPU (dzg_mip_solve_nodes, DESIGN.md 7c "FAST node LPs"): the checker of
tests/mip_fast_check.py is tested on the reference searches (it passes on the cold and the warm one
and fails on a moved objective, a flipped status and a fractional incumbent), the new structs and
calls through the C ABI and the Python surface, and the float64 restatement of the acceptance
certificate over the warm reference search: it accepts every correct warm optimum and rejects the
false one of knapsack 1001 (1946.69 for a node whose optimum is 1948.80)."""
import ctypes as C
import importlib.util
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from dantzig_amd import _ffi
from dantzig_amd import rust as rs
from oracle import oracle as ora
from tests import mip_fast_check as fc
from tests import mip_reference as mr
from tests import mip_warm_reference as mw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mip_bench():
    spec = importlib.util.spec_from_file_location("mip_bench", os.path.join(ROOT, "tools", "mip_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _models():
    rng = np.random.default_rng(2024)
    out = [mr.random_pure_milp(rng) for _ in range(16)]
    out += [mr.random_mixed_milp(rng) for _ in range(24)]
    return out


def _as_result(ref):
    return SimpleNamespace(has_incumbent=ref["objective"] is not None, objective=ref["objective"])


# ---------------------------------------------------------------- the checker
@pytest.fixture(scope="module")
def searches():
    """(md, flags, cold reference, warm reference) of the first optimal models."""
    out = []
    for md, flags in _models()[:8]:
        cold = mr.branch_and_bound(md, flags)
        if cold["status"] == "optimal":
            out.append((md, flags, cold, mw.branch_and_bound_warm(md, flags)))
    assert len(out) >= 5
    return out


def test_checker_passes_on_the_reference_searches(searches):
    for md, flags, cold, warm in searches:
        fc.check_search(md, flags, _as_result(cold), cold["values"], cold["log"], [0] * len(cold["log"]),
                        cold_objective=cold["objective"])
        route = [1 if w and not r else 0 for w, r in warm["flags"]]
        fc.check_search(md, flags, _as_result(warm), warm["values"], warm["log"], route,
                        cold_objective=cold["objective"])


def _first(log, pred):
    return next(k for k, e in enumerate(log) if pred(e))


def test_checker_fails_on_a_moved_objective_a_flipped_status_and_a_fractional_incumbent(searches):
    md, flags, cold, _ = searches[0]
    res, values, log = _as_result(cold), cold["values"], cold["log"]
    k = _first(log, lambda e: e[5] == 0)
    for route in ([0] * len(log), [1] * len(log)):  # bit equality and the tolerance both catch 1e-6
        moved = list(log)
        moved[k] = moved[k][:7] + (moved[k][7] + 1e-6 * max(1.0, abs(moved[k][7])),)
        with pytest.raises(AssertionError, match=f"node {log[k][0]} "):
            fc.check_search(md, flags, res, values, moved, route)
    flipped = list(log)
    flipped[k] = flipped[k][:5] + (2,) + flipped[k][6:7] + (None,)
    with pytest.raises(AssertionError, match="status 2"):
        fc.check_search(md, flags, res, values, flipped, [0] * len(log))
    ints = [u for u, f in enumerate(flags) if f]
    frac = np.array(values, dtype=float)
    frac[ints[0]] += 0.25
    with pytest.raises(AssertionError, match="not integral"):
        fc.check_search(md, flags, res, frac, log, [0] * len(log))
    last_bit = list(log)  # one ulp: inside the tolerance, outside bit equality
    last_bit[k] = last_bit[k][:7] + (float(np.nextafter(last_bit[k][7], np.inf)),)
    fc.check_search(md, flags, res, values, last_bit, [1] * len(log))
    with pytest.raises(AssertionError, match="bit for bit"):
        fc.check_search(md, flags, res, values, last_bit, [2] * len(log))


def test_cold_children_are_the_branches_that_add_a_bound_row():
    seen = 0
    for md, flags in _models()[16:24]:
        warm = mw.branch_and_bound_warm(md, flags)
        want = [e[0] for e, (w, _) in zip(warm["log"], warm["flags"]) if e[0] > 0 and not w]
        assert fc.cold_children(md, flags, warm["log"]) == want
        seen += bool(want)
    assert seen >= 3


# ---------------------------------------------------------------- plumbing
def test_struct_layouts(tmp_path):
    assert C.sizeof(_ffi.MipOpts) == 48 and C.sizeof(_ffi.MipNode) == 56 and C.sizeof(_ffi.MipResult) == 136
    assert C.sizeof(_ffi.MipNodeOpts) == 40 and C.sizeof(_ffi.MipFastStats) == 32
    structs = {"dzg_mip_node_opts": _ffi.MipNodeOpts, "dzg_mip_fast_stats": _ffi.MipFastStats,
               "dzg_mip_debug_node": _ffi.MipDebugNode, "dzg_mip_opts": _ffi.MipOpts,
               "dzg_mip_node": _ffi.MipNode, "dzg_mip_result": _ffi.MipResult}
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
    with open(os.path.join(ROOT, "include", "dantzig_amd.h")) as f:
        assert "#define DZG_ABI_VERSION 4" in f.read()


def test_exports_and_defaults():
    lib = _ffi.lib()
    for name in ("dzg_mip_solve_nodes", "dzg_mip_last_fast_stats", "dzg_mip_node_opts_default",
                 "dzg_debug_mip_fast_node"):
        assert name in _ffi.EXPORTS and hasattr(lib, name), name
    o = _ffi.default_mip_node_opts()
    assert (o.numerics, o.reserved, o.pivots_per_launch, o.refactor_every, o.route, o.route_cap) == (
        _ffi.STRICT, 0, 0, 0, None, 0)
    assert _ffi.default_mip_node_opts(numerics="fast").numerics == _ffi.FAST
    assert _ffi.default_mip_node_opts(numerics="strict", refactor_every=3).refactor_every == 3
    with pytest.raises(ValueError):
        _ffi.default_mip_node_opts(numerics="auto")
    for name in ("reserved", "bogus"):
        with pytest.raises(TypeError):
            _ffi.default_mip_node_opts(**{name: 1})
    lib.dzg_mip_node_opts_default(None)  # NULL is ignored


def _nodes_rc(node=None, opts=None, **kw):
    arrays = mr.c_arrays({"vars": [{"lb": 0.0, "ub": 3.0}], "objective": {"terms": [[0, 1.0]]},
                          "constraints": [{"terms": [[0, 2.0]], "b": 3.0}]})
    model = rs._c_model(arrays)
    flags = np.array([1, 0], dtype=np.int32)
    r = _ffi.MipResult()
    o = _ffi.default_opts(**(opts or {}))
    m = _ffi.default_mip_opts()
    no = _ffi.MipNodeOpts() if node is None else node
    for k, v in kw.items():
        setattr(no, k, v)
    rc = _ffi.lib().dzg_mip_solve_nodes(C.byref(model), _ffi.ptr(flags), C.byref(o), C.byref(m), C.byref(no),
                                        C.byref(r))
    return rc, _ffi.lib().dzg_last_error().decode()


@pytest.mark.parametrize("kw, word", [({"numerics": 2}, "numerics"), ({"numerics": -1}, "numerics"),
                                       ({"numerics": 7}, "numerics"),
                                       ({"pivots_per_launch": -1}, "pivots_per_launch"),
                                       ({"refactor_every": -1}, "refactor_every"),
                                       ({"route_cap": -1}, "route_cap"), ({"route_cap": 4}, "route")])
def test_node_option_argument_errors(kw, word):
    rc, msg = _nodes_rc(**kw)
    assert rc == _ffi.E_ARG, (rc, msg)
    assert msg.startswith("mip:") and word in msg, msg


def test_opts_numerics_fast_stays_an_argument_error():
    rc, msg = _nodes_rc(numerics=_ffi.FAST, opts={"numerics": _ffi.FAST})
    assert rc == _ffi.E_ARG and msg.startswith("mip:") and "FAST" in msg, (rc, msg)


def test_last_fast_stats_zero_fills_and_ignores_null():
    lib = _ffi.lib()
    _nodes_rc(numerics=9)  # a call that fails its argument checks leaves zeros
    out = _ffi.MipFastStats(7, 7, 7, 7)
    lib.dzg_mip_last_fast_stats(C.byref(out))
    assert (out.nodes_fast, out.nodes_rejected, out.fast_iterations, out.strict_iterations) == (0, 0, 0, 0)
    lib.dzg_mip_last_fast_stats(None)
    s = _ffi.mip_last_fast_stats()
    assert (s.nodes_fast, s.nodes_rejected, s.fast_iterations, s.strict_iterations) == (0, 0, 0, 0)


def test_set_mip_options_splits_the_node_options():
    rs.set_mip_options(warm_start=True, node_numerics="fast", fast_pivots_per_launch=5, refactor_every=2)
    try:
        assert rs._mip_options == {"warm_start": True, "node_numerics": "fast", "fast_pivots_per_launch": 5,
                                   "refactor_every": 2}
        search, node = rs._split_mip_options(rs._mip_options)
        assert search == {"warm_start": True}
        no = rs._node_opts(node)
        assert (no.numerics, no.pivots_per_launch, no.refactor_every) == (_ffi.FAST, 5, 2)
        for bad in ({"bogus": 1}, {"numerics": "fast"}, {"reserved": 1}):
            with pytest.raises(TypeError):
                rs.set_mip_options(**bad)
        with pytest.raises(ValueError):
            rs.set_mip_options(node_numerics="auto")
        assert rs._mip_options["node_numerics"] == "fast"  # a refused call changes nothing
    finally:
        rs.set_mip_options()
    assert rs._mip_options == {} and rs._node_opts({}) is None
    assert rs._node_opts({"node_numerics": "strict"}).numerics == _ffi.STRICT


def test_mip_info_slots():
    info = rs.MipInfo(status="optimal")
    assert info.nodes_fast_accepted is None and info.nodes_fast_rejected is None
    assert {"nodes_fast_accepted", "nodes_fast_rejected", "nodes_warm"} <= set(rs.MipInfo.__slots__)
    info = rs.MipInfo(nodes_fast_accepted=3, nodes_fast_rejected=1)
    assert (info.nodes_fast_accepted, info.nodes_fast_rejected) == (3, 1)


# ---------------------------------------------------------------- the certificate, restated in float64
def _optimal_warm_attempts(monkeypatch, md, flags, **kw):
    """Every warm attempt of the warm reference search that ended optimal: (the node's bounds, the
    attempt's result, the node's final objective -- the cold run's when the attempt was discarded)."""
    calls, out = [], []
    real_solve, real_node = ora.simplex_solve, mw.solve_warm_node

    def spy(sf, *a, **k):
        res = real_solve(sf, *a, **k)
        if "xbar" in k:  # only the warm attempts pass perturbation vectors
            calls.append(res)
        return res

    def node(model, ints, bnd, parent_state, attempts=None):
        n0 = len(calls)
        r = real_node(model, ints, bnd, parent_state, attempts)
        out.extend((list(bnd), res, r[2] if r[0] == 0 else None) for res in calls[n0:] if res.status == "optimal")
        return r

    monkeypatch.setattr(ora, "simplex_solve", spy)
    monkeypatch.setattr(mw, "solve_warm_node", node)
    mw.branch_and_bound_warm(md, flags, **kw)
    monkeypatch.undo()
    return out


def test_certificate_accepts_every_correct_warm_optimum_of_the_random_models(monkeypatch):
    accepted = rejected = 0
    for i, (md, flags) in enumerate(_models()):
        ints = [u for u, f in enumerate(flags) if f]
        for bnd, res, _ in _optimal_warm_attempts(monkeypatch, md, flags):
            node_md = mr.node_model(md, ints, bnd)
            st, _, cold_obj, _ = mr.solve_node(node_md)
            correct = st == 0 and fc.within_tol(float(res.objective), cold_obj)
            ok, x, z = fc.certificate(ora.build_standard_form(node_md), res.basis, res.nonbasis)
            if correct:
                assert ok, (i, bnd, float(np.min(x)), float(np.min(z)))
                accepted += 1
            else:
                assert not ok, (i, bnd, float(res.objective), cold_obj)
                rejected += 1
    print(f"certificate over the 40 random models: {accepted} correct warm optima accepted, "
          f"{rejected} false ones rejected")
    assert accepted >= 20  # the check is not vacuous: at least 20 of the models have warm nodes


def test_certificate_rejects_the_false_warm_optimum_of_knapsack_1001(monkeypatch):
    md, flags = _mip_bench().knapsack(1001)
    ints = [u for u, f in enumerate(flags) if f]
    attempts = _optimal_warm_attempts(monkeypatch, md, flags, node_limit=5000)
    false_optima = 0
    for k, (bnd, res, final_obj) in enumerate(attempts):
        low = min(float(np.min(res.x, initial=np.inf)), float(np.min(res.z, initial=np.inf)))
        if low >= -1.0 and k % 25:
            continue  # the false optima all, one in 25 of the others
        ok, _, _ = fc.certificate(ora.build_standard_form(mr.node_model(md, ints, bnd)), res.basis, res.nonbasis)
        if low < -1.0:
            # the warm "optimum" is not the node LP's: the cold run that replaced it found more
            print(f"knapsack 1001: false warm optimum {float(res.objective)!r}, the node LP's {final_obj!r}")
            assert final_obj is not None and float(res.objective) < final_obj - 1.0
            assert not ok
            false_optima += 1
        else:
            assert ok == (low >= -mw.WARM_TOL), (k, low)
    assert false_optima >= 1


