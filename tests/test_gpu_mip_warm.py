"""Warm-started branch and bound on the GPU (dzg_mip_opts.warm_start, k_mip.hip): the node log
equals the warm reference search of tests/mip_warm_reference.py node for node, bit for bit, the
warm counters included; a false warm optimum is restarted; invariance under the slicing knobs;
warm_start=0 is the cold search; structure changes give cold children; the Python surface."""
import importlib.util
import os

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi
from dantzig_amd import rust as rs
from tests import mip_reference as mr
from tests import mip_warm_reference as mw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_bb(md, flags, node_log=8192, **mo):
    res, values, log = rs._mip_call(mr.c_arrays(md), flags, node_log, **mo)
    log = [(i, p, bv, d, b, st, it, obj if st == 0 else None) for i, p, bv, d, b, st, it, obj in log]
    return res, values, log


def within_tol(a, b):
    return abs(a - b) <= 1e-9 * max(1.0, abs(b)) + 1e-9


def assert_same_warm_search(md, flags, what, **mo):
    ref = mw.branch_and_bound_warm(md, flags, **{k: v for k, v in mo.items() if k != "pivots_per_launch"})
    res, values, log = gpu_bb(md, flags, warm_start=1, **mo)
    assert len(log) == len(ref["log"]), (what, len(log), len(ref["log"]))
    for g, w in zip(log, ref["log"]):
        assert g == w, (what, g, w)  # ids, parents, branch decisions, status, summed iterations, objective
    want = {"optimal": 0, "infeasible": 2, "node_limit": _ffi.NODE_LIMIT}.get(ref["status"], ref["status"])
    assert res.status == want, what
    assert res.nodes_solved == ref["nodes_solved"] and res.rounds == ref["rounds"], what
    assert res.lp_iterations == ref["lp_iterations"], what
    if ref["objective"] is not None:
        assert res.has_incumbent and res.objective == ref["objective"], what
        assert res.incumbent_node == ref["incumbent_node"], what
        assert np.array_equal(values[:len(flags)], ref["values"]), what
    assert res.warm_stats == (ref["nodes_warm"], ref["nodes_restarted"], ref["warm_iterations"],
                              ref["restart_iterations"]), (what, res.warm_stats)
    return res, log, ref


def _models():
    rng = np.random.default_rng(2024)
    out = [mr.random_pure_milp(rng) for _ in range(16)]
    out += [mr.random_mixed_milp(rng) for _ in range(24)]
    return out


def _mip_bench():
    spec = importlib.util.spec_from_file_location("mip_bench", os.path.join(ROOT, "tools", "mip_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_warm_tree_parity_with_the_warm_reference():
    with_warm = restarted = 0
    for i, (md, flags) in enumerate(_models()):
        res, _, _ = assert_same_warm_search(md, flags, f"model {i}")
        with_warm += res.warm_stats[0] > 0
        restarted += res.warm_stats[1]
    assert with_warm >= 10 and restarted >= 1, (with_warm, restarted)


def test_warm_tree_parity_in_the_largest_row_bucket():
    # tests/test_gpu_mip.py's 40 binaries, 3 knapsack rows: 83 rows, 256 threads per node
    rng = np.random.default_rng(41)
    n = 40
    w = rng.integers(1, 15, (3, n)).astype(float)
    v = rng.integers(1, 100, n).astype(float)
    md = {"vars": [{"lb": 0.0, "ub": 1.0} for _ in range(n)],
          "objective": {"terms": [[u, float(v[u])] for u in range(n)], "constant": 0.0},
          "constraints": [{"terms": [[u, float(w[d, u])] for u in range(n)], "b": float(w[d].sum() // 2)}
                          for d in range(3)]}
    res, log, _ = assert_same_warm_search(md, [1] * n, "knapsack 40", node_limit=80)
    assert res.nodes_batched == res.nodes_solved == len(log) >= 10
    assert res.warm_stats[0] == res.nodes_solved - 1  # binaries: every child keeps the root's structure


def test_false_warm_optimum_is_restarted_on_the_gpu():
    md, flags = _mip_bench().knapsack(1001)
    res, _, ref = assert_same_warm_search(md, flags, "knapsack 1001", node_limit=5000)
    assert res.status == _ffi.OPTIMAL and res.warm_stats[1] >= 1
    cold, _, _ = gpu_bb(md, flags, node_limit=5000)
    assert cold.status == _ffi.OPTIMAL and cold.warm_stats == (0, 0, 0, 0)
    print("knapsack 1001: warm", res.objective, res.lp_iterations, "cold", cold.objective, cold.lp_iterations)
    assert within_tol(res.objective, cold.objective), (res.objective, cold.objective)
    assert res.lp_iterations * 8 <= cold.lp_iterations


def test_warm_slicing_and_round_size_invariance():
    compared = 0
    for md, flags in _models()[:32:2]:
        r0, v0, l0 = gpu_bb(md, flags, warm_start=1)
        for ppl in (1, 5, 0):
            r1, v1, l1 = gpu_bb(md, flags, warm_start=1, pivots_per_launch=ppl)
            assert l1 == l0 and np.array_equal(v1, v0) and r1.warm_stats == r0.warm_stats
        runs = [gpu_bb(md, flags, warm_start=1, nodes_per_round=npr)[0] for npr in (1, 7, 0)]
        if any(r.status not in (_ffi.OPTIMAL, _ffi.INFEASIBLE) for r in runs):
            continue  # a node LP hit a panic path: which nodes are solved depends on the round size
        assert len({int(r.status) for r in runs}) == 1
        if runs[0].status == _ffi.OPTIMAL:
            for r in runs:
                assert within_tol(r.objective, runs[0].objective), [x.objective for x in runs]
        compared += r0.warm_stats[0] > 0
    assert compared >= 3


def test_warm_start_zero_is_the_cold_search():
    for md, flags in _models()[:5]:
        r0, v0, l0 = gpu_bb(md, flags)
        r1, v1, l1 = gpu_bb(md, flags, warm_start=0)
        assert l1 == l0 and np.array_equal(v1, v0)
        assert (r1.status, r1.objective, r1.lp_iterations, r1.rounds) == (r0.status, r0.objective,
                                                                         r0.lp_iterations, r0.rounds)
        assert r1.warm_stats == (0, 0, 0, 0)
        ref = mr.branch_and_bound(md, flags)
        assert l1 == ref["log"]


def test_branches_that_add_bound_rows_give_cold_children():
    seen = 0
    for i, (md, flags) in enumerate(_models()[16:], start=16):
        unbounded_side = any(f and (v.get("lb") is None or v.get("ub") is None)
                             for v, f in zip(md["vars"], flags))
        if not unbounded_side:
            continue
        res, _, ref = assert_same_warm_search(md, flags, f"model {i}")
        cold_children = sum(1 for e, (w, _) in zip(ref["log"], ref["flags"]) if e[0] > 0 and not w)
        if cold_children:
            assert res.warm_stats[0] < res.nodes_solved - 1
            seen += 1
    assert seen >= 10, seen


def test_warm_start_on_the_surface():
    # 0/1 knapsack: weights 12 2 1 1 4, values 4 2 1 2 10, capacity 15 -> items 1..4, value 15
    w, v = [12, 2, 1, 1, 4], [4, 2, 1, 2, 10]
    xs = [dz.Variable.binary() for _ in w]
    prob = dz.Maximize(sum(vi * xi for vi, xi in zip(v, xs))).subject_to(
        sum(wi * xi for wi, xi in zip(w, xs)) <= 15)
    cold = prob.solve()
    assert cold.mip.nodes_warm == 0 and cold.mip.nodes_restarted == 0
    rs.set_mip_options(warm_start=True)
    try:
        sol = prob.solve()
        low = dz.Minimize(sum(-vi * xi for vi, xi in zip(v, xs))).subject_to(
            sum(wi * xi for wi, xi in zip(w, xs)) <= 15).solve()
    finally:
        rs.set_mip_options()
    assert sol.objective_value == 15.0 and [round(sol[xi]) for xi in xs] == [0, 1, 1, 1, 1]
    assert sol.mip.nodes_warm > 0 and sol.mip.nodes_restarted >= 0 and sol.mip.status == "optimal"
    assert low.objective_value == -15.0 and low.mip.nodes_warm > 0  # the flipped MipInfo keeps them
    obj, cons = prob._rust_problem()
    per_call = rs.solve_mip(obj, cons, warm_start=True)
    assert per_call.objective_value == 15.0 and per_call.mip.nodes_warm == sol.mip.nodes_warm
