"""Branch and bound on the GPU (dzg_mip_solve, k_mip.hip): the node log equals the reference
search of tests/mip_reference.py node for node, bit for bit; node LPs equal .solve() of the node
model; known answers; invariance under the slicing knobs; the sequential route; the node limit."""
import math
import warnings

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi
from dantzig_amd import rust as rs
from tests import mip_reference as mr

pytestmark = pytest.mark.gpu


def gpu_bb(md, flags, node_log=4096, **mo):
    res, values, log = rs._mip_call(mr.c_arrays(md), flags, node_log, **mo)
    log = [(i, p, bv, d, b, st, it, obj if st == 0 else None) for i, p, bv, d, b, st, it, obj in log]
    return res, values, log


def assert_same_search(md, flags, what, **mo):
    ref = mr.branch_and_bound(md, flags, **{k: v for k, v in mo.items() if k != "pivots_per_launch"})
    res, values, log = gpu_bb(md, flags, **mo)
    assert len(log) == len(ref["log"]), what
    for g, w in zip(log, ref["log"]):
        assert g == w, (what, g, w)  # ids, parents, branch decisions, status, iterations, objective
    want = {"optimal": 0, "infeasible": 2, "node_limit": _ffi.NODE_LIMIT}.get(ref["status"], ref["status"])
    assert res.status == want, what
    assert res.nodes_solved == ref["nodes_solved"] and res.rounds == ref["rounds"], what
    assert res.lp_iterations == ref["lp_iterations"], what
    if ref["objective"] is not None:
        assert res.has_incumbent and res.objective == ref["objective"], what
        assert res.incumbent_node == ref["incumbent_node"], what
        assert np.array_equal(values[:len(flags)], ref["values"]), what
    return res, log


def _models():
    rng = np.random.default_rng(2024)
    out = [mr.random_pure_milp(rng) for _ in range(16)]
    out += [mr.random_mixed_milp(rng) for _ in range(24)]
    return out


def test_tree_parity_with_the_reference_search():
    statuses = set()
    grew = 0
    for i, (md, flags) in enumerate(_models()):
        res, log = assert_same_search(md, flags, f"model {i}")
        statuses.add(int(res.status))
        grew += res.nodes_solved > 1
    assert 0 in statuses and grew >= 10, (statuses, grew)  # infeasible: test_known_answers


def test_tree_parity_in_the_largest_row_bucket():
    # 40 binaries, 3 knapsack rows: 83 rows, the 65-128-row bucket (256 threads, m > BLOCK / 2)
    rng = np.random.default_rng(41)
    n = 40
    w = rng.integers(1, 15, (3, n)).astype(float)
    v = rng.integers(1, 100, n).astype(float)
    md = {"vars": [{"lb": 0.0, "ub": 1.0} for _ in range(n)],
          "objective": {"terms": [[u, float(v[u])] for u in range(n)], "constant": 0.0},
          "constraints": [{"terms": [[u, float(w[d, u])] for u in range(n)], "b": float(w[d].sum() // 2)}
                          for d in range(3)]}
    res, log = assert_same_search(md, [1] * n, "knapsack 40", node_limit=80)
    assert res.status == _ffi.OPTIMAL and res.nodes_batched == res.nodes_solved == len(log) >= 10


def _node_bounds(md, flags, log, node):
    """The integer bounds of a logged node: the root's, then every branch on its parent chain."""
    by_id = {e[0]: e for e in log}
    chain = []
    while node > 0:
        chain.append(by_id[node])
        node = by_id[node][1]
    vs = [dict(v) for v in md["vars"]]
    for _, _, var, d, bound, *_ in reversed(chain):
        vs[var]["lb" if d > 0 else "ub"] = bound
    return dict(md, vars=vs)


def test_node_lps_equal_solve_of_the_node_model():
    checked = 0
    for md, flags in _models()[16:30]:
        _, _, log = gpu_bb(md, flags)
        for e in log[::3]:
            nm = _node_bounds(md, flags, log, e[0])
            vs = [rs.Variable(lb=v["lb"], ub=v["ub"]) for v in nm["vars"]]
            obj = rs.PyAffExpr(linexpr=rs.PyLinExpr([t[1] for t in nm["objective"]["terms"]],
                                                    [vs[t[0]] for t in nm["objective"]["terms"]]),
                               constant=nm["objective"]["constant"])
            cons = [rs.PyInequality(linexpr=rs.PyLinExpr([t[1] for t in c["terms"]],
                                                         [vs[t[0]] for t in c["terms"]]), b=c["b"])
                    for c in nm["constraints"]]
            try:
                sol = rs.solve(obj, cons)
            except dz.exceptions.InfeasibleError:
                assert e[5] == _ffi.INFEASIBLE
                continue
            except RuntimeError as err:  # a reference panic path: the same status in the log
                assert e[5] == _ffi.PANIC and "panic" in str(err)
                continue
            assert e[5] == _ffi.OPTIMAL
            assert (sol.iterations, sol.objective_value) == (e[6], e[7])
            checked += 1
    assert checked >= 20


def test_known_answers():
    x, y = dz.Variable.integer(), dz.Variable.integer()
    sol = dz.Maximize(x + y).subject_to(2 * x + 2 * y <= 3).solve()
    assert sol.objective_value == 1.0 and sol.mip is not None and sol.mip.status == "optimal"
    assert sol.mip.nodes > 1
    # 0/1 knapsack: weights 12 2 1 1 4, values 4 2 1 2 10, capacity 15 -> items 1..4, value 15
    w, v = [12, 2, 1, 1, 4], [4, 2, 1, 2, 10]
    xs = [dz.Variable.binary() for _ in w]
    sol = dz.Maximize(sum(vi * xi for vi, xi in zip(v, xs))).subject_to(
        sum(wi * xi for wi, xi in zip(w, xs)) <= 15).solve()
    assert sol.objective_value == 15.0
    assert [round(sol[xi]) for xi in xs] == [0, 1, 1, 1, 1]
    # 5 x 5 assignment, minimised
    cost = [[9, 2, 7, 8, 6], [6, 4, 3, 7, 5], [5, 8, 1, 8, 7], [7, 6, 9, 4, 8], [3, 7, 5, 9, 2]]
    a = [[dz.Variable.binary() for _ in range(5)] for _ in range(5)]
    prob = dz.Minimize(sum(cost[i][j] * a[i][j] for i in range(5) for j in range(5)))
    for i in range(5):
        prob = prob.subject_to(sum(a[i][j] for j in range(5)) == 1)
        prob = prob.subject_to(sum(a[j][i] for j in range(5)) == 1)
    sol = prob.solve()
    best = min(sum(cost[i][p[i]] for i in range(5)) for p in __import__("itertools").permutations(range(5)))
    assert sol.objective_value == best
    assert sol.mip.best_bound == best  # the user's sense
    # 2x == 1: the relaxation is feasible, no integer point is
    z = dz.Variable.integer(lb=None, ub=None)
    with pytest.raises(dz.exceptions.InfeasibleError):
        dz.Maximize(z).subject_to(2 * z == 1).solve()
    u = dz.Variable.integer()
    with pytest.raises(dz.exceptions.UnboundedError):
        dz.Maximize(u).subject_to(-1 * u <= 0).solve()


def test_slicing_and_round_size_invariance():
    compared = 0
    for md, flags in _models()[20:28]:
        _, v0, l0 = gpu_bb(md, flags)
        for ppl in (1, 256):
            _, v1, l1 = gpu_bb(md, flags, pivots_per_launch=ppl)
            assert l1 == l0 and np.array_equal(v1, v0)
        runs = [gpu_bb(md, flags, nodes_per_round=npr)[0] for npr in (1, 7, 0)]
        if any(r.status not in (_ffi.OPTIMAL, _ffi.INFEASIBLE) for r in runs):
            continue  # a node LP hit a panic path: which nodes are solved depends on the round size
        assert len({int(r.status) for r in runs}) == 1
        if runs[0].status == _ffi.OPTIMAL:  # alternative optima may differ in the last bits
            objs = [r.objective for r in runs]
            assert max(objs) - min(objs) <= 1e-9 * max(1.0, abs(objs[0])), objs
        compared += 1
    assert compared >= 3


def _big_knapsack(n, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(5, 40, n).astype(float)
    v = (w + rng.integers(-3, 4, n)).astype(float)
    return ({"vars": [{"lb": 0.0, "ub": 1.0} for _ in range(n)],
             "objective": {"terms": [[u, float(v[u])] for u in range(n)], "constant": 0.0},
             "constraints": [{"terms": [[u, float(w[u])] for u in range(n)], "b": float(w.sum() // 2) + 0.5}]},
            [1] * n)


def test_sequential_route_over_128_rows():
    md, flags = _big_knapsack(80, 5)  # 161 rows: still STRICT under AUTO, too big for a batch
    res, log = assert_same_search(md, flags, "knapsack 80", node_limit=12)
    assert res.nodes_sequential == res.nodes_solved == len(log) and res.nodes_batched == 0


def test_node_limit():
    md, flags = _big_knapsack(10, 3)  # 11 nodes at one per round, the first incumbent at the 10th
    full, _, _ = gpu_bb(md, flags, nodes_per_round=1)
    assert full.status == _ffi.OPTIMAL and full.nodes_solved > 3
    limit = next(k for k in range(1, full.nodes_solved)
                 if gpu_bb(md, flags, nodes_per_round=1, node_limit=k)[0].has_incumbent)
    res, _, _ = gpu_bb(md, flags, nodes_per_round=1, node_limit=limit)
    assert res.status == _ffi.NODE_LIMIT and res.has_incumbent and res.nodes_solved == limit
    assert res.best_bound >= res.objective
    assert_same_search(md, flags, "limited", nodes_per_round=1, node_limit=limit)
    xs = [dz.Variable.binary() for _ in flags]
    terms = md["objective"]["terms"]
    prob = dz.Maximize(sum(c * xs[u] for u, c in terms)).subject_to(
        sum(c * xs[u] for u, c in md["constraints"][0]["terms"]) <= md["constraints"][0]["b"])
    rs.set_mip_options(nodes_per_round=1, node_limit=limit)
    try:
        with pytest.warns(dz.exceptions.MipLimitWarning):
            sol = prob.solve()
        assert sol.objective_value == res.objective and sol.mip.status == "node_limit"
        rs.set_mip_options(nodes_per_round=1, node_limit=1)
        with pytest.raises(RuntimeError, match="node limit"):
            prob.solve()
    finally:
        rs.set_mip_options()


def test_solve_many_accepts_integer_models():
    x, y = dz.Variable.integer(), dz.Variable.integer()
    p1 = dz.Maximize(x + y).subject_to(2 * x + 2 * y <= 3)
    a, b = dz.Variable.nonneg(), dz.Variable.nonneg()
    p2 = dz.Maximize(a + b).subject_to(2 * a + 2 * b <= 3)
    got = dz.solve_many([p1, p2])
    assert got[0].objective_value == 1.0 and got[0].mip is not None
    assert got[1].objective_value == 1.5 and got[1].mip is None
