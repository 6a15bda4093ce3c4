"""Branch-and-bound node LPs in FAST numerics on the GPU (dzg_mip_solve_nodes with numerics = FAST,
k_mip_node_fast in csrc/k_mip.hip, DESIGN.md 7c "FAST node LPs").

Every search is checked node by node against the CPU oracle by tests/mip_fast_check.check_search: the
same status for every logged node, the objective within 1e-9 max(1, |ref|) + 1e-9 and bit-equal where
the node went through the STRICT kernel, and the incumbent against the model itself.  The fallback is
the cold search bit for bit; the certificate's x and z lie within C_FAST_RESTART of the long-double
state of the final basis; a singular start basis is rejected; the same call twice is the same bits;
NULL and STRICT node options are dzg_mip_solve; the Python surface."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi
from dantzig_amd import rust as rs
from oracle import oracle as ora
from tests import batch_fast_from_reference as ffr
from tests import mip_fast_check as fc
from tests import mip_reference as mr
from tests import reopt_check as rc
from tests import state_check as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANIC_MODELS = (10, 18, 20, 29, 31, 32)  # the cold reference ends on a node LP with status 5


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


def K(n, d, seed):
    """tests/test_gpu_mip_warm.py's knapsack: n binaries, d rows."""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 15, (d, n)).astype(float)
    v = rng.integers(1, 100, n).astype(float)
    md = {"vars": [{"lb": 0.0, "ub": 1.0} for _ in range(n)],
          "objective": {"terms": [[u, float(v[u])] for u in range(n)], "constant": 0.0},
          "constraints": [{"terms": [[u, float(w[r, u])] for u in range(n)], "b": float(w[r].sum() // 2)}
                          for r in range(d)]}
    return md, [1] * n


def nodes_bb(md, flags, node=None, opts=None, node_log=8192, call="nodes", **mo):
    """dzg_mip_solve_nodes (call="solve": dzg_mip_solve; node=None with "nodes": NULL node options):
    (result with .warm_stats / .fast_stats, values, log as rust._mip_call's, route)."""
    arrays = mr.c_arrays(md)
    is_int = np.array(list(flags) + [0], dtype=np.int32)
    values = np.zeros(max(arrays["nvars"], 1))
    res = _ffi.MipResult()
    res.values = _ffi.ptr(values)
    log = (_ffi.MipNode * node_log)()
    res.log = C.cast(log, C.c_void_p)
    res.log_cap = node_log
    route = np.full(node_log, -1, dtype=np.int32)
    o = _ffi.default_opts(**(opts or {}))
    m = _ffi.default_mip_opts(**mo)
    model = rs._c_model(arrays)
    if call == "solve":
        got = _ffi.lib().dzg_mip_solve(C.byref(model), _ffi.ptr(is_int), C.byref(o), C.byref(m), C.byref(res))
    else:
        no = None
        if node is not None:
            no = _ffi.default_mip_node_opts(**node)
            no.route = _ffi.ptr(route)
            no.route_cap = node_log
        got = _ffi.lib().dzg_mip_solve_nodes(C.byref(model), _ffi.ptr(is_int), C.byref(o), C.byref(m),
                                             C.byref(no) if no is not None else None, C.byref(res))
    _ffi.check(got, "dzg_mip_solve_nodes")
    ws, fs = _ffi.mip_last_warm_stats(), _ffi.mip_last_fast_stats()
    res.warm_stats = (int(ws.nodes_warm), int(ws.nodes_restarted), int(ws.warm_iterations),
                      int(ws.restart_iterations))
    res.fast_stats = (int(fs.nodes_fast), int(fs.nodes_rejected), int(fs.fast_iterations),
                      int(fs.strict_iterations))
    entries = [(e.id, e.parent, e.branch_var, e.direction, e.bound, e.status, e.iterations,
                e.objective if e.status == 0 else None) for e in log[:res.log_count]]
    return res, values, entries, route[:res.log_count].tolist()


FAST = {"numerics": "fast"}


def fast_checked(md, flags, what, cold_objective=None, **mo):
    res, values, log, route = nodes_bb(md, flags, FAST, **mo)
    nf, nr = res.fast_stats[:2]
    print(f"{what}: {len(log)} nodes, FAST accepted {nf - nr}, rejected {nr}, pivots FAST {res.fast_stats[2]} "
          f"STRICT {res.fast_stats[3]}, status {res.status}")
    assert all(r in (fc.ROUTE_FAST, fc.ROUTE_REJECTED) for r in route), route  # every node here is batched
    assert (nf, nr) == (len(route), route.count(fc.ROUTE_REJECTED)) or res.failed_node >= 0
    fc.check_search(md, flags, res, values, log, route, cold_objective=cold_objective)
    return res, values, log, route


# ------------------------------------------------------------------ 1. bucket edges
@pytest.mark.parametrize("n, d, rows", [(6, 4, 16), (14, 4, 32), (15, 3, 33), (30, 4, 64), (31, 3, 65),
                                        (62, 4, 128)])
@pytest.mark.parametrize("warm", [0, 1])
def test_bucket_edges(n, d, rows, warm):
    md, flags = K(n, d, 41)
    assert ora.build_standard_form(md).m == rows
    res, _, log, route = fast_checked(md, flags, f"K({n},{d},41) warm_start={warm}", node_limit=24,
                                      warm_start=warm)
    assert res.nodes_batched == res.nodes_solved == len(log)
    assert route.count(fc.ROUTE_FAST) >= 1  # not through the fallback alone
    if not warm:
        assert res.warm_stats == (0, 0, 0, 0)


# ------------------------------------------------------------------ 2. whole searches
@pytest.fixture(scope="module")
def cold_1001():
    md, flags = _mip_bench().knapsack(1001)
    return nodes_bb(md, flags, call="solve", node_limit=5000)[0]


def test_whole_search_35_rows():
    md, flags = K(16, 3, 41)
    cold = nodes_bb(md, flags, call="solve")[0]
    res, _, _, _ = fast_checked(md, flags, "K(16,3,41)", cold_objective=cold.objective, warm_start=1)
    assert res.status == cold.status == _ffi.OPTIMAL


def test_whole_search_81_rows():
    md, flags = _mip_bench().knapsack(1003)
    cold = nodes_bb(md, flags, call="solve", node_limit=5000)[0]
    res, _, _, _ = fast_checked(md, flags, "knapsack 1003", cold_objective=cold.objective, warm_start=1,
                                node_limit=5000)
    assert res.status == cold.status == _ffi.OPTIMAL
    print("knapsack 1003: FAST warm pivots", res.lp_iterations, "cold", cold.lp_iterations)
    assert res.lp_iterations * 8 <= cold.lp_iterations


def test_whole_search_119_rows(cold_1001):
    # knapsack 1001: the model whose warm STRICT search meets a false optimum through the carried z.
    # The FAST restart does not take that z, so no attempt is rejected here; the sign check has
    # tests of its own below.
    md, flags = _mip_bench().knapsack(1001)
    res, _, _, _ = fast_checked(md, flags, "knapsack 1001", cold_objective=cold_1001.objective, warm_start=1,
                                node_limit=5000)
    assert res.status == cold_1001.status == _ffi.OPTIMAL
    print("knapsack 1001: FAST warm pivots", res.lp_iterations, "cold", cold_1001.lp_iterations)
    assert res.lp_iterations * 8 <= cold_1001.lp_iterations


# ------------------------------------------------------------------ 3. the 40 random models
def test_random_models_fast_and_warm():
    with_cold_child = 0
    for i, (md, flags) in enumerate(_models()):
        if i in PANIC_MODELS:  # FAST may get past the panicking node LP or stop on it
            res = nodes_bb(md, flags, FAST, warm_start=1)[0]
            assert res.status >= 0
            continue
        cold = mr.branch_and_bound(md, flags)
        res, _, log, route = fast_checked(md, flags, f"model {i}", cold_objective=cold["objective"],
                                          warm_start=1)
        want = {"optimal": 0, "infeasible": 2}[cold["status"]]
        assert res.status == want, (i, res.status, cold["status"])
        with_cold_child += i >= 16 and bool(fc.cold_children(md, flags, log))
    assert with_cold_child >= 10, with_cold_child


# ------------------------------------------------------------------ 4. the fallback is the cold search
def test_the_fallback_is_the_cold_search():
    stop_everything = {"near_tie_action": _ffi.NEAR_TIE_STOP, "tie_tol": 1e300}
    for what, (md, flags) in [(f"model {i}", mf) for i, mf in enumerate(_models()[:5])] + [("K(6,4,41)", K(6, 4, 41))]:
        ref = mr.branch_and_bound(md, flags)
        res, values, log, route = nodes_bb(md, flags, FAST, opts=stop_everything, warm_start=0)
        assert len(log) == len(ref["log"]), what
        for g, w in zip(log, ref["log"]):
            assert g[:6] == w[:6] and g[7] == w[7] and g[6] >= w[6], (what, g, w)
        if ref["values"] is not None:
            assert np.array_equal(values[:len(flags)], ref["values"]), what
        assert res.objective == (ref["objective"] or 0.0), what
        assert route == [fc.ROUTE_REJECTED] * len(log), (what, route)
        assert res.fast_stats[0] == res.fast_stats[1] == len(log), (what, res.fast_stats)


# ------------------------------------------------------------------ 5. the certificate
def debug_node(md, flags, bnd, start_basis=None, opts=None, **node):
    arrays = mr.c_arrays(md)
    is_int = np.array(list(flags) + [0], dtype=np.int32)
    model = rs._c_model(arrays)
    cap = 512
    basis, nonbasis = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    x, z = np.zeros(cap), np.zeros(cap)
    m, q = C.c_int64(0), C.c_int64(0)
    out = _ffi.MipDebugNode()
    o = _ffi.default_opts(**(opts or {}))
    no = _ffi.default_mip_node_opts(numerics="fast", **node)
    sb = None if start_basis is None else np.ascontiguousarray(start_basis, dtype=np.int32)
    bounds = np.ascontiguousarray(bnd, dtype=np.float64)  # held here: ptr() keeps no reference
    got = _ffi.lib().dzg_debug_mip_fast_node(C.byref(model), _ffi.ptr(is_int), _ffi.ptr(bounds),
                                             _ffi.ptr(sb), C.byref(o), C.byref(no), cap, cap, _ffi.ptr(basis),
                                             _ffi.ptr(nonbasis), _ffi.ptr(x), _ffi.ptr(z), C.byref(m), C.byref(q),
                                             C.byref(out))
    _ffi.check(got, "dzg_debug_mip_fast_node")
    return out, basis[:m.value].copy(), nonbasis[:q.value].copy(), x[:m.value].copy(), z[:q.value].copy()


def _exact(sf, basis, nonbasis):
    dense = ora.csc_to_dense(sf.m, sf.n, sf.col_ptr, sf.row_idx, sf.val)
    start = dict(basis=sf.basis, nonbasis=sf.nonbasis, x=sf.x, xbar=None, z=sf.z, zbar=None)
    return sc.exact_state(dense, sf.n, start, basis, nonbasis)


@pytest.mark.parametrize("n, d", [(30, 4), (62, 4)])
def test_certificate_state_against_long_double(n, d):
    md, flags = K(n, d, 41)
    _, root = fc.root_bounds(md, flags)
    sf = ora.build_standard_form(md)
    out, basis, nonbasis, x, z = debug_node(md, flags, root)
    assert (out.status, out.route) == (_ffi.OPTIMAL, fc.ROUTE_FAST), (out.status, out.route)
    ex = _exact(sf, basis, nonbasis)
    drift = rc.restart_drift(ex, dict(x=x, z=z, xbar=np.ones(len(x)), zbar=np.ones(len(z))))
    print(f"K({n},{d},41) root, cold: {out.iterations} pivots, certificate D = {drift['D']:.3e}")
    assert max(ex.err["x"], ex.err["z"]) * 1e2 <= ffr.C_FAST_RESTART, ex.err
    assert drift["D"] <= ffr.C_FAST_RESTART, drift
    assert float(x.min()) >= -1e-9 and float(z.min()) >= -1e-9
    # a child, warm from the root's final basis: branch on the first fractional variable's column
    res, _, log, route = nodes_bb(md, flags, FAST, node_limit=3, warm_start=1)
    child = log[1]
    bnd = list(root)
    bnd[2 * child[2] + (1 if child[3] < 0 else 0)] = child[4]
    node_md = mr.node_model(md, list(range(n)), bnd)
    want_st, _, want_obj, _ = mr.solve_node(node_md)
    out2, b2, n2, x2, z2 = debug_node(md, flags, bnd, start_basis=basis)
    assert out2.status == want_st
    if out2.status == _ffi.OPTIMAL:
        assert fc.within_tol(out2.objective, want_obj)
    if out2.route == fc.ROUTE_FAST:
        d2 = rc.restart_drift(_exact(ora.build_standard_form(node_md), b2, n2),
                              dict(x=x2, z=z2, xbar=np.ones(len(x2)), zbar=np.ones(len(z2))))
        print(f"K({n},{d},41) child, warm: {out2.iterations} pivots, certificate D = {d2['D']:.3e}")
        assert d2["D"] <= ffr.C_FAST_RESTART, d2
        assert out2.iterations < out.iterations
    else:
        assert out2.objective == want_obj


def test_a_start_basis_with_two_equal_columns_is_rejected():
    md, flags = K(30, 4, 41)
    _, root = fc.root_bounds(md, flags)
    _, basis, _, _, _ = debug_node(md, flags, root)
    twice = basis.copy()
    twice[1] = twice[0]
    out, _, _, _, _ = debug_node(md, flags, root, start_basis=twice)
    want_st, want_it, want_obj, _ = mr.solve_node(md)
    assert out.route == fc.ROUTE_REJECTED and out.fast_iterations == 0
    assert (out.status, out.iterations, out.objective) == (want_st, want_it, want_obj)  # the STRICT result stands


# The sign check itself.  status() ends OPTIMAL as soon as both perturbation ratios are <= opts.epsilon
# (fast_decide.h: `primal <= eps && dual <= eps`), so with epsilon = 1e6 the FAST loop ends OPTIMAL at
# its start state, without a pivot and without a singular inverse, whatever the signs of x and z: only
# the certificate's sign check stands between such a state and an accepted node.
STOP_AT_ONCE = {"epsilon": 1e6}


def test_sign_check_rejects_a_negative_recomputed_z():
    # cold: the slack basis has x = rhs >= 0 and z = -c < 0 (every value of K is >= 1)
    md, flags = K(30, 4, 41)
    _, root = fc.root_bounds(md, flags)
    sf = ora.build_standard_form(md)
    ok, x, z = fc.certificate(sf, sf.basis, sf.nonbasis)
    assert not ok and float(x.min()) >= 0.0 and float(z.min()) <= -1.0
    out, basis, nonbasis, gx, gz = debug_node(md, flags, root, opts=STOP_AT_ONCE)
    assert (out.route, out.fast_iterations) == (fc.ROUTE_REJECTED, 0), (out.route, out.fast_iterations)
    # the STRICT run under the same epsilon stands: OPTIMAL at the slack basis, bit for bit
    assert (out.status, out.iterations, out.objective) == (_ffi.OPTIMAL, 0, 0.0)
    assert basis.tolist() == sf.basis.tolist() and np.array_equal(gx, sf.x) and np.array_equal(gz, sf.z)


def test_sign_check_rejects_a_negative_recomputed_x():
    # warm: the root's optimal basis under a child's bounds is nonsingular and dual feasible, and
    # primal infeasible in the row of the tightened bound
    md, flags = K(30, 4, 41)
    _, root = fc.root_bounds(md, flags)
    _, basis, nonbasis, _, _ = debug_node(md, flags, root)
    child = nodes_bb(md, flags, FAST, node_limit=3, warm_start=1)[2][1]
    bnd = list(root)
    bnd[2 * child[2] + (1 if child[3] < 0 else 0)] = child[4]
    sf = ora.build_standard_form(mr.node_model(md, list(range(len(flags))), bnd))
    ok, x, z = fc.certificate(sf, basis, nonbasis)
    assert not ok and float(x.min()) <= -1e-3 and float(z.min()) >= -1e-9, (float(x.min()), float(z.min()))
    out, b2, _, x2, _ = debug_node(md, flags, bnd, start_basis=basis, opts=STOP_AT_ONCE)
    assert (out.route, out.fast_iterations) == (fc.ROUTE_REJECTED, 0), (out.route, out.fast_iterations)
    assert (out.status, out.iterations, out.objective) == (_ffi.OPTIMAL, 0, 0.0)
    assert b2.tolist() == sf.basis.tolist() and np.array_equal(x2, sf.x)
    # with the default epsilon the same start is pivoted to the child's optimum and accepted
    fine, _, _, x3, z3 = debug_node(md, flags, bnd, start_basis=basis)
    assert fine.route == fc.ROUTE_FAST and float(x3.min()) >= -1e-9 and float(z3.min()) >= -1e-9


def test_a_search_of_rejected_optima_is_the_strict_search():
    md, flags = K(30, 4, 41)
    ref = nodes_bb(md, flags, call="solve", opts=STOP_AT_ONCE, warm_start=1)
    res, values, log, route = nodes_bb(md, flags, FAST, opts=STOP_AT_ONCE, warm_start=1)
    assert log == ref[2] and np.array_equal(values, ref[1]) and len(log) >= 1
    assert (res.status, res.objective, res.lp_iterations) == (ref[0].status, ref[0].objective, ref[0].lp_iterations)
    assert route == [fc.ROUTE_REJECTED] * len(log)
    assert res.fast_stats == (len(log), len(log), 0, res.lp_iterations), res.fast_stats


# ------------------------------------------------------------------ 6. invariance and the off switch
def test_the_same_call_twice_is_the_same_bits():
    md, flags = K(30, 4, 41)
    a = nodes_bb(md, flags, FAST, node_limit=60, warm_start=1)
    b = nodes_bb(md, flags, FAST, node_limit=60, warm_start=1)
    assert a[2] == b[2] and a[3] == b[3] and np.array_equal(a[1], b[1])
    assert a[0].fast_stats == b[0].fast_stats and a[0].warm_stats == b[0].warm_stats
    assert (a[0].status, a[0].objective, a[0].lp_iterations) == (b[0].status, b[0].objective, b[0].lp_iterations)


def test_refactor_and_slicing_knobs_keep_the_answer():
    for md, flags in (K(16, 3, 41), _models()[3]):
        base = nodes_bb(md, flags, FAST, warm_start=1)[0]
        for node in ({"refactor_every": 2}, {"pivots_per_launch": 1}, {"pivots_per_launch": 5}):
            res, values, log, route = nodes_bb(md, flags, {**FAST, **node}, warm_start=1)
            assert res.status == base.status, node
            if base.has_incumbent:
                assert fc.within_tol(res.objective, base.objective), (node, res.objective, base.objective)
            fc.check_search(md, flags, res, values, log, route)


def test_null_and_strict_node_options_are_dzg_mip_solve():
    for md, flags in _models()[:4] + [K(15, 3, 41)]:
        for mo in ({}, {"warm_start": 1}):
            ref = nodes_bb(md, flags, call="solve", **mo)
            for node in (None, {"numerics": "strict"}, {"numerics": "strict", "refactor_every": 3}):
                got = nodes_bb(md, flags, node, **mo)
                assert got[2] == ref[2] and np.array_equal(got[1], ref[1])
                assert got[0].warm_stats == ref[0].warm_stats and got[0].fast_stats == (0, 0, 0, 0)
                assert (got[0].status, got[0].objective, got[0].lp_iterations, got[0].rounds) == (
                    ref[0].status, ref[0].objective, ref[0].lp_iterations, ref[0].rounds)
                if node is not None:
                    assert set(got[3]) <= {fc.ROUTE_STRICT}


def test_fast_nodes_on_the_surface():
    # tests/test_gpu_mip_warm.py's knapsack: weights 12 2 1 1 4, values 4 2 1 2 10, capacity 15
    w, v = [12, 2, 1, 1, 4], [4, 2, 1, 2, 10]
    xs = [dz.Variable.binary() for _ in w]
    prob = dz.Maximize(sum(vi * xi for vi, xi in zip(v, xs))).subject_to(
        sum(wi * xi for wi, xi in zip(w, xs)) <= 15)
    plain = prob.solve()
    assert plain.mip.nodes_fast_accepted is None and plain.mip.nodes_fast_rejected is None
    rs.set_mip_options(node_numerics="fast")
    try:
        sol = prob.solve()
        low = dz.Minimize(sum(-vi * xi for vi, xi in zip(v, xs))).subject_to(
            sum(wi * xi for wi, xi in zip(w, xs)) <= 15).solve()
    finally:
        rs.set_mip_options()
    assert sol.objective_value == 15.0 and [round(sol[xi]) for xi in xs] == [0, 1, 1, 1, 1]
    assert sol.mip.nodes_fast_accepted > 0 and sol.mip.nodes_fast_rejected >= 0 and sol.mip.status == "optimal"
    assert sol._solution.numerics == plain._solution.numerics == "strict"  # the solution's numerics is unchanged
    assert low.objective_value == -15.0 and low.mip.nodes_fast_accepted == sol.mip.nodes_fast_accepted
    obj, cons = prob._rust_problem()
    per_call = rs.solve_mip(obj, cons, node_numerics="fast", warm_start=True)
    assert per_call.objective_value == 15.0 and per_call.mip.nodes_fast_accepted > 0
