"""The warm-started branch and bound (dzg_mip_opts.warm_start = 1) in Python over the
CPU oracle: tests/mip_reference.py's search, with each node LP following the warm node spec.

A child is warm when it and its parent have the same set of finite integer bounds (one structure)
and that structure goes through the batched kernel (<= 128 rows).  A warm node starts from its
parent's final basis, nonbasis and carried z, bars at one, x = lu_solve(B, b); the attempt stands
only if it ends optimal with every carried x and z >= -WARM_TOL, otherwise the node is solved again
cold and the cold result is the node's, its logged iterations the sum of both runs.

Emits branch_and_bound's dict (same log tuples) plus `flags`, one (warm, restarted) pair per log
entry, and the four counters of dzg_mip_last_warm_stats.  Not a test: tests/test_mip_warm_host.py
checks it against the cold reference, tests/test_gpu_mip_warm.py checks the GPU search against it."""
from __future__ import annotations

import math
import os
import re

import numpy as np

from oracle import oracle as ora
from tests import mip_reference as mr

INF = math.inf


def _header_define(name: str) -> float:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "dantzig_amd.h")) as f:
        return float(re.search(r"#define " + name + r" (\S+)", f.read()).group(1))


WARM_TOL = _header_define("DZG_MIP_WARM_TOL")  # the acceptance tolerance is the header's
BATCH_MAX_ROWS = 128  # DZG_BATCH_MAX_ROWS


def mask_of(bnd) -> tuple:
    return tuple(not math.isinf(b) for b in bnd)


def solve_warm_node(model: dict, ints: list, bnd: list, parent_state, attempts=None):
    """One node LP.  parent_state: None (cold) or the parent's dict(mask, basis, nonbasis, z).
    Returns (status, iterations, objective, values, warm, restarted, warm_iterations, state);
    `state` is the node's own final state when it ended optimal on the batched route.  `attempts`,
    if a list, collects (status, min over carried x and z) of every warm attempt."""
    sf = ora.build_standard_form(mr.node_model(model, ints, bnd))
    mask = mask_of(bnd)
    warm = parent_state is not None and parent_state["mask"] == mask and sf.m <= BATCH_MAX_ROWS
    restarted, warm_it = False, 0
    res = None
    if warm:
        dense = ora.csc_to_dense(sf.m, sf.n, sf.col_ptr, sf.row_idx, sf.val)
        wf = ora.StdForm(m=sf.m, n=sf.n, col_ptr=sf.col_ptr, row_idx=sf.row_idx, val=sf.val, c=sf.c,
                         constant=sf.constant, basis=parent_state["basis"].copy(),
                         nonbasis=parent_state["nonbasis"].copy(),
                         x=ora.lu_solve(np.ascontiguousarray(dense[:, parent_state["basis"]]), sf.x),
                         z=parent_state["z"].copy(), pos_col=sf.pos_col, neg_col=sf.neg_col)
        res = ora.simplex_solve(wf, xbar=np.ones(sf.m), zbar=np.ones(sf.n - sf.m))
        warm_it = int(res.iterations)
        ok = res.status == "optimal" and bool(np.all(res.x >= -WARM_TOL)) and bool(np.all(res.z >= -WARM_TOL))
        if attempts is not None:
            low = min(float(np.min(res.x, initial=INF)), float(np.min(res.z, initial=INF)))
            attempts.append((res.status, low))
        if not ok:
            restarted, res = True, None
    if res is None:
        res = ora.simplex_solve(sf)
    st = mr.STATUS[res.status]
    values = ora.solution_values(sf, res)
    state = None
    if st == 0 and sf.m <= BATCH_MAX_ROWS:
        state = dict(mask=mask, basis=res.basis.copy(), nonbasis=res.nonbasis.copy(), z=res.z.copy())
    total = int(res.iterations) + (warm_it if restarted else 0)
    return st, total, float(res.objective), values, warm, restarted, warm_it, state


def branch_and_bound_warm(model: dict, is_integer, *, nodes_per_round=1024, node_limit=100000,
                          int_tol=1e-6, abs_gap=1e-9, rel_gap=0.0, map_fn=map, attempts=None):
    ints = [u for u, f in enumerate(is_integer) if f]
    root_bnd = []
    for u in ints:
        v = model["vars"][u]
        root_bnd += [-INF if v.get("lb") is None else float(v["lb"]),
                     INF if v.get("ub") is None else float(v["ub"])]
    nodes = [dict(id=0, parent=-1, branch_var=-1, direction=0, bound=0.0, parent_obj=INF, bnd=root_bnd,
                  state=None)]
    open_ = {0}
    inc, inc_values, inc_node = None, None, -1
    log, flags = [], []
    solved = rounds = iters = pruned = dropped = 0
    nodes_warm = nodes_restarted = warm_iterations = restart_iterations = 0
    status, failed = None, -1

    def tol():
        return max(abs_gap, rel_gap * abs(inc))

    while open_:
        order = sorted(open_, key=lambda i: (-nodes[i]["parent_obj"], i))
        rnd = []
        for i in order:
            if len(rnd) >= nodes_per_round:
                break
            if inc is not None and nodes[i]["parent_obj"] <= inc + tol():
                open_.discard(i)
                nodes[i]["state"] = None
                pruned += 1
                continue
            if solved + len(rnd) >= node_limit:
                break
            open_.discard(i)
            rnd.append(i)
        if not rnd:
            if open_:
                status = "node_limit"
            break
        rnd.sort()
        rounds += 1
        results = list(map_fn(lambda i: solve_warm_node(model, ints, nodes[i]["bnd"], nodes[i]["state"],
                                                        attempts), rnd))
        solved += len(rnd)
        for i, (st, it, obj, values, warm, restarted, warm_it, state) in zip(rnd, results):
            nd = nodes[i]
            nd["state"] = None  # the parent's state is needed no longer
            iters += it
            nodes_warm += warm
            nodes_restarted += restarted
            warm_iterations += warm_it
            restart_iterations += it - warm_it if restarted else 0
            log.append((i, nd["parent"], nd["branch_var"], nd["direction"], nd["bound"], st, it,
                        obj if st == 0 else None))
            flags.append((bool(warm), bool(restarted)))
            if st == mr.STATUS["infeasible"]:
                dropped += 1
                continue
            if st != 0:
                status, failed = st, i
                break
            if inc is not None and obj <= inc + tol():
                pruned += 1
                continue
            k, v, integral = mr.branch_choice(values, ints, int_tol)
            if integral:
                inc, inc_values, inc_node = obj, np.array(values, dtype=float), i
                continue
            if k < 0:
                dropped += 1
                continue
            fl = float(math.floor(v))
            for d in (-1, 1):
                cb = list(nd["bnd"])
                if d < 0:
                    nb = min(cb[2 * k + 1], fl)
                    cb[2 * k + 1] = nb
                else:
                    nb = max(cb[2 * k], fl + 1.0)
                    cb[2 * k] = nb
                if cb[2 * k] > cb[2 * k + 1]:
                    dropped += 1
                    continue
                nodes.append(dict(id=len(nodes), parent=i, branch_var=ints[k], direction=d, bound=nb,
                                  parent_obj=obj, bnd=cb, state=state))
                open_.add(len(nodes) - 1)
        if status is not None:
            break
    if status is None:
        status = "optimal" if inc is not None else "infeasible"
    return dict(status=status, objective=inc, values=inc_values, incumbent_node=inc_node, log=log,
                flags=flags, nodes_solved=solved, rounds=rounds, lp_iterations=iters,
                nodes_pruned=pruned, nodes_dropped=dropped, failed_node=failed,
                nodes_warm=nodes_warm, nodes_restarted=nodes_restarted,
                warm_iterations=warm_iterations, restart_iterations=restart_iterations)
