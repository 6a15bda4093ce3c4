"""A Python branch and bound that follows dzg_mip_solve's spec (include/dantzig_amd.h,
dantzig_amd/csrc/mip.cpp) step for step, solving every node LP with the CPU oracle on the node
model.  It emits the same node log as dzg_mip_node: (id, parent, branch_var, direction, bound,
status, iterations, objective).  Not a test: tests/test_mip_host.py checks it against exhaustive
enumeration, tests/test_gpu_mip.py checks the GPU search against it."""
from __future__ import annotations

import itertools
import math

import numpy as np

from oracle import oracle as ora

STATUS = {"optimal": 0, "unbounded": 1, "infeasible": 2, "iter_limit": 3, "singular": 4, "panic": 5}
INF = math.inf


def node_model(model: dict, ints: list, bnd: list) -> dict:
    """The user's model with each integer variable's bounds replaced by the node's."""
    md = dict(model)
    md["vars"] = [dict(v) for v in model["vars"]]
    for k, u in enumerate(ints):
        lo, hi = bnd[2 * k], bnd[2 * k + 1]
        md["vars"][u]["lb"] = None if lo == -INF else lo
        md["vars"][u]["ub"] = None if hi == INF else hi
    return md


def branch_choice(values, ints, int_tol):
    """(branch index into ints or -1, its value, integral) -- mip_branch_choice."""
    best, best_score, integral = -1, -1.0, True
    for k, u in enumerate(ints):
        v = float(values[u])
        if not (abs(v - round(v)) <= int_tol):
            integral = False
        f = v - math.floor(v)
        score = min(f, 1.0 - f)
        if score > best_score:
            best_score, best = score, k
    if integral or best < 0:
        return -1, 0.0, integral
    return best, float(values[ints[best]]), False


def solve_node(model: dict):
    r = ora.solve_model(model)
    return STATUS[r.status], int(r.iterations), float(r.objective), r.values


def branch_and_bound(model: dict, is_integer, *, nodes_per_round=1024, node_limit=100000,
                     int_tol=1e-6, abs_gap=1e-9, rel_gap=0.0, solve=solve_node, map_fn=map):
    ints = [u for u, f in enumerate(is_integer) if f]
    root_bnd = []
    for u in ints:
        v = model["vars"][u]
        root_bnd += [-INF if v.get("lb") is None else float(v["lb"]),
                     INF if v.get("ub") is None else float(v["ub"])]
    nodes = [dict(id=0, parent=-1, branch_var=-1, direction=0, bound=0.0, parent_obj=INF, bnd=root_bnd)]
    open_ = {0}
    inc, inc_values, inc_node = None, None, -1
    log = []
    solved = rounds = iters = pruned = dropped = 0
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
        # the node models are built by the solving function itself, so a thread pool's map builds
        # them in its workers
        results = list(map_fn(lambda b: solve(node_model(model, ints, b)), [nodes[i]["bnd"] for i in rnd]))
        solved += len(rnd)
        for i, (st, it, obj, values) in zip(rnd, results):
            nd = nodes[i]
            iters += it
            log.append((i, nd["parent"], nd["branch_var"], nd["direction"], nd["bound"], st, it,
                        obj if st == 0 else None))
            if st == STATUS["infeasible"]:
                dropped += 1
                continue
            if st != 0:
                status, failed = st, i
                break
            if inc is not None and obj <= inc + tol():
                pruned += 1
                continue
            k, v, integral = branch_choice(values, ints, int_tol)
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
                                  parent_obj=obj, bnd=cb))
                open_.add(len(nodes) - 1)
        if status is not None:
            break
    if status is None:
        status = "optimal" if inc is not None else "infeasible"
    return dict(status=status, objective=inc, values=inc_values, incumbent_node=inc_node, log=log,
                nodes_solved=solved, rounds=rounds, lp_iterations=iters, nodes_pruned=pruned,
                nodes_dropped=dropped, failed_node=failed)


def enumerate_optimum(model: dict):
    """Pure-integer, bounded models: max over every integral point (None if infeasible)."""
    vs = model["vars"]
    ranges = [range(int(v["lb"]), int(v["ub"]) + 1) for v in vs]
    best = None
    for pt in itertools.product(*ranges):
        if all(sum(c * pt[u] for u, c in con["terms"]) <= con["b"] + 1e-9 for con in model["constraints"]):
            val = model["objective"].get("constant", 0.0) + sum(c * pt[u] for u, c in model["objective"]["terms"])
            best = val if best is None else max(best, val)
    return best


def random_pure_milp(rng, nvars=None):
    """A small bounded pure-integer model (binaries and small ranges), integer data."""
    nv = int(rng.integers(2, 7)) if nvars is None else nvars
    vs = []
    for _ in range(nv):
        if rng.integers(0, 2):
            vs.append({"lb": 0.0, "ub": 1.0})
        else:
            lo = float(rng.integers(-2, 1))
            vs.append({"lb": lo, "ub": lo + float(rng.integers(1, 4))})
    obj = {"terms": [[u, float(rng.integers(-5, 10))] for u in range(nv)], "constant": float(rng.integers(-3, 4))}
    cons = []
    for _ in range(int(rng.integers(1, 5))):
        idx = rng.choice(nv, size=int(rng.integers(1, nv + 1)), replace=False)
        cons.append({"terms": [[int(u), float(rng.integers(-3, 7)) + 0.5 * float(rng.integers(0, 2))] for u in idx],
                     "b": float(rng.integers(0, 9)) + 0.5})
    return {"vars": vs, "objective": obj, "constraints": cons}, [1] * nv


def random_mixed_milp(rng):
    """Binaries, bounded integers, integers with no ub (new structures appear mid-tree), free
    integers and continuous variables; bounded in total by a budget row over nonnegative parts."""
    nv = int(rng.integers(3, 8))
    vs, flags = [], []
    for _ in range(nv):
        kind = int(rng.integers(0, 5))
        if kind == 0:
            vs.append({"lb": 0.0, "ub": 1.0}); flags.append(1)
        elif kind == 1:
            vs.append({"lb": float(rng.integers(-2, 1)), "ub": float(rng.integers(1, 6))}); flags.append(1)
        elif kind == 2:
            vs.append({"lb": 0.0, "ub": None}); flags.append(1)
        elif kind == 3:
            vs.append({"lb": None, "ub": None}); flags.append(1)
        else:
            vs.append({"lb": 0.0, "ub": float(rng.integers(1, 5)) + 0.5}); flags.append(0)
    obj = {"terms": [[u, float(rng.integers(-4, 9))] for u in range(nv)], "constant": 0.0}
    cons = []
    # |x_u| bounded for every variable: x_u <= B and -x_u <= B keep the root bounded
    for u in range(nv):
        cons.append({"terms": [[u, 1.0]], "b": 7.5})
        cons.append({"terms": [[u, -1.0]], "b": 6.5})
    for _ in range(int(rng.integers(1, 5))):
        idx = rng.choice(nv, size=int(rng.integers(2, nv + 1)), replace=False)
        cons.append({"terms": [[int(u), float(rng.integers(1, 9)) / float(rng.integers(1, 4))] for u in idx],
                     "b": float(rng.integers(3, 20)) + 0.5})
    return {"vars": vs, "objective": obj, "constraints": cons}, flags


def c_arrays(model: dict) -> dict:
    """The arrays of dzg_model (rust.lower's layout) for a model dict, variables in table order."""
    vs = model["vars"]
    ot = model["objective"]["terms"]
    cons = model.get("constraints", [])
    con_ptr, cv, cc, cb = [0], [], [], []
    for con in cons:
        for u, c in con["terms"]:
            cv.append(u)
            cc.append(c)
        con_ptr.append(len(cv))
        cb.append(con["b"])
    return dict(
        has_lb=np.array([v.get("lb") is not None for v in vs] + [False], dtype=np.int32),
        has_ub=np.array([v.get("ub") is not None for v in vs] + [False], dtype=np.int32),
        lb=np.array([0.0 if v.get("lb") is None else v["lb"] for v in vs] + [0.0]),
        ub=np.array([0.0 if v.get("ub") is None else v["ub"] for v in vs] + [0.0]),
        obj_var=np.array([t[0] for t in ot] + [0], dtype=np.int64),
        obj_coef=np.array([t[1] for t in ot] + [0.0]),
        con_ptr=np.array(con_ptr, dtype=np.int64), con_var=np.array(cv + [0], dtype=np.int64),
        con_coef=np.array(cc + [0.0]), con_b=np.array(cb + [0.0]),
        nvars=len(vs), obj_nterms=len(ot), ncons=len(cons),
        obj_const=float(model["objective"].get("constant", 0.0)))
