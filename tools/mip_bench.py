"""Branch and bound throughput (dzg_mip_solve) against the same tree on the CPU oracle.

Workloads, seeded:
    knap   3-dimensional 0/1 knapsacks, 30-60 binaries (63-123 rows with the bound rows),
           uncorrelated values: best-first search reaches the optimum in a few hundred to a few
           thousand nodes
    gap    bounded-integer generalised assignment models (3 agents x 6-9 jobs, x_ij in {0..3})

Per model, one JSON line: nodes, rounds, LP pivots, GPU wall time and nodes/s, and the CPU
baseline: tests/mip_reference.py's search (the same tree: same selection, branching and pruning)
with each round's node LPs solved by the oracle on 16 threads (ctypes releases the GIL).  Each
worker builds its node model itself.  `oracle16_lp_s` is the time inside those per-round maps only
(node models and node LPs); `oracle16_total_s` adds the serial Python search around them.  The
speed-up is taken against `oracle16_lp_s`.  `equal` says whether the GPU's status, node count,
objective and values equal the baseline's bit for bit.

    python tools/mip_bench.py [--models 4] [--node-limit 5000] [--out profiles/mip_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dantzig_amd import rust as rs  # noqa: E402
from tests import mip_reference as mr  # noqa: E402


def knapsack(seed: int):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(30, 61))
    dims = 3
    w = rng.integers(1, 15, (dims, n)).astype(float)
    v = rng.integers(1, 100, n).astype(float)
    cons = [{"terms": [[u, float(w[d, u])] for u in range(n)], "b": float(w[d].sum() // 2)}
            for d in range(dims)]
    return ({"vars": [{"lb": 0.0, "ub": 1.0} for _ in range(n)],
             "objective": {"terms": [[u, float(v[u])] for u in range(n)], "constant": 0.0},
             "constraints": cons}, [1] * n)


def gap(seed: int):
    rng = np.random.default_rng(seed)
    agents, jobs = 3, int(rng.integers(6, 10))
    nv = agents * jobs
    cost = rng.integers(1, 20, (agents, jobs)).astype(float)
    size = rng.integers(2, 9, (agents, jobs)).astype(float)
    cons = []
    for j in range(jobs):  # every job covered once or twice: sum_i x_ij in [1, 2]
        cons.append({"terms": [[i * jobs + j, 1.0] for i in range(agents)], "b": 2.0})
        cons.append({"terms": [[i * jobs + j, -1.0] for i in range(agents)], "b": -1.0})
    for i in range(agents):
        cons.append({"terms": [[i * jobs + j, float(size[i, j])] for j in range(jobs)],
                     "b": float(size[i].sum() * 0.5) + 0.5})
    return ({"vars": [{"lb": 0.0, "ub": 3.0} for _ in range(nv)],
             "objective": {"terms": [[i * jobs + j, -float(cost[i, j])] for i in range(agents)
                                     for j in range(jobs)], "constant": 0.0},
             "constraints": cons}, [1] * nv)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=4)
    ap.add_argument("--node-limit", type=int, default=5000)
    ap.add_argument("--nodes-per-round", type=int, default=1024)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mip_bench.jsonl"))
    args = ap.parse_args()
    pool = ThreadPoolExecutor(max_workers=16)
    lines = []
    for family, maker in (("knap", knapsack), ("gap", gap)):
        for k in range(args.models):
            md, flags = maker(1000 + k)
            mo = dict(node_limit=args.node_limit, nodes_per_round=args.nodes_per_round)
            rs._mip_call(mr.c_arrays(md), flags, 0, node_limit=1)  # warm-up: device, code objects
            arrays = mr.c_arrays(md)
            t0 = time.perf_counter()
            res, values, _ = rs._mip_call(arrays, flags, 0, **mo)
            gpu_s = time.perf_counter() - t0
            line = dict(family=family, seed=1000 + k, nvars=len(flags),
                        status=int(res.status), objective=res.objective if res.has_incumbent else None,
                        nodes=int(res.nodes_solved), rounds=int(res.rounds),
                        lp_pivots=int(res.lp_iterations), batched=int(res.nodes_batched),
                        gpu_s=gpu_s, gpu_nodes_per_s=res.nodes_solved / gpu_s)
            if not args.no_oracle:
                lp_s = [0.0]

                def timed_map(fn, items):
                    t = time.perf_counter()
                    out = list(pool.map(fn, items))
                    lp_s[0] += time.perf_counter() - t
                    return out

                t0 = time.perf_counter()
                ref = mr.branch_and_bound(md, flags, map_fn=timed_map, **mo)
                cpu_s = time.perf_counter() - t0
                want = {"optimal": 0, "infeasible": 2, "node_limit": 8}.get(ref["status"], ref["status"])
                same_inc = (ref["objective"] is None and not res.has_incumbent) or (
                    ref["objective"] is not None and bool(res.has_incumbent) and ref["objective"] == res.objective
                    and np.array_equal(ref["values"], values[:len(flags)]))
                line.update(oracle16_lp_s=lp_s[0], oracle16_total_s=cpu_s,
                            oracle16_nodes_per_s=ref["nodes_solved"] / lp_s[0], speedup=lp_s[0] / gpu_s,
                            equal=bool(want == res.status and ref["nodes_solved"] == res.nodes_solved
                                       and same_inc))
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
