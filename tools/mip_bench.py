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

--warm measures the warm-started search (dzg_mip_opts.warm_start = 1) instead: per model, after a
warm-up solve of each kind, the cold and the warm GPU search are run alternately `--repeats` times
(3); the minimum of each is reported with its spread (max - min).  The CPU baseline is the warm
reference search (tests/mip_warm_reference.py) with its node LPs on 16 oracle threads; `equal`
says whether the warm GPU search equals it bit for bit (status, nodes, rounds, pivots, objective,
values, warm counters).  One JSON line per model to profiles/mip_bench_warm.jsonl.

    python tools/mip_bench.py --warm [--models 4] [--node-limit 5000] [--repeats 3]

--fast measures the FAST node LPs (dzg_mip_solve_nodes, numerics = FAST): per model three modes
alternate in one process `--repeats` times after a warm-up of each -- cold STRICT, warm STRICT and
warm FAST -- and each reports its minimum, its spread (max - min), nodes, rounds and pivots; warm
FAST also its accepted and rejected attempts.  The baseline is the 16-thread warm oracle of --warm.
One JSON line per model to profiles/mip_bench_fast.jsonl.

    python tools/mip_bench.py --fast [--models 4] [--node-limit 5000] [--repeats 3]
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
from tests import mip_warm_reference as mw  # noqa: E402


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


def warm_line(family, seed, md, flags, mo, repeats, pool):
    arrays = mr.c_arrays(md)
    for w in (0, 1):  # warm-up: device, code objects, allocator
        rs._mip_call(arrays, flags, 0, warm_start=w, **mo)
    times = {0: [], 1: []}
    got = {}
    for _ in range(repeats):
        for w in (0, 1):
            t0 = time.perf_counter()
            got[w] = rs._mip_call(arrays, flags, 0, warm_start=w, **mo)
            times[w].append(time.perf_counter() - t0)
    (cold, _, _), (res, values, _) = got[0], got[1]
    cold_s, warm_s = min(times[0]), min(times[1])
    line = dict(family=family, seed=seed, nvars=len(flags), status=int(res.status),
                objective=res.objective if res.has_incumbent else None,
                cold_status=int(cold.status), cold_objective=cold.objective if cold.has_incumbent else None,
                nodes_cold=int(cold.nodes_solved), nodes_warm_search=int(res.nodes_solved),
                rounds_cold=int(cold.rounds), rounds_warm=int(res.rounds),
                lp_pivots_cold=int(cold.lp_iterations), lp_pivots_warm=int(res.lp_iterations),
                warm_attempts=res.warm_stats[0], restarts=res.warm_stats[1],
                warm_pivots=res.warm_stats[2], restart_pivots=res.warm_stats[3],
                gpu_cold_s=cold_s, gpu_cold_spread_s=max(times[0]) - cold_s,
                gpu_warm_s=warm_s, gpu_warm_spread_s=max(times[1]) - warm_s,
                gpu_warm_over_cold=cold_s / warm_s, repeats=repeats)
    lp_s = [0.0]

    def timed_map(fn, items):
        t = time.perf_counter()
        out = list(pool.map(fn, items))
        lp_s[0] += time.perf_counter() - t
        return out

    t0 = time.perf_counter()
    ref = mw.branch_and_bound_warm(md, flags, map_fn=timed_map, **mo)
    cpu_s = time.perf_counter() - t0
    want = {"optimal": 0, "infeasible": 2, "node_limit": 8}.get(ref["status"], ref["status"])
    same_inc = (ref["objective"] is None and not res.has_incumbent) or (
        ref["objective"] is not None and bool(res.has_incumbent) and ref["objective"] == res.objective
        and np.array_equal(ref["values"], values[:len(flags)]))
    same_counts = (ref["nodes_solved"], ref["rounds"], ref["lp_iterations"]) == (
        res.nodes_solved, res.rounds, res.lp_iterations) and res.warm_stats == (
        ref["nodes_warm"], ref["nodes_restarted"], ref["warm_iterations"], ref["restart_iterations"])
    line.update(oracle16_warm_lp_s=lp_s[0], oracle16_warm_total_s=cpu_s, speedup_warm=lp_s[0] / warm_s,
                equal=bool(want == res.status and same_counts and same_inc))
    return line


FAST_MODES = (("cold_strict", {}), ("warm_strict", {"warm_start": 1}),
              ("warm_fast", {"warm_start": 1, "node_numerics": "fast"}))


def fast_line(family, seed, md, flags, mo, repeats, pool):
    """Cold STRICT, warm STRICT and warm FAST node LPs, alternating in one process."""
    arrays = mr.c_arrays(md)
    for _, kw in FAST_MODES:  # warm-up: device, code objects, allocator
        rs._mip_call(arrays, flags, 0, **kw, **mo)
    times = {name: [] for name, _ in FAST_MODES}
    got = {}
    for _ in range(repeats):
        for name, kw in FAST_MODES:
            t0 = time.perf_counter()
            got[name] = rs._mip_call(arrays, flags, 0, **kw, **mo)[0]
            times[name].append(time.perf_counter() - t0)
    line = dict(family=family, seed=seed, nvars=len(flags), rows=len(md["constraints"]) + 2 * len(flags),
                repeats=repeats)
    for name, _ in FAST_MODES:
        res, ts = got[name], times[name]
        line[name] = dict(status=int(res.status), objective=res.objective if res.has_incumbent else None,
                          nodes=int(res.nodes_solved), rounds=int(res.rounds), lp_pivots=int(res.lp_iterations),
                          gpu_s=min(ts), spread_s=max(ts) - min(ts))
    fast = got["warm_fast"].fast_stats
    line["warm_fast"].update(accepted=fast[0], rejected=fast[1])
    lp_s = [0.0]

    def timed_map(fn, items):
        t = time.perf_counter()
        out = list(pool.map(fn, items))
        lp_s[0] += time.perf_counter() - t
        return out

    mw.branch_and_bound_warm(md, flags, map_fn=timed_map, **mo)
    line.update(oracle16_warm_lp_s=lp_s[0],
                **{f"speedup_{name}": lp_s[0] / line[name]["gpu_s"] for name, _ in FAST_MODES})
    return line


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", type=int, default=4)
    ap.add_argument("--node-limit", type=int, default=5000)
    ap.add_argument("--nodes-per-round", type=int, default=1024)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--warm", action="store_true", help="cold vs warm-started GPU search, see above")
    ap.add_argument("--fast", action="store_true", help="cold STRICT, warm STRICT and warm FAST node LPs")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        name = "mip_bench_fast.jsonl" if args.fast else "mip_bench_warm.jsonl" if args.warm else "mip_bench.jsonl"
        args.out = os.path.join(ROOT, "profiles", name)
    pool = ThreadPoolExecutor(max_workers=16)
    lines = []
    for family, maker in (("knap", knapsack), ("gap", gap)):
        for k in range(args.models):
            md, flags = maker(1000 + k)
            mo = dict(node_limit=args.node_limit, nodes_per_round=args.nodes_per_round)
            if args.warm or args.fast:
                line = (fast_line if args.fast else warm_line)(family, 1000 + k, md, flags, mo, args.repeats, pool)
                print(json.dumps(line), flush=True)
                lines.append(line)
                continue
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
