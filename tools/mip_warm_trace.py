"""Where the time of one warm-started search sits: splits the k_mip_node launches of a
rocprofv3 --kernel-trace CSV into rounds, and the rounds into cold (the root, structure changes),
restart (a round that holds a restarted node) and warm.

The search is replayed with the warm reference (tests/mip_warm_reference.py); a round of one row
bucket takes max over its nodes of the slices each needs (pivots // pivots_per_launch + 1 per run,
a restarted node's two runs added), which names the launches of the trace in order.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o NAME -- \\
        python tools/mip_warm_trace.py --run knap 1001
    python tools/mip_warm_trace.py knap 1001 OUT/NAME_kernel_trace.csv
"""
from __future__ import annotations

import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mip_bench  # noqa: E402
from tests import mip_reference as mr  # noqa: E402
from tests import mip_warm_reference as mw  # noqa: E402

PPL = 16  # the default pivots_per_launch
NODE_LIMIT = 5000


def model(family: str, seed: int):
    return {"knap": mip_bench.knapsack, "gap": mip_bench.gap}[family](seed)


def run(family: str, seed: int) -> None:
    from dantzig_amd import rust as rs

    md, flags = model(family, seed)
    res, _, _ = rs._mip_call(mr.c_arrays(md), flags, 0, node_limit=NODE_LIMIT, warm_start=1)
    print(json.dumps(dict(status=int(res.status), nodes=int(res.nodes_solved), rounds=int(res.rounds),
                          lp_pivots=int(res.lp_iterations), warm_stats=res.warm_stats)))


def split(family: str, seed: int, trace: str) -> None:
    md, flags = model(family, seed)
    rounds = []

    def record(fn, items):
        out = [fn(i) for i in items]
        rounds.append([(r[1], r[4], r[5], r[6]) for r in out])  # pivots, warm, restarted, warm pivots
        return out

    mw.branch_and_bound_warm(md, flags, node_limit=NODE_LIMIT, map_fn=record)
    with open(trace) as f:
        stamps = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)
                  if "k_mip_node" in r["Kernel_Name"]]
    launches = [e - b for b, e in stamps]

    def slices(p):
        return p // PPL + 1

    plan = []
    for rd in rounds:
        need = max(slices(wit) + slices(total - wit) if restarted else slices(total)
                   for total, _, restarted, wit in rd)
        kind = "restart" if any(r for _, _, r, _ in rd) else "warm" if all(w for _, w, _, _ in rd) else "cold"
        plan.append((kind, need, len(rd), max(t for t, _, _, _ in rd)))
    if sum(n for _, n, _, _ in plan) != len(launches):
        raise SystemExit(f"the trace holds {len(launches)} k_mip_node launches, the replay needs "
                         f"{sum(n for _, n, _, _ in plan)}: not this search, or several row buckets")
    at = 0
    total = {}
    for kind, need, nodes, pivots in plan:
        ns = sum(launches[at:at + need])
        at += need
        t = total.setdefault(kind, [0, 0, 0])
        t[0] += 1
        t[1] += need
        t[2] += ns
        print(f"{kind:8s} launches {need:3d}  nodes {nodes:5d}  most pivots in a node {pivots:4d}  {ns / 1e6:9.2f} ms")
    for kind, (nr, nl, ns) in total.items():
        print(f"{kind}: {nr} rounds, {nl} launches, {ns / 1e6:.1f} ms")
    print(f"first k_mip_node start to last end: {(stamps[-1][1] - stamps[0][0]) / 1e6:.1f} ms, "
          f"inside the launches {sum(launches) / 1e6:.1f} ms")


if __name__ == "__main__":
    if sys.argv[1] == "--run":
        run(sys.argv[2], int(sys.argv[3]))
    else:
        split(sys.argv[1], int(sys.argv[2]), sys.argv[3])
