"""A warm batch against a cold one (dzg_batch_solve_from, core.solve_batch(start=...)).

The README's batch workload: 4 096 LPs at 64 x 128 from gen_dense_lp.  They are solved cold once;
then (b, c) of every LP moves by tests/reopt_check.moved at scales 1e-3, 1e-1 and 1, and the changed
LPs are solved twice, alternately, --repeats times each, in this one process on one device:

    warm   solve_batch(changed, start=previous)    every LP from the basis its first solve ended on
    cold   solve_batch(changed)                    every LP from the slack basis

Per scale: each side's wall times (a host clock around the call, which ends in a device
synchronise; uploads and downloads included), their minimum and spread (max - min), total pivots,
the device time of the restart launches alone (events around them on the call's stream,
dzg_debug_batch_restart_ms), the statuses, and the largest relative difference between the warm and
the cold objective of an LP that ended optimal both ways.  No threshold on time: the tool reports.

    python tools/batch_reopt_bench.py [--lps 4096] [--m 64] [--ns 128] [--repeats 5] [--out profiles/batch_reopt_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dantzig_amd import _ffi, core  # noqa: E402
from tests.reopt_check import moved  # noqa: E402

SCALES = (1e-3, 1e-1, 1.0)


def side(times, results) -> dict:
    lo = min(times)
    return dict(wall_s=[round(t, 4) for t in times], min_s=round(lo, 4), spread_s=round(max(times) - lo, 4),
                total_pivots=int(sum(r.iterations for r in results)),
                statuses={s: sum(r.status == s for r in results) for s in sorted({r.status for r in results})})


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lps", type=int, default=4096)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--ns", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ppl", type=int, default=0, help="pivots per launch (0 = the library's default)")
    ap.add_argument("--out", default=None, help="write the JSON document to this file as well")
    args = ap.parse_args()
    data = [core.gen_dense_lp(seed=1_000_000 + i, m=args.m, n_struct=args.ns) for i in range(args.lps)]
    data = [(np.array(a), b, c) for a, b, c in data]
    lps = [core.CoreLP.from_inequality_form(a, b, c) for a, b, c in data]
    kw = dict(log=False, pivots_per_launch=args.ppl)
    head = core.solve_batch(lps[:64], **kw)  # warm-up: both paths, every kernel
    core.solve_batch(lps[:64], start=head, **kw)
    previous = core.solve_batch(lps, **kw)
    doc = dict(tool="tools/batch_reopt_bench.py", lps=args.lps, m=args.m, n_struct=args.ns, repeats=args.repeats,
               pivots_per_launch=args.ppl or "default",
               first_cold=dict(wall_s=round(previous[0].solve_ms / 1e3, 4),
                               total_pivots=int(sum(r.iterations for r in previous))),
               scales=[])
    for scale in SCALES:
        changed = []
        for i, (a, b, c) in enumerate(data):
            b2, c2 = moved(i, b, c, scale=scale)
            changed.append(core.CoreLP.from_inequality_form(a, b2, c2))
        warm_s, cold_s, restart_ms = [], [], []
        for _ in range(args.repeats):
            warm = core.solve_batch(changed, start=previous, **kw)
            warm_s.append(warm[0].solve_ms / 1e3)
            restart_ms.append(float(_ffi.lib().dzg_debug_batch_restart_ms()))
            cold = core.solve_batch(changed, **kw)
            cold_s.append(cold[0].solve_ms / 1e3)
        both = [(w.objective, c.objective) for w, c in zip(warm, cold) if w.status == c.status == "optimal"]
        diff = max((abs(w - c) / max(1.0, abs(c)) for w, c in both), default=0.0)
        w, c = side(warm_s, warm), side(cold_s, cold)
        entry = dict(scale=scale, warm=w, cold=c,
                     restart_launches_ms=[round(t, 3) for t in restart_ms], restart_launches_min_ms=round(min(restart_ms), 3),
                     cold_over_warm=round(c["min_s"] / w["min_s"], 3),
                     warm_beats_cold_by_more_than_the_spread=bool(c["min_s"] - w["min_s"] > max(w["spread_s"], c["spread_s"])),
                     same_statuses=bool(all(x.status == y.status for x, y in zip(warm, cold))),
                     optimal_both_ways=len(both), max_rel_objective_diff=float(diff))
        doc["scales"].append(entry)
        print(json.dumps(entry), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
