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

--fast measures the FAST batch from its last bases (dzg_batch_solve_fast_from) instead.  Workloads:
4 096 LPs at 64 x 128 and 1 024 LPs at 128 x 256 (or the one --lps / --m / --ns name), solved cold once
by solve_batch_fast (AUTO); then per scale three sides, alternately, --repeats times each after one
warm-up round:

    warm_fast    solve_batch_fast(changed, start=previous)   AUTO: FAST, what it gives up on in STRICT
    warm_strict  solve_batch(changed, start=previous)        dzg_batch_solve_from
    cold_fast    solve_batch_fast(changed)                   AUTO, every LP from the slack basis

Per side: wall times, minimum, spread, total pivots, statuses; for the FAST sides the number of LPs
handed to STRICT; for warm_fast the device time of the restart launches
(dzg_debug_batch_fast_restart_ms) and its share of the call; and per pair of sides whether the
difference of the minima exceeds both spreads.

    python tools/batch_reopt_bench.py --fast [--repeats 5] [--out profiles/batch_fast_reopt_bench.json]

--resident measures the batch kept on the device (dzg_batch, core.BatchSolver) against the stateless
warm call of the same numerics: STRICT, or with --fast AUTO.  The same two workloads and scales.  The
handle is created and solved cold once, outside the window; then per scale two sides, alternately,
--repeats times each after one warm-up round:

    resident    handle.update_many(changed b, c of every LP) + handle.solve()     timed together
    stateless   solve_batch(changed, start=previous) / solve_batch_fast(...)

Between repeats the handle's data is moved back and every LP's start is set to the basis of the cold
solve again (set_start), so every repeat does the same work; the start bases then ride in the next
solve's staging buffer (4 n bytes per LP that a chain of re-solves would not upload: they are part
of the traffic reported).  Per side wall_s is a host clock around the whole Python call, which ends
in a device synchronise (marshalling included: what a caller pays); call_s is the clock around the C
call alone, the figure the other modes of this tool record.  The tool checks that both sides return
identical bits and reports the handle's traffic(): bytes up, bytes down, and the device time of the
stage + restart launches.

    python tools/batch_reopt_bench.py --resident [--fast] [--repeats 5] [--out profiles/batch_resident_bench.json]
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


FAST_WORKLOADS = ((4096, 64, 128), (1024, 128, 256))


def beats(a: dict, b: dict) -> dict:
    """Side a against side b: b's minimum over a's, and whether a is faster by more than both spreads."""
    return dict(ratio=round(b["min_s"] / a["min_s"], 3),
                faster_by_more_than_both_spreads=bool(b["min_s"] - a["min_s"] > max(a["spread_s"], b["spread_s"])),
                slower_by_more_than_both_spreads=bool(a["min_s"] - b["min_s"] > max(a["spread_s"], b["spread_s"])))


def fast_workload(n_lps: int, m: int, ns: int, repeats: int, ppl: int) -> dict:
    data = [core.gen_dense_lp(seed=1_000_000 + i, m=m, n_struct=ns) for i in range(n_lps)]
    data = [(np.array(a), b, c) for a, b, c in data]
    lps = [core.CoreLP.from_inequality_form(a, b, c) for a, b, c in data]
    kw = dict(log=False, pivots_per_launch=ppl)
    previous = core.solve_batch_fast(lps, **kw)
    doc = dict(lps=n_lps, m=m, n_struct=ns,
               first_cold=dict(wall_s=round(previous[0].solve_ms / 1e3, 4),
                               total_pivots=int(sum(r.iterations for r in previous)),
                               handed_to_strict=int(sum(r.numerics == "strict" for r in previous))),
               scales=[])
    sides = dict(warm_fast=lambda ch: core.solve_batch_fast(ch, start=previous, **kw),
                 warm_strict=lambda ch: core.solve_batch(ch, start=previous, **kw),
                 cold_fast=lambda ch: core.solve_batch_fast(ch, **kw))
    for scale in SCALES:
        changed = []
        for i, (a, b, c) in enumerate(data):
            b2, c2 = moved(i, b, c, scale=scale)
            changed.append(core.CoreLP.from_inequality_form(a, b2, c2))
        times = {name: [] for name in sides}
        last, restart_ms = {}, []
        for rep in range(repeats + 1):   # round 0 is the warm-up
            for name, run in sides.items():
                last[name] = run(changed)
                if rep == 0:
                    continue
                times[name].append(last[name][0].solve_ms / 1e3)
                if name == "warm_fast":
                    restart_ms.append(float(_ffi.lib().dzg_debug_batch_fast_restart_ms()))
        out = {name: side(times[name], last[name]) for name in sides}
        for name in ("warm_fast", "cold_fast"):
            out[name]["handed_to_strict"] = int(sum(r.numerics == "strict" for r in last[name]))
        both = [(w.objective, c.objective) for w, c in zip(last["warm_fast"], last["warm_strict"])
                if w.status == c.status == "optimal"]
        diff = max((abs(w - c) / max(1.0, abs(c)) for w, c in both), default=0.0)
        entry = dict(scale=scale, **out,
                     restart_launches_ms=[round(t, 3) for t in restart_ms],
                     restart_launches_min_ms=round(min(restart_ms), 3),
                     restart_share_of_warm_fast=round(min(restart_ms) / 1e3 / out["warm_fast"]["min_s"], 4),
                     warm_fast_vs_warm_strict=beats(out["warm_fast"], out["warm_strict"]),
                     warm_fast_vs_cold_fast=beats(out["warm_fast"], out["cold_fast"]),
                     same_statuses=bool(all(x.status == y.status
                                            for x, y in zip(last["warm_fast"], last["warm_strict"]))),
                     optimal_both_ways=len(both), max_rel_objective_diff=float(diff))
        doc["scales"].append(entry)
        print(json.dumps(dict(lps=n_lps, m=m, n_struct=ns, **entry)), flush=True)
    return doc


def same_bits(a, b) -> bool:
    return all(x.status == y.status and x.iterations == y.iterations and x.numerics == y.numerics
               and x.basis.tobytes() == y.basis.tobytes() and x.nonbasis.tobytes() == y.nonbasis.tobytes()
               and x.x.tobytes() == y.x.tobytes() and x.z.tobytes() == y.z.tobytes()
               and x.xbar.tobytes() == y.xbar.tobytes() and x.zbar.tobytes() == y.zbar.tobytes()
               and np.float64(x.objective).tobytes() == np.float64(y.objective).tobytes() for x, y in zip(a, b))


def resident_workload(n_lps: int, m: int, ns: int, repeats: int, ppl: int, fast: bool) -> dict:
    import time

    data = [core.gen_dense_lp(seed=1_000_000 + i, m=m, n_struct=ns) for i in range(n_lps)]
    data = [(np.array(a), np.array(b), np.array(c)) for a, b, c in data]
    lps = [core.CoreLP.from_inequality_form(a, b, c) for a, b, c in data]
    numerics = core.AUTO if fast else core.STRICT
    stateless = core.solve_batch_fast if fast else core.solve_batch
    kw = dict(log=False, pivots_per_launch=ppl)
    zeros = np.zeros(m)
    back = [(i, b, np.concatenate([c, zeros]), None) for i, (_, b, c) in enumerate(data)]
    t0 = time.perf_counter()
    handle = core.BatchSolver(lps, log_cap=0, pivots_per_launch=ppl, numerics=numerics)
    create_s = time.perf_counter() - t0
    previous = handle.solve(log=False)
    doc = dict(lps=n_lps, m=m, n_struct=ns, numerics="auto" if fast else "strict", create_s=round(create_s, 4),
               first_cold=dict(wall_s=round(previous[0].solve_ms / 1e3, 4),
                               total_pivots=int(sum(r.iterations for r in previous))),
               scales=[])
    for scale in SCALES:
        changed, changes = [], []
        for i, (a, b, c) in enumerate(data):
            b2, c2 = moved(i, b, c, scale=scale)
            changed.append(core.CoreLP.from_inequality_form(a, b2, c2))
            changes.append((i, b2, np.concatenate([c2, zeros]), None))
        wall = dict(resident=[], stateless=[])
        call = dict(resident=[], stateless=[])
        traffic, last = [], {}
        for rep in range(repeats + 1):   # round 0 is the warm-up
            for i, r in enumerate(previous):
                handle.set_start(i, r)
            t0 = time.perf_counter()
            handle.update_many(changes)
            last["resident"] = handle.solve(log=False)
            t1 = time.perf_counter()
            up, down, ms = handle.traffic()
            handle.update_many(back)
            t2 = time.perf_counter()
            last["stateless"] = stateless(changed, start=previous, **kw)
            t3 = time.perf_counter()
            if rep == 0:
                continue
            wall["resident"].append(t1 - t0)
            wall["stateless"].append(t3 - t2)
            for name in call:
                call[name].append(last[name][0].solve_ms / 1e3)
            traffic.append((up, down, ms))
        out = {name: side(wall[name], last[name]) for name in wall}
        for name in out:
            out[name]["call_s"] = [round(t, 4) for t in call[name]]
            out[name]["call_min_s"] = round(min(call[name]), 4)
            out[name]["call_spread_s"] = round(max(call[name]) - min(call[name]), 4)
            out[name]["handed_to_strict"] = int(sum(r.numerics == "strict" for r in last[name])) if fast else 0
        calls = {name: dict(min_s=out[name]["call_min_s"], spread_s=out[name]["call_spread_s"]) for name in out}
        entry = dict(scale=scale, **out,
                     resident_vs_stateless=beats(out["resident"], out["stateless"]),
                     resident_vs_stateless_call_alone=beats(calls["resident"], calls["stateless"]),
                     identical_bits=bool(same_bits(last["resident"], last["stateless"])),
                     traffic=dict(host_to_device_bytes=traffic[-1][0], device_to_host_bytes=traffic[-1][1],
                                  stage_and_restart_ms=[round(t[2], 3) for t in traffic],
                                  stage_and_restart_min_ms=round(min(t[2] for t in traffic), 3),
                                  matrix_bytes=8 * n_lps * m * ns))
        doc["scales"].append(entry)
        print(json.dumps(dict(lps=n_lps, m=m, n_struct=ns, **entry)), flush=True)
    handle.close()
    return doc


def main_resident(args) -> int:
    given = (args.lps, args.m, args.ns)
    workloads = FAST_WORKLOADS if given == FAST_WORKLOADS[0] else (given,)
    head = [core.CoreLP.from_inequality_form(*core.gen_dense_lp(seed=1_000_000 + i, m=workloads[0][1],
                                                                n_struct=workloads[0][2])) for i in range(64)]
    numerics = core.AUTO if args.fast else core.STRICT
    with core.BatchSolver(head, log_cap=0, numerics=numerics) as warm_up:   # every path, every kernel
        first = warm_up.solve(log=False)
        warm_up.solve(log=False)
    (core.solve_batch_fast if args.fast else core.solve_batch)(head, start=first, log=False)
    doc = dict(tool="tools/batch_reopt_bench.py --resident" + (" --fast" if args.fast else ""), repeats=args.repeats,
               pivots_per_launch=args.ppl or "default",
               workloads=[resident_workload(n, m, ns, args.repeats, args.ppl, args.fast) for n, m, ns in workloads])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


def main_fast(args) -> int:
    given = (args.lps, args.m, args.ns)
    workloads = FAST_WORKLOADS if given == FAST_WORKLOADS[0] else (given,)
    head = [core.CoreLP.from_inequality_form(*core.gen_dense_lp(seed=1_000_000 + i, m=workloads[0][1],
                                                                n_struct=workloads[0][2])) for i in range(64)]
    first = core.solve_batch_fast(head, log=False)   # warm-up: every path, every kernel
    core.solve_batch_fast(head, start=first, log=False)
    core.solve_batch(head, start=first, log=False)
    doc = dict(tool="tools/batch_reopt_bench.py --fast", repeats=args.repeats,
               pivots_per_launch=args.ppl or "default",
               workloads=[fast_workload(n, m, ns, args.repeats, args.ppl) for n, m, ns in workloads])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--fast", action="store_true", help="measure the FAST batch from its last bases (see above)")
    ap.add_argument("--resident", action="store_true",
                    help="measure the batch kept on the device against the stateless warm call (see above)")
    ap.add_argument("--lps", type=int, default=4096)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--ns", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ppl", type=int, default=0, help="pivots per launch (0 = the library's default)")
    ap.add_argument("--out", default=None, help="write the JSON document to this file as well")
    args = ap.parse_args()
    if args.resident:
        return main_resident(args)
    if args.fast:
        return main_fast(args)
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
