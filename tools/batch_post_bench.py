"""Duals and ranges after every re-solve on a resident handle (dzg_batch_resolve_post) against what
there was before for the same answer: the cold STRICT batch with ranging.

The workloads of tools/batch_reopt_bench.py --resident: 4 096 LPs at 64 x 128 and 1 024 LPs at
128 x 256 from gen_dense_lp (or the one --lps / --m / --ns name), (b, c) of every LP moved by
tests/reopt_check.moved at scales 1e-3, 1e-1 and 1.  A handle under AUTO is created and solved cold
once, outside the window; then per scale three sides, alternately, --repeats times each after one
warm-up round, in this one process on one device, every LP from the basis the first solve ended on:

    plain    handle.update_many(changed) + handle.solve()
    post     handle.update_many(changed) + handle.solve(duals=True, ranging=True)
    cold     solve_batch(changed, ranging=True)          STRICT, cold, the matrices uploaded again

ranging=True is every unit direction: n cost and m right-hand-side directions per LP.  Per side: the
C call's times (CoreResult.solve_ms: a host clock around the call, which ends in a device
synchronise), their minimum and spread, total pivots, statuses; for `post` the device time of the
post-solve launches (events around them, dzg_debug_batch_post_ms), the number of LPs with ranges and
of LPs handed to STRICT; and the largest relative difference between a finite range end of `post`
and of `cold` over the LPs that ended optimal on the same basis.  No threshold: the tool reports.

    python tools/batch_post_bench.py [--repeats 5] [--out profiles/batch_post_bench.json]
"""
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
WORKLOADS = ((4096, 64, 128), (1024, 128, 256))


def side(times, results) -> dict:
    lo = min(times)
    return dict(call_s=[round(t, 4) for t in times], min_s=round(lo, 4), spread_s=round(max(times) - lo, 4),
                total_pivots=int(sum(r.iterations for r in results)),
                statuses={s: sum(r.status == s for r in results) for s in sorted({r.status for r in results})})


def range_diff(got, want) -> tuple:
    """(LPs compared, largest relative difference of a finite end) over LPs optimal on the same basis."""
    worst, count = 0.0, 0
    for g, w in zip(got, want):
        if g.ranging is None or w.ranging is None or g.basis.tolist() != w.basis.tolist() \
                or g.nonbasis.tolist() != w.nonbasis.tolist():
            continue
        count += 1
        for f in ("cost_lo", "cost_hi", "rhs_lo", "rhs_hi"):
            a, b = getattr(g.ranging, f), getattr(w.ranging, f)
            fin = np.isfinite(a) & np.isfinite(b)
            if fin.any():
                worst = max(worst, float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin])))))
    return count, worst


def workload(n_lps: int, m: int, ns: int, repeats: int) -> dict:
    data = [core.gen_dense_lp(seed=1_000_000 + i, m=m, n_struct=ns) for i in range(n_lps)]
    data = [(np.array(a), np.array(b), np.array(c)) for a, b, c in data]
    lps = [core.CoreLP.from_inequality_form(a, b, c) for a, b, c in data]
    zeros = np.zeros(m)
    back = [(i, b, np.concatenate([c, zeros]), None) for i, (_, b, c) in enumerate(data)]
    handle = core.BatchSolver(lps, log_cap=0, numerics=core.AUTO)
    previous = handle.solve(log=False)
    doc = dict(lps=n_lps, m=m, n_struct=ns, numerics="auto", directions_per_lp=m + ns + m, scales=[])
    for scale in SCALES:
        changed, changes = [], []
        for i, (a, b, c) in enumerate(data):
            b2, c2 = moved(i, b, c, scale=scale)
            changed.append(core.CoreLP.from_inequality_form(a, b2, c2))
            changes.append((i, b2, np.concatenate([c2, zeros]), None))
        times = dict(plain=[], post=[], cold=[])
        last, post_ms = {}, []
        for rep in range(repeats + 1):   # round 0 is the warm-up
            for name in ("plain", "post"):
                for i, r in enumerate(previous):
                    handle.set_start(i, r)
                handle.update_many(changes)
                last[name] = handle.solve(log=False, **(dict(duals=True, ranging=True) if name == "post" else {}))
                if name == "post" and rep:
                    post_ms.append(float(_ffi.lib().dzg_debug_batch_post_ms()))
                handle.update_many(back)
            last["cold"] = core.solve_batch(changed, log=False, ranging=True)
            if rep:
                for name in times:
                    times[name].append(last[name][0].solve_ms / 1e3)
        out = {name: side(times[name], last[name]) for name in times}
        compared, diff = range_diff(last["post"], last["cold"])
        entry = dict(scale=scale, **out,
                     post_launches_ms=[round(t, 3) for t in post_ms], post_launches_min_ms=round(min(post_ms), 3),
                     post_minus_plain_min_s=round(out["post"]["min_s"] - out["plain"]["min_s"], 4),
                     cold_over_post=round(out["cold"]["min_s"] / out["post"]["min_s"], 2),
                     lps_with_ranges=int(sum(r.ranging is not None for r in last["post"])),
                     handed_to_strict=int(sum(r.numerics == "strict" for r in last["post"])),
                     same_basis_as_cold=compared, max_rel_range_diff=diff)
        doc["scales"].append(entry)
        print(json.dumps(dict(lps=n_lps, m=m, n_struct=ns, **entry)), flush=True)
    handle.close()
    return doc


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lps", type=int, default=0)
    ap.add_argument("--m", type=int, default=0)
    ap.add_argument("--ns", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the JSON document to this file as well")
    args = ap.parse_args()
    _ffi.require_gpu()
    loads = ((args.lps, args.m, args.ns),) if args.lps and args.m and args.ns else WORKLOADS
    doc = dict(tool="tools/batch_post_bench.py", repeats=args.repeats,
               workloads=[workload(n, m, ns, args.repeats) for n, m, ns in loads])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
