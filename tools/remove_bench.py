"""The cutting-plane loop of tools/extend_bench.py with a purge of slack cuts (dzg_solver_remove).

The LP is G1 at 2048 x 4096 in FAST numerics.  Two live solvers run the same loop side by side: per
round 16 cuts violated at the current optimum x* (rows uniform in [0, 1), rhs = 0.9 rows . x*) are
appended with extend() and the solve carries on.  The first handle only grows, which is all a handle
could do before this entry point (tools/extend_bench.py's loop).  The second one drops, after every
round, each cut added so far whose slack is basic at the optimum (removable()), with remove(), and
runs again -- which must take no pivot.  Per round one JSON line with

    grow_*    the handle that only grows: rows held, new pivots, extend call + run (wall)
    purge_*   the handle that purges: rows held after the purge, cuts purged, new pivots, the wall
              time of the extend call, of the run, of the remove call (host clock, removable()
              included; its device side split as dzg_debug_extend_ms reports it: the successor with
              its gathered matrix, the refactorisation, the restart state) and of the run after it,
              and their sum

and the relative difference of the two objectives.  It prints and does not assert; DESIGN.md section
7j holds a table measured with it.

    python tools/remove_bench.py [--m 2048] [--ns 4096] [--seed 7] [--cuts 16] [--rounds 8]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dantzig_amd import core  # noqa: E402

OPTS = dict(numerics=core.FAST, refactor_interval=-1)


def _cuts(s, res, ns: int, count: int, rnd: int):
    """`count` cuts violated at the optimum `res` of the LP `s` holds (structural column j is variable
    j throughout: removals only ever take slacks here)."""
    value = np.zeros(s._lp.n)
    value[res.basis] = res.x
    rows = np.random.default_rng(rnd).random((count, ns))
    return rows, 0.9 * rows @ value[:ns]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--m", type=int, default=2048)
    ap.add_argument("--ns", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--cuts", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=8)
    args = ap.parse_args()
    m, ns = args.m, args.ns
    a, b, c = core.gen_dense_lp(seed=args.seed, m=m, n_struct=ns)
    lp = core.CoreLP.from_inequality_form(a, b, c)

    handles = []
    for name in ("grow", "purge"):
        t0 = time.perf_counter()
        s = core.Solver(lp, **OPTS)
        status = s.run(0)
        res = s.result(log=False)
        print(json.dumps(dict(round=0, handle=name, status=status, rows=m, pivots=res.iterations,
                              k=res.dense_columns, wall_s=round(time.perf_counter() - t0, 4))), flush=True)
        handles.append([s, res])
    for rnd in range(1, args.rounds + 1):
        line = dict(round=rnd)
        # both handles get the cuts drawn at the growing handle's x* (the purged cuts are slack there:
        # the two LPs have the same optimum, and the objectives differ by rounding alone)
        rows, rhs = _cuts(handles[0][0], handles[0][1], ns, args.cuts, rnd)
        for name, h in zip(("grow", "purge"), handles):
            s, res = h
            done = res.iterations
            t0 = time.perf_counter()
            s.extend(rows=rows, rhs=rhs)
            t1 = time.perf_counter()
            status = s.run(0)
            t2 = time.perf_counter()
            res = s.result(log=False)
            line.update({f"{name}_status": status, f"{name}_pivots": res.iterations - done,
                         f"{name}_extend_call_ms": round(1e3 * (t1 - t0), 2),
                         f"{name}_run_ms": round(1e3 * (t2 - t1), 2)})
            total = t2 - t0
            if name == "purge":
                t3 = time.perf_counter()
                slack = np.flatnonzero(s.removable()[0][m:]) + m
                if len(slack):
                    s.remove(rows=slack)
                t4 = time.perf_counter()
                gather, refactor, restart = s.debug_extend_ms() if len(slack) else (0.0, 0.0, 0.0)
                status = s.run(0)
                t5 = time.perf_counter()
                after = s.result(log=False)
                line.update(purged=int(len(slack)), purge_remove_call_ms=round(1e3 * (t4 - t3), 2),
                            purge_gather_ms=round(gather, 2), purge_refactor_ms=round(refactor, 2),
                            purge_restart_ms=round(restart, 2),
                            purge_rerun_ms=round(1e3 * (t5 - t4), 2), purge_rerun_status=status,
                            purge_rerun_pivots=after.iterations - res.iterations, purge_k=after.dense_columns)
                total += t5 - t3
                res = after
            line.update({f"{name}_rows": s.dims()[0], f"{name}_wall_s": round(total, 4)})
            h[1] = res
        grow, purge = handles[0][1].objective, handles[1][1].objective
        line["objective_rel_diff"] = abs(grow - purge) / max(1.0, abs(grow))
        print(json.dumps(line), flush=True)
    for s, _ in handles:
        s.close()


if __name__ == "__main__":
    main()
