"""A cutting-plane loop on a live solver (dzg_solver_extend) against cold solves of the accumulated LP.

The LP is G1 at 2048 x 4096 in FAST numerics.  It is solved once; then, per round, 16 cuts violated at
the current optimum x* (rows uniform in [0, 1), rhs = 0.9 rows . x*: tests/extend_check.py's recipe)
are appended and the solve carries on from the basis it holds.  Per round one JSON line with

    cold_*     a fresh Solver on the accumulated LP (all a caller could do before this entry point):
               pivots, wall time of create + run, and of the run alone
    extend_*   extend() + run() on the live solver: the wall time of the call, its split as
               dzg_debug_extend_ms reports it -- the matrix re-laid on the device (relayout), the
               refactorisation of the extended basis (refactor), the restart state (restart) -- the
               host's own share (building the extended CoreLP: host), then the run and its pivots

and whether the two optima agree (relative difference of the objectives).  It prints and does not
assert; DESIGN.md section 7i holds a table measured with it.

    python tools/extend_bench.py [--m 2048] [--ns 4096] [--seed 7] [--cuts 16] [--rounds 8]
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

    t0 = time.perf_counter()
    s = core.Solver(lp, **OPTS)
    status = s.run(0)
    res = s.result(log=False)
    print(json.dumps(dict(round=0, status=status, pivots=res.iterations, k=res.dense_columns,
                          wall_s=round(time.perf_counter() - t0, 4), run_s=round(res.solve_ms / 1e3, 4))),
          flush=True)
    done, run_ms = res.iterations, res.solve_ms
    for rnd in range(1, args.rounds + 1):
        # the cuts, at the optimum the live solver holds (benchmark numbering: variables 0..ns-1 are
        # the structural columns and stay so, the new slacks are numbered after everything else)
        value = np.zeros(lp.n)
        value[res.basis] = res.x
        rng = np.random.default_rng(rnd)
        rows = rng.random((args.cuts, ns))
        rhs = 0.9 * rows @ value[:ns]
        t0 = time.perf_counter()
        s.extend(rows=rows, rhs=rhs)
        t1 = time.perf_counter()
        warm_status = s.run(0)
        t2 = time.perf_counter()
        lp = s._lp
        res = s.result(log=False)
        relayout, refactor, restart = s.debug_extend_ms()
        t3 = time.perf_counter()
        with core.Solver(lp, **OPTS) as cold:
            cold_status = cold.run(0)
            cr = cold.result(log=False)
        cold_wall = time.perf_counter() - t3
        print(json.dumps(dict(
            round=rnd, rows=lp.m, cold_status=cold_status, cold_pivots=cr.iterations,
            cold_wall_s=round(cold_wall, 4), cold_run_s=round(cr.solve_ms / 1e3, 4),
            extend_status=warm_status, extend_pivots=res.iterations - done,
            extend_call_ms=round(1e3 * (t1 - t0), 2), relayout_ms=round(relayout, 2),
            refactor_ms=round(refactor, 2), restart_ms=round(restart, 2),
            host_ms=round(1e3 * (t1 - t0) - relayout - refactor - restart, 2),
            extend_run_ms=round(res.solve_ms - run_ms, 2), extend_wall_s=round(t2 - t0, 4),
            k=res.dense_columns,
            objective_rel_diff=abs(cr.objective - res.objective) / max(1.0, abs(cr.objective)))), flush=True)
        done, run_ms = res.iterations, res.solve_ms
    s.close()


if __name__ == "__main__":
    main()
