"""Re-optimisation from the optimal basis (dzg_solver_reoptimize) against a cold solve of the changed LP.

The LP is G1 at 2048 x 4096 in FAST numerics.  It is solved once; then, for b' = b + d on 1 %, 10 % and
100 % of the rows and for c' = c - e on 1 %, 10 % and 100 % of the columns (d, e uniform in [0, 1): the
LP stays feasible and bounded), per change one JSON line with

    cold_*    a fresh Solver on the changed LP (all a caller could do before this entry point):
              pivots, wall time of create + run, and of the run alone
    reopt_*   reoptimize() + run() on the solver that holds the optimal basis of the previous LP of
              the sweep: new pivots, wall time of the two together, the reoptimize call split out

and whether the two optima agree (relative difference of the objectives).  It prints and does not
assert; DESIGN.md section 7h holds a table measured with it.

    python tools/reopt_bench.py [--m 2048] [--ns 4096] [--seed 7]
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
    args = ap.parse_args()
    m, ns = args.m, args.ns
    a, b, c = core.gen_dense_lp(seed=args.seed, m=m, n_struct=ns)
    rng = np.random.default_rng(args.seed)
    zeros = np.zeros(m)

    t0 = time.perf_counter()
    s = core.Solver(core.CoreLP.from_inequality_form(a, b, c), **OPTS)
    status = s.run(0)
    first = s.result(log=False)
    print(json.dumps(dict(change="none", status=status, pivots=first.iterations, k=first.dense_columns,
                          wall_s=round(time.perf_counter() - t0, 4), run_s=round(first.solve_ms / 1e3, 4))),
          flush=True)
    done = first.iterations
    for what, size in (("b", m), ("c", ns)):
        for frac in (0.01, 0.1, 1.0):
            idx = rng.choice(size, size=max(1, int(round(frac * size))), replace=False)
            b2, c2 = b.copy(), c.copy()
            (b2 if what == "b" else c2)[idx] += (1.0 if what == "b" else -1.0) * rng.random(len(idx))
            t0 = time.perf_counter()
            with core.Solver(core.CoreLP.from_inequality_form(a, b2, c2), **OPTS) as cold:
                cold_status = cold.run(0)
                cr = cold.result(log=False)
            cold_wall = time.perf_counter() - t0
            t0 = time.perf_counter()
            s.reoptimize(b=b2, c=np.concatenate([c2, zeros]))
            t1 = time.perf_counter()
            warm_status = s.run(0)
            t2 = time.perf_counter()
            wr = s.result(log=False)
            print(json.dumps(dict(
                change=f"{what} on {frac:.0%}", cold_status=cold_status, cold_pivots=cr.iterations,
                cold_wall_s=round(cold_wall, 4), cold_run_s=round(cr.solve_ms / 1e3, 4),
                reopt_status=warm_status, reopt_pivots=wr.iterations - done, reopt_wall_s=round(t2 - t0, 4),
                reopt_call_s=round(t1 - t0, 4), reopt_run_s=round(t2 - t1, 4), k=wr.dense_columns,
                objective_rel_diff=abs(cr.objective - wr.objective) / max(1.0, abs(cr.objective)))), flush=True)
            done = wr.iterations
    s.close()


if __name__ == "__main__":
    main()
