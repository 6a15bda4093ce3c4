"""What dual values and reduced costs cost (dzg_solver_duals, dzg_batch_solve_duals): three JSON lines.

    fast    wall time of Solver.duals() after a FAST solve of the 1024 x 2048 config-2 LP
            (generator G1, seed 1002; refactor_interval = -1 reserves the workspace): first call
            (buffers reserved, c uploaded) and the minimum of three further calls
    strict  the same after a STRICT solve of a 128 x 256 G1 LP
    batch   dzg_batch_solve_duals against dzg_batch_solve on workload (a) of tools/batch_bench.py
            (4 096 LPs at 64 x 128), alternating, minimum of three each

    python tools/duals_bench.py [--only fast,strict,batch] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dantzig_amd import core  # noqa: E402
from tools.batch_bench import WORKLOADS, make  # noqa: E402


def handle(name: str, m: int, ns: int, seed: int, **opts) -> dict:
    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), **opts) as s:
        t0 = time.perf_counter()
        status = s.run(0)
        solve_s = time.perf_counter() - t0
        r = s.result(log=False)
        calls = []
        for _ in range(4):
            t0 = time.perf_counter()
            du = s.duals()
            calls.append(time.perf_counter() - t0)
    return dict(measurement=name, m=m, n_struct=ns, seed=seed, status=status, pivots=r.iterations,
                dense_columns=r.dense_columns, solve_s=round(solve_s, 4),
                duals_first_call_ms=round(calls[0] * 1e3, 3), duals_ms=round(min(calls[1:]) * 1e3, 3),
                duals_over_solve=round(min(calls[1:]) / solve_s, 6), source=du.source,
                gap=abs(du.primal_obj - du.dual_obj), z_diff=du.z_diff,
                primal_infeas=du.primal_infeas, dual_infeas=du.dual_infeas)


def batch() -> dict:
    count, kind, m, ns = WORKLOADS["a"]
    lps = [core.CoreLP.from_inequality_form(*make(1_000_000 + i, kind, m, ns)) for i in range(count)]
    core.solve_batch(lps[:64], log=False, duals=True)  # warm-up
    plain, with_duals = [], []
    for _ in range(3):
        plain.append(core.solve_batch(lps, log=False)[0].solve_ms)
        res = core.solve_batch(lps, log=False, duals=True)
        with_duals.append(res[0].solve_ms)
    optimal = sum(r.duals is not None for r in res)
    p, d = min(plain), min(with_duals)
    return dict(measurement="batch", lps=count, m=m, n_struct=ns, optimal=optimal,
                total_pivots=sum(r.iterations for r in res), batch_solve_ms=round(p, 2),
                batch_solve_duals_ms=round(d, 2), overhead_pct=round(100.0 * (d - p) / p, 2),
                all_plain_ms=[round(v, 2) for v in plain], all_duals_ms=[round(v, 2) for v in with_duals],
                largest_gap=max(abs(r.duals.primal_obj - r.duals.dual_obj) for r in res if r.duals))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", default="fast,strict,batch")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    jobs = {"fast": lambda: handle("fast", 1024, 2048, 1002, numerics=core.FAST, refactor_interval=-1),
            "strict": lambda: handle("strict", 128, 256, 1004, numerics=core.STRICT),
            "batch": batch}
    for name in args.only.split(","):
        line = json.dumps(jobs[name]())
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
