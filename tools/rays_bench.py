"""What unboundedness and infeasibility rays cost (dzg_solver_ray, dzg_batch_solve_rays): JSON lines.

    fast    wall time of Solver.ray() after a FAST solve (refactor_interval = -1 reserves the
            workspace) of an LP built to end UNBOUNDED and one built to end INFEASIBLE, 300 x 520:
            first call (buffers reserved, c uploaded) and the minimum of three further calls
    strict  the same after STRICT solves at 97 x 161
    batch   dzg_batch_solve_rays against dzg_batch_solve on workload (c) of tools/batch_bench.py
            (8 192 LPs of the 0/1 family at 16 x 32, where the pivot rule ends many LPs UNBOUNDED or
            INFEASIBLE), at most 4 096 pivots per LP, alternating, minimum of three each

    python tools/rays_bench.py [--only fast,strict,batch] [--out FILE]

The two LP families are those of tests/rays_helpers.py: feasible and dual feasible random data plus
one column (one row) that nearly cancels another, so that the verdict is found late in the solve.
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
from tools.batch_bench import WORKLOADS, make  # noqa: E402


def _g1(seed, m, ns):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (m, ns)); x0 = rng.uniform(0, 1, ns); y0 = rng.uniform(0, 1, m)
    return rng, a, a @ x0 + rng.uniform(0, 1, m), a.T @ y0 - rng.uniform(0, 1, ns)


def unbounded_lp(seed, m, ns, delta=1e-3, ps=1e-2):
    rng, a, b, c = _g1(seed, m, ns - 1)
    j = int(rng.integers(0, ns - 1)); at = int(rng.integers(0, ns))
    col = -a[:, j] - ps * rng.uniform(0.1, 1, m)
    return np.insert(a, at, col, axis=1), b, np.insert(c, at, -c[j] + delta)


def infeasible_lp(seed, m, ns, delta=1e-3, ps=1e-2):
    rng, a, b, c = _g1(seed, m - 1, ns)
    r = int(rng.integers(0, m - 1)); at = int(rng.integers(0, m))
    row = -a[r] + ps * rng.uniform(0.1, 1, ns)
    return np.insert(a, at, row, axis=0), np.insert(b, at, -b[r] - delta), c


def handle(name: str, family, m: int, ns: int, **opts) -> dict:
    a, b, c = family(0, m, ns)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), **opts) as s:
        t0 = time.perf_counter()
        status = s.run(0)
        solve_s = time.perf_counter() - t0
        r = s.result(log=False)
        out = dict(measurement=name, family=family.__name__, m=m, n_struct=ns, seed=0, status=status,
                   pivots=r.iterations, dense_columns=r.dense_columns, solve_s=round(solve_s, 4))
        if status not in ("unbounded", "infeasible"):
            return out
        calls = []
        for _ in range(4):
            t0 = time.perf_counter()
            ray = s.ray()
            calls.append(time.perf_counter() - t0)
    out.update(ray_first_call_ms=round(calls[0] * 1e3, 3), ray_ms=round(min(calls[1:]) * 1e3, 3),
               ray_over_solve=round(min(calls[1:]) / solve_s, 6), kind=ray.kind, proven=ray.proven,
               value=ray.value, violation=ray.violation)
    return out


def batch() -> dict:
    count, kind, m, ns = WORKLOADS["c"]
    lps = [core.CoreLP.from_inequality_form(*make(3_000_000 + i, kind, m, ns)) for i in range(count)]
    # (a few LPs of this family cycle under the reference's pivot rule: the cap of tools/batch_bench.py)
    kw = dict(log=False, max_iter=4096)
    core.solve_batch(lps[:64], rays=True, **kw)  # warm-up
    plain, with_rays = [], []
    for _ in range(3):
        plain.append(core.solve_batch(lps, **kw)[0].solve_ms)
        res = core.solve_batch(lps, rays=True, **kw)
        with_rays.append(res[0].solve_ms)
    rays = [r.ray for r in res if r.ray is not None]
    p, d = min(plain), min(with_rays)
    return dict(measurement="batch", lps=count, m=m, n_struct=ns, rays=len(rays),
                primal=sum(r.kind == "primal" for r in rays), farkas=sum(r.kind == "farkas" for r in rays),
                proven=sum(r.proven for r in rays), total_pivots=sum(r.iterations for r in res),
                batch_solve_ms=round(p, 2), batch_solve_rays_ms=round(d, 2),
                overhead_pct=round(100.0 * (d - p) / p, 2), all_plain_ms=[round(v, 2) for v in plain],
                all_rays_ms=[round(v, 2) for v in with_rays])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", default="fast,strict,batch")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    fast = dict(numerics=core.FAST, refactor_interval=-1)
    jobs = {"fast": [lambda: handle("fast", unbounded_lp, 300, 520, **fast),
                     lambda: handle("fast", infeasible_lp, 300, 520, **fast)],
            "strict": [lambda: handle("strict", unbounded_lp, 97, 161, numerics=core.STRICT),
                       lambda: handle("strict", infeasible_lp, 97, 161, numerics=core.STRICT)],
            "batch": [batch]}
    for name in args.only.split(","):
        for job in jobs[name]:
            line = json.dumps(job())
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
