"""What sensitivity ranging costs on a FAST handle (dzg_solver_ranging): one JSON line.

After a FAST solve of the 1024 x 2048 config-2 LP of tools/duals_bench.py (generator G1, seed 1002,
refactor_interval = -1): the wall time of Solver.ranging() for the cost directions of all k basic
structurals and the right-hand-side directions of all m rows (first call and the minimum of three
further calls), of the two kinds by themselves, and of Solver.duals() on the same handle -- every
ranging() call contains one duals() call, and D single passes in the style of duals() would cost D
of them.

k_range_cost_mfma by itself needs a kernel trace: run

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ranging_bench.py --out ''

and then `python tools/ranging_bench.py --stats DIR/.../*kernel_stats.csv`, which adds the kernel's
time per ranging() call (the trace's total over the kernel's launches, divided by the eight
ranging() calls of a run that carry cost directions), its achieved TFLOP/s (useful flops
2 D m q_dense, against the 46.9 TFLOP/s that tools/mfma_f64_peak.hip measured) and bytes/s (every
launch reads the dense nonbasic columns once, its Y and G_N -- the algorithmic bytes, not counted
traffic; against the 8 TB/s HBM roofline) to the line.

    python tools/ranging_bench.py [--stats CSV] [--out FILE]     (default: profiles/ranging_bench.jsonl)
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dantzig_amd import core  # noqa: E402

MFMA_F64_PEAK_TFLOPS = 46.9
HBM_PEAK_TBS = 8.0
CHUNK = 256  # DZG_RANGE_CHUNK: directions per launch


def _best(call, repeats=4):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return out, times[0] * 1e3, min(times[1:]) * 1e3


COST_CALLS = 8  # ranging() calls of one run that carry the cost directions: 4 with both kinds, 4 cost only


def kernel_numbers(path: str, m: int, q: int, q_dense: int, dirs: int) -> dict:
    """k_range_cost_mfma's row of a rocprofv3 kernel_stats CSV (of a run of this tool) as time,
    TFLOP/s and bytes/s per ranging() call."""
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "k_range_cost_mfma" in r["Name"]]
    if not rows:
        return {}
    calls, total_ns = int(rows[0]["Calls"]), float(rows[0]["TotalDurationNs"])
    launches = (dirs + CHUNK - 1) // CHUNK
    if calls != COST_CALLS * launches:
        raise SystemExit(f"{path}: {calls} launches of k_range_cost_mfma, expected {COST_CALLS * launches}")
    per_set_ns = total_ns / COST_CALLS  # the launches of one ranging() call, the short last one included
    flops = 2.0 * dirs * m * q_dense
    ldy = (m + 63) // 64 * 64
    bytes_ = 8.0 * (launches * m * q_dense + dirs * ldy + dirs * q)
    return dict(mfma_launches_per_call=launches, mfma_us_per_call=round(per_set_ns / 1e3, 2),
                mfma_tflops=round(flops / per_set_ns / 1e3, 3),
                mfma_fraction_of_peak=round(flops / per_set_ns / 1e3 / MFMA_F64_PEAK_TFLOPS, 4),
                mfma_algorithmic_tb_per_s=round(bytes_ / per_set_ns / 1e3, 3),
                mfma_fraction_of_hbm=round(bytes_ / per_set_ns / 1e3 / HBM_PEAK_TBS, 4))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats CSV of an earlier run of this tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranging_bench.jsonl"),
                    help="the JSON line is appended to this file ('' : print only)")
    args = ap.parse_args()
    m, ns, seed = 1024, 2048, 1002
    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), numerics=core.FAST, refactor_interval=-1) as s:
        t0 = time.perf_counter()
        status = s.run(0)
        solve_s = time.perf_counter() - t0
        r = s.result(log=False)
        cost = [{int(j): 1.0} for j in r.basis if j < ns]
        rhs = [{i: 1.0} for i in range(m)]
        _, duals_first, duals_ms = _best(s.duals)
        rg, both_first, both_ms = _best(lambda: s.ranging(cost, rhs))
        _, _, cost_ms = _best(lambda: s.ranging(cost, []))
        _, _, rhs_ms = _best(lambda: s.ranging([], rhs))
    dirs = len(cost) + len(rhs)
    q_dense = int((r.nonbasis < ns).sum())
    line = dict(measurement="fast_ranging", m=m, n_struct=ns, seed=seed, status=status, pivots=r.iterations,
                dense_columns=r.dense_columns, solve_s=round(solve_s, 4), cost_directions=len(cost),
                rhs_directions=len(rhs), duals_ms=round(duals_ms, 3),
                ranging_first_call_ms=round(both_first, 3), ranging_ms=round(both_ms, 3),
                ranging_cost_only_ms=round(cost_ms, 3), ranging_rhs_only_ms=round(rhs_ms, 3),
                ranging_less_its_duals_ms=round(both_ms - duals_ms, 3),
                single_passes_ms=round(dirs * duals_ms, 1),
                single_passes_over_ranging=round(dirs * duals_ms / both_ms, 1),
                finite_cost_ends=int((rg.cost_lo > -float("inf")).sum() + (rg.cost_hi < float("inf")).sum()),
                finite_rhs_ends=int((rg.rhs_lo > -float("inf")).sum() + (rg.rhs_hi < float("inf")).sum()))
    if args.stats:
        line.update(kernel_numbers(args.stats, m, len(r.nonbasis), q_dense, len(cost)))
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
