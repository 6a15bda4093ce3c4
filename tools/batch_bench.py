"""Throughput of the batched STRICT solver (dzg_batch_solve) on three seeded workloads.

    (a) 4 096 kind-0 LPs at  64 x 128      (tests/lp_families.py: continuous G1 data)
    (b) 1 024 kind-0 LPs at 128 x 256
    (c) 8 192 kind-2 LPs at  16 x 32       (degenerate 0/1 data)

Per workload, one JSON line: the batch's wall time (a host clock around dzg_batch_solve after a
warm-up call, uploads and downloads included), total pivots, LPs/s and pivots/s; sequential
core.solve(numerics=STRICT) on the first 32 LPs, extrapolated to the whole set; the CPU oracle over
the whole set on 16 threads; and whether every batch result equals the oracle's bit for bit
(status, iterations, pivot log with mu, basis, nonbasis, x, xbar, z, zbar, objective).

    python tools/batch_bench.py [--workloads abc] [--no-oracle] [--no-sequential] [--ppl P] [--max-iter N]

--fast compares the STRICT batch with the FAST batch under the AUTO policy (dzg_batch_solve_fast:
FAST that stops at a near tie, those LPs re-solved in STRICT inside the call) instead: both solve
the workload alternately in one process, three times each (--repeats), and the line reports each
side's minimum wall time and its spread (max - min), their ratio, how many LPs AUTO handed to
STRICT, whether every result that stayed FAST with near_ties == 0 has the STRICT result's status
and pivot log, and the 16-thread oracle's rate.

    python tools/batch_bench.py --fast [--workloads abc] [--repeats 3] [--out profiles/batch_fast_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dantzig_amd import core  # noqa: E402
from oracle import oracle as ora  # noqa: E402

WORKLOADS = {"a": (4096, 0, 64, 128), "b": (1024, 0, 128, 256), "c": (8192, 2, 16, 32)}


def make(seed: int, kind: int, m: int, ns: int):
    """tests/lp_families.make_lp's families at a fixed shape."""
    if kind == 0:
        a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
        return np.array(a), b, c
    rng = np.random.default_rng(seed)
    a = (rng.uniform(size=(m, ns)) < 0.3).astype(np.float64)
    return a, rng.integers(0, 4, m).astype(np.float64), rng.integers(-1, 6, ns).astype(np.float64)


def bits_equal(x, y) -> bool:
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return x.shape == y.shape and bool(np.all((x.view(np.int64) == y.view(np.int64))
                                              | ((x == 0) & (y == 0)) | (np.isnan(x) & np.isnan(y))))


def same(g, w) -> bool:
    return (g.status == w.status and g.iterations == w.iterations
            and [p[:3] for p in g.pivots] == [tuple(p[:3]) for p in w.pivots]
            and bits_equal([p[3] for p in g.pivots], [p[3] for p in w.pivots])
            and g.basis.tolist() == w.basis.tolist() and g.nonbasis.tolist() == w.nonbasis.tolist()
            and all(bits_equal(getattr(g, k), getattr(w, k)) for k in ("x", "xbar", "z", "zbar"))
            and bits_equal([g.objective], [w.objective]))


def run(name: str, args) -> dict:
    count, kind, m, ns = WORKLOADS[name]
    data = [make(1_000_000 * (ord(name) - 96) + i, kind, m, ns) for i in range(count)]
    lps = [core.CoreLP.from_inequality_form(a, b, c) for a, b, c in data]
    log_cap = args.log_cap
    kw = dict(log_cap=log_cap, pivots_per_launch=args.ppl, max_iter=args.max_iter)
    core.solve_batch(lps[:64], **kw)  # warm-up
    res = core.solve_batch(lps, **kw)
    wall_s = res[0].solve_ms / 1e3
    pivots = sum(r.iterations for r in res)
    out = dict(workload=name, lps=count, kind=kind, m=m, n_struct=ns,
               pivots_per_launch=args.ppl or "default", batch_wall_s=round(wall_s, 4),
               total_pivots=pivots, lps_per_s=round(count / wall_s, 1),
               pivots_per_s=round(pivots / wall_s, 1),
               statuses={s: sum(r.status == s for r in res) for s in sorted({r.status for r in res})})
    if not args.no_sequential:
        k = min(32, count)
        t0 = time.perf_counter()
        seq = [core.solve(lp, numerics=core.STRICT, max_iter=args.max_iter) for lp in lps[:k]]
        t = time.perf_counter() - t0
        seq_piv = sum(r.iterations for r in seq)
        out.update(sequential_lps=k, sequential_s=round(t, 3),
                   sequential_pivots_per_s=round(seq_piv / t, 1),
                   sequential_extrapolated_s=round(t * count / k, 2),
                   speedup_vs_sequential_pivots=round((pivots / wall_s) / (seq_piv / t), 1))
    if not args.no_oracle:
        def one(abc):
            return ora.simplex_solve(ora.stdform_from_dense(*abc), max_iter=args.max_iter,
                                     log_cap=log_cap)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=16) as ex:  # ctypes releases the GIL
            want = list(ex.map(one, data))
        t = time.perf_counter() - t0
        opiv = sum(w.iterations for w in want)
        mism = [i for i, (g, w) in enumerate(zip(res, want)) if not same(g, w)]
        out.update(oracle_threads=16, oracle_s=round(t, 3), oracle_pivots_per_s=round(opiv / t, 1),
                   speedup_vs_oracle_pivots=round((pivots / wall_s) / (opiv / t), 2),
                   bit_equal_to_oracle=not mism, mismatches=len(mism), first_mismatch=mism[:1])
    return out


def run_fast(name: str, args) -> dict:
    count, kind, m, ns = WORKLOADS[name]
    data = [make(1_000_000 * (ord(name) - 96) + i, kind, m, ns) for i in range(count)]
    lps = [core.CoreLP.from_inequality_form(a, b, c) for a, b, c in data]
    kw = dict(log_cap=args.log_cap, max_iter=args.max_iter)
    fkw = dict(kw, numerics=core.AUTO, pivots_per_launch=args.fast_ppl, refactor_every=args.refactor_every)
    core.solve_batch(lps[:64], pivots_per_launch=args.ppl, **kw)  # warm-up
    core.solve_batch_fast(lps[:64], **fkw)
    strict_s, fast_s = [], []
    for _ in range(args.repeats):
        strict = core.solve_batch(lps, pivots_per_launch=args.ppl, **kw)
        strict_s.append(strict[0].solve_ms / 1e3)
        fast = core.solve_batch_fast(lps, **fkw)
        fast_s.append(fast[0].solve_ms / 1e3)
    pivots = sum(r.iterations for r in strict)
    stayed = [i for i, r in enumerate(fast) if r.numerics == "fast"]
    clean = [i for i in stayed if fast[i].near_ties == 0]
    off = [i for i in clean if fast[i].status != strict[i].status
           or [p[:3] for p in fast[i].pivots] != [p[:3] for p in strict[i].pivots]]
    off += [i for i, r in enumerate(fast) if r.numerics == "strict" and not same(r, strict[i])]
    s_min, f_min = min(strict_s), min(fast_s)
    s_spread, f_spread = max(strict_s) - s_min, max(fast_s) - f_min
    out = dict(workload=name, mode="fast-vs-strict", lps=count, kind=kind, m=m, n_struct=ns, repeats=args.repeats,
               total_pivots=pivots, strict_wall_s=[round(t, 4) for t in strict_s],
               fast_wall_s=[round(t, 4) for t in fast_s], strict_min_s=round(s_min, 4),
               strict_spread_s=round(s_spread, 4), fast_min_s=round(f_min, 4), fast_spread_s=round(f_spread, 4),
               strict_pivots_per_s=round(pivots / s_min, 1), fast_pivots_per_s=round(pivots / f_min, 1),
               fast_over_strict=round(s_min / f_min, 2),
               fast_beats_strict_by_more_than_the_spread=bool(s_min - f_min > max(s_spread, f_spread)),
               resolved_in_strict=count - len(stayed), stayed_fast_clean=len(clean),
               max_refactors=max(r.refactors for r in fast), max_pivot_error=max(r.max_pivot_error for r in fast),
               log_equal_to_strict=not off, mismatches=len(off), first_mismatch=off[:1])
    if not args.no_oracle:
        def one(abc):
            return ora.simplex_solve(ora.stdform_from_dense(*abc), max_iter=args.max_iter, log_cap=args.log_cap)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=16) as ex:  # ctypes releases the GIL
            want = list(ex.map(one, data))
        t = time.perf_counter() - t0
        opiv = sum(w.iterations for w in want)
        out.update(oracle_threads=16, oracle_s=round(t, 3), oracle_pivots_per_s=round(opiv / t, 1),
                   fast_vs_oracle_pivots=round((pivots / f_min) / (opiv / t), 2),
                   strict_vs_oracle_pivots=round((pivots / s_min) / (opiv / t), 2),
                   strict_bit_equal_to_oracle=all(same(g, w) for g, w in zip(strict, want)))
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workloads", default="abc")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--no-sequential", action="store_true")
    ap.add_argument("--ppl", type=int, default=0, help="pivots per launch (0 = the library's default)")
    ap.add_argument("--log-cap", type=int, default=4096)
    ap.add_argument("--max-iter", type=int, default=4096,
                    help="per-LP pivot cap, the same on every side (degenerate 0/1 LPs can cycle: the "
                         "reference's rule has no anti-cycling)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--fast", action="store_true", help="STRICT against FAST/AUTO, alternately (see above)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fast-ppl", type=int, default=0, help="--fast: the FAST batch's pivots per launch")
    ap.add_argument("--refactor-every", type=int, default=0)
    args = ap.parse_args()
    ok = True
    for name in args.workloads:
        line = json.dumps(run_fast(name, args) if args.fast else run(name, args))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        ok = ok and '"bit_equal_to_oracle": false' not in line and '"log_equal_to_strict": false' not in line
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
