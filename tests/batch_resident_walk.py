"""A host mirror of a live core.BatchSolver and the random walks it is driven through
(tests/test_gpu_batch_resident.py), in the style of tests/handle_walk.py.

`Mirror` holds what the handle holds per LP: the matrix, the current b (by constraint row), c (by
structural column) and constant, and `last`, the result its last solve ended with (None before the
first solve; set_start(i, None) forgets it).  Its operations carry the signatures of BatchSolver's.
solve(which) answers with the stateless call on the same data -- core.solve_batch for STRICT,
core.solve_batch_fast otherwise -- handing over start = the mirror's `last`, through the rule
core._batch_starts applies to a CoreResult (singular and panic count as no start).  Nothing here
computes: the stateless call is the reference, as the feature is defined.

`recipe(seed, count, steps)` draws ragged LPs of at most 33 rows (every bucket edge up to there, odd
sizes, a single row) and a list of operations: update (b, c, both, the constant), set_start(None),
solve(a random subset) and solve().  Changes are reopt_check.moved's, so every LP stays feasible and
bounded and its re-solve pivots a little.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from dantzig_amd import core
from tests import reopt_check as rc

SHAPES = [(1, 3), (2, 3), (5, 9), (7, 4), (15, 6), (16, 24), (17, 24), (24, 40), (31, 8), (32, 12), (33, 40), (33, 5)]


@dataclasses.dataclass
class Op:
    call: str      # update_many | set_start | solve
    kind: str      # what the recipe drew, for the coverage counts
    args: tuple


def full_c(c, m):
    return np.concatenate([np.asarray(c, dtype=np.float64), np.zeros(m)])


class Mirror:
    def __init__(self, data, **opts):
        self.a = [np.ascontiguousarray(a, dtype=np.float64) for a, _, _ in data]
        self.b = [np.array(b, dtype=np.float64) for _, b, _ in data]
        self.c = [np.array(c, dtype=np.float64) for _, _, c in data]
        self.constant = [0.0] * len(data)
        self.last = [None] * len(data)
        self.opts = opts
        self.strict = opts.get("numerics", core.AUTO) == core.STRICT

    def lp(self, i) -> core.CoreLP:
        return core.CoreLP.from_inequality_form(self.a[i], self.b[i], self.c[i], self.constant[i])

    def lps(self):
        return [self.lp(i) for i in range(len(self.a))]

    def update_many(self, changes):
        for i, b, c, constant in changes:
            if b is not None:
                self.b[i] = np.array(b, dtype=np.float64)
            if c is not None:
                self.c[i] = np.array(c, dtype=np.float64)[:self.a[i].shape[1]]
            if constant is not None:
                self.constant[i] = float(constant)

    def set_start(self, i, start):
        self.last[i] = start

    def solve(self, which=None, log=True):
        ids = list(range(len(self.a))) if which is None else list(which)
        lps, start = [self.lp(i) for i in ids], [self.last[i] for i in ids]
        start = start if any(s is not None for s in start) else None
        if self.strict:
            out = core.solve_batch(lps, log=log, start=start, **self.opts)
        else:
            out = core.solve_batch_fast(lps, log=log, start=start, **self.opts)
        for i, r in zip(ids, out):
            self.last[i] = r
        return out


def recipe(seed: int, count: int = 12, steps: int = 30):
    """(data, ops): `count` LPs as (a, b, c) and `steps` operations; the walk ends with a solve()."""
    rng = np.random.default_rng(seed)
    shapes = [SHAPES[k % len(SHAPES)] for k in rng.permutation(count)]
    data = [core.gen_dense_lp(seed=1000 * seed + k, m=m, n_struct=ns) for k, (m, ns) in enumerate(shapes)]
    data = [(np.ascontiguousarray(a), np.array(b), np.array(c)) for a, b, c in data]
    cur = [(b.copy(), c.copy()) for _, b, c in data]
    ops = [Op("solve", "solve all", (None,))]
    kinds = ["b", "c", "both", "constant", "cold", "subset", "subset", "all"]
    for step in range(steps - 2):
        kind = kinds[int(rng.integers(len(kinds)))]
        if kind in ("b", "c", "both", "constant"):
            changes = []
            for i in rng.choice(count, size=int(rng.integers(1, count + 1)), replace=False).tolist():
                m = data[i][0].shape[0]
                b2, c2 = rc.moved(int(rng.integers(1 << 30)), *cur[i], scale=float(rng.choice([1e-3, 1e-1, 1.0])))
                if kind == "constant":
                    changes.append((i, None, None, float(rng.integers(-3, 4))))
                    continue
                cur[i] = (b2 if kind != "c" else cur[i][0], c2 if kind != "b" else cur[i][1])
                changes.append((i, b2 if kind != "c" else None, full_c(c2, m) if kind != "b" else None, None))
            ops.append(Op("update_many", kind, (changes,)))
        elif kind == "cold":
            ops.append(Op("set_start", kind, (int(rng.integers(count)), None)))
        elif kind == "subset":
            which = rng.choice(count, size=int(rng.integers(1, count)), replace=False).tolist()
            ops.append(Op("solve", kind, (which,)))
        else:
            ops.append(Op("solve", "solve all", (None,)))
    ops.append(Op("solve", "solve all", (None,)))
    return data, ops
