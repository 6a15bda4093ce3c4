"""The inverse the batched FAST solver keeps in LDS (csrc/k_batch_fast.hip), written down
again in plain numpy float64, and the input families its tests run on.

The transcription does what build_inverse and the rank-1 update are documented to do, in one thread
and one summation order; it is the reference that sets the bound of tests/inverse_check.py for these
families (10x its own worst residual ratio), not a bit-for-bit target.  The families are functions,
so that tests/test_batch_fast_inverse_host.py (no GPU) and tests/test_gpu_batch_fast_inverse.py run
on the same inputs.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np


# ------------------------------------------------------------------ the transcription
def gather(a, basis, ns: int) -> np.ndarray:
    """B, column c = the column of basis[c]: stored entries only (an explicit -0.0 arrives as +0.0)."""
    a = np.asarray(a, dtype=np.float64)
    basis = np.asarray(basis)
    m = len(basis)
    b = np.zeros((m, m))
    for c, var in enumerate(basis):
        if var < ns:
            col = a[:, var]
            b[:, c] = np.where(col != 0.0, col, 0.0)
        else:
            b[var - ns, c] = 1.0
    return b


def eliminate(b: np.ndarray):
    """Gauss-Jordan in place with partial pivoting on a copy of b: (W before the swaps are undone,
    piv), or None on a zero or non-finite pivot."""
    w = np.array(b, dtype=np.float64)
    m = len(w)
    piv = np.arange(m)
    for k in range(m):
        pr = k + int(np.argmax(np.abs(w[k:, k])))   # first maximum: lowest row on ties
        piv[k] = pr
        if pr != k:
            w[[k, pr]] = w[[pr, k]]
        pivot = w[k, k]
        if not (pivot != 0.0) or not np.isfinite(pivot):
            return None
        colk = w[:, k].copy()
        w[:, k] = 0.0
        w[k, k] = 1.0
        w[k] = w[k] / pivot
        others = np.arange(m) != k
        w[others] = w[others] - colk[others, None] * w[k]   # a product, then a difference: no FMA
    return w, piv


def undo_swaps(w: np.ndarray, piv, last_first: bool = True) -> np.ndarray:
    """The row swaps of the elimination applied to the columns: (P B)^-1 P.  last_first=False is the
    wrong order (a negative control)."""
    w = w.copy()
    order = range(len(piv) - 1, -1, -1) if last_first else range(len(piv))
    for k in order:
        if piv[k] != k:
            w[:, [k, piv[k]]] = w[:, [piv[k], k]]
    return w


def invert(a, basis, ns: int):
    """W = B^-1 as build_inverse builds it, or None where it reports a singular basis."""
    out = eliminate(gather(a, basis, ns))
    return None if out is None else undo_swaps(*out)


def entering_column(a, ns: int, var: int) -> np.ndarray:
    a = np.asarray(a, dtype=np.float64)
    if var < ns:
        return a[:, var]
    e = np.zeros(a.shape[0])
    e[var - ns] = 1.0
    return e


def ftran(w: np.ndarray, col: np.ndarray) -> np.ndarray:
    """dx = W a_q as documented: every row in four interleaved partial sums, j ascending, then
    (s0 + s1) + (s2 + s3).  (For a slack this adds zeros to one entry of W: the column itself.)"""
    m = len(w)
    prod = np.zeros((m, (m + 3) // 4 * 4))
    prod[:, :m] = w * col
    s = np.zeros((m, 4))
    for j in range(0, prod.shape[1], 4):
        s = s + prod[:, j:j + 4]
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def update(w: np.ndarray, dx: np.ndarray, p: int) -> np.ndarray:
    """The product-form update of a pivot at basis position p: row p <- row p / dx_p,
    row i <- row i - dx_i * row p."""
    new = w.copy()
    new[p] = w[p] / dx[p]
    others = np.arange(len(w)) != p
    new[others] = w[others] - dx[others, None] * new[p]
    return new


def follow(a, ns: int, basis, log, stops, refactor_every: int) -> dict:
    """{stop: (W, basis)} as one launch of the kernel leaves them after the first `stop` pivots of
    `log` ((kind, entering, leaving, ...) per pivot), for every stop of `stops` the log reaches and for the log's end if a stop lies beyond it:
    built at step 0, rebuilt whenever refactor_every pivots have run on it -- also right before the
    budget ends the launch -- updated in between."""
    basis = np.array(basis, dtype=np.int64)
    w, since, out = None, 0, {}
    for step in range(min(max(stops), len(log)) + 1):
        if step == 0 or since >= refactor_every:
            w, since = invert(a, basis, ns), 0
            assert w is not None
        if step in stops or step == len(log):
            out[step] = (w.copy(), basis.copy())
        if step == len(log):
            break
        _, entering, leaving = log[step][:3]
        p = int(np.flatnonzero(basis == leaving)[0])
        dx = ftran(w, entering_column(a, ns, entering))
        w = update(w, dx, p)
        basis[p] = entering
        since += 1
    return out


# ------------------------------------------------------------------ the families
@dataclass
class Case:
    name: str
    lp: object              # core.CoreLP
    a: np.ndarray           # the structural block, m x ns
    ns: int
    exact: np.ndarray | None = None   # family 2: B^-1, every entry representable
    opts: dict = field(default_factory=dict)

    @property
    def m(self) -> int:
        return self.a.shape[0]


def scattered_lp(core, m, k, seed):
    """A basis of k structural columns (a random subset) at random positions; the slacks of m - k
    random rows fill the other positions, in random order."""
    ns = 2 * m
    a, _, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    rng = np.random.default_rng(seed)
    cols = rng.choice(ns, k, replace=False)
    pos = rng.choice(m, k, replace=False)
    slack_rows = rng.choice(m, m - k, replace=False)
    basis = np.empty(m, dtype=np.int64)
    basis[pos] = cols
    basis[np.setdiff1d(np.arange(m), pos)] = ns + slack_rows
    nonbasis = np.setdiff1d(np.arange(ns + m), basis).astype(np.int64)
    rng.shuffle(nonbasis)
    a = np.asarray(a)
    lp = core.CoreLP(a=a, c=np.concatenate([c, np.zeros(m)]), basis=basis, nonbasis=nonbasis,
                     x=np.ones(m), z=-np.ones(ns))
    return lp, a, ns


F1_ROWS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)
F1_SEEDS = 3


def family1(core) -> list:
    """Scattered bases: every bucket edge, k = 1, m // 2, m - 1, m structural columns, three seeds."""
    out = []
    for m in F1_ROWS:
        for k in sorted({k for k in (1, m // 2, m - 1, m) if 1 <= k <= m}):
            for s in range(F1_SEEDS):
                lp, a, ns = scattered_lp(core, m, k, seed=61000 + 1000 * s + 7 * m + k)
                out.append(Case(f"scattered m={m} k={k} seed {s}", lp, a, ns))
    return out


F2_ROWS = (16, 17, 32, 33, 128)
_EXTRA = 3  # nonbasic structural columns beside the block


def _planted(core, name, block, exact, seed) -> Case:
    """The m x m block as structural columns 0..m-1, basic in that order; _EXTRA more columns and
    all slacks nonbasic."""
    m = len(block)
    rng = np.random.default_rng(seed)
    a = np.concatenate([block, rng.integers(-2, 3, (m, _EXTRA)).astype(np.float64)], axis=1)
    ns = m + _EXTRA
    lp = core.CoreLP(a=a, c=np.concatenate([rng.integers(-3, 4, ns).astype(np.float64), np.zeros(m)]),
                     basis=np.arange(m, dtype=np.int64), nonbasis=np.arange(m, ns + m, dtype=np.int64),
                     x=np.ones(m), z=-np.ones(ns))
    return Case(name, lp, a, ns, exact=exact)


def family2(core) -> list:
    """Row exchanges with an exactly representable inverse: a permutation matrix times a
    power-of-two diagonal (column c has its one entry 2^e in row perm[c]: the elimination swaps at
    every step that is not yet in place), and a unit lower-bidiagonal block of 0 / +-1."""
    out = []
    for m in F2_ROWS:
        rng = np.random.default_rng(62000 + m)
        perms = {"cyclic shift": (np.arange(m) + 1) % m, "reversal": np.arange(m)[::-1],
                 "random permutation": rng.permutation(m)}
        for what, perm in perms.items():
            scale = 2.0 ** rng.integers(-3, 4, m)
            block, exact = np.zeros((m, m)), np.zeros((m, m))
            block[perm, np.arange(m)] = scale
            exact[np.arange(m), perm] = 1.0 / scale
            out.append(_planted(core, f"{what} m={m}", block, exact, 62100 + m))
        sub = rng.integers(-1, 2, m - 1)
        block = np.eye(m) + np.diag(sub.astype(np.float64), -1)
        exact = np.zeros((m, m), dtype=np.int64)
        for j in range(m):
            exact[j, j] = 1
            for i in range(j + 1, m):
                exact[i, j] = -sub[i - 1] * exact[i - 1, j]
        out.append(_planted(core, f"bidiagonal m={m}", block, exact.astype(np.float64), 62200 + m))
    return out


F3_ROWS = (5, 16, 17, 33, 65, 128)


def family3(core) -> list:
    """Singular bases whose zero pivot is exact: a basic structural column that is all zero, two
    basic structural columns that are equal, and a row of the structural block that is zero while
    its slack is nonbasic."""
    import dataclasses

    out = []
    for m in F3_ROWS:
        seed = 63000 + m
        rng = np.random.default_rng(seed)
        lp, a, ns = scattered_lp(core, m, max(2, m // 2), seed)
        basic = np.sort(lp.basis[lp.basis < ns])
        a0 = a.copy()
        a0[:, basic[-1]] = 0.0
        out.append(Case(f"zero column m={m}", dataclasses.replace(lp, a=a0), a0, ns))
        a1 = rng.integers(-3, 4, a.shape).astype(np.float64)
        a1[:, basic[1]] = a1[:, basic[0]]
        out.append(Case(f"equal columns m={m}", dataclasses.replace(lp, a=a1), a1, ns))
        # a row without a basic slack: its slack is nonbasic already, or leaves for a structural column
        free = np.setdiff1d(np.arange(m), lp.basis[lp.basis >= ns] - ns)
        a2 = a.copy()
        a2[free[0], :] = 0.0
        out.append(Case(f"zero row m={m}", dataclasses.replace(lp, a=a2), a2, ns))
    return out


F4_ROWS = (16, 17, 32, 33, 64, 65, 128)
F4_TIES = ((9600, 1), (9601, 2))          # tests/lp_families.make_lp(seed, kind, 30, 48): slacks re-enter
F4_STOPS_REBUILT = (1, 2, 7, 8, 9, 20, 63)  # with refactor_every = 8
F4_STOPS_PLAIN = (1, 2, 63)                 # with no rebuild inside the launch
F4_REFACTOR = 8


def family4(core) -> list:
    """Starts for runs of pivots: continuous data from the slack basis and from a scattered basis
    (k = m // 2), and integer / 0-1 LPs (near ties counted, so FAST keeps going) where slacks re-enter."""
    import dataclasses

    from tests.lp_families import make_lp

    out = []
    for m in F4_ROWS:
        a, b, c = core.gen_dense_lp(seed=64000 + m, m=m, n_struct=2 * m)
        a = np.array(a)
        out.append(Case(f"slack start m={m}", core.CoreLP.from_inequality_form(a, b, c), a, 2 * m))
        # a state without scattered_lp's exact ties (x = 1, z = -1 makes every first ratio equal,
        # and a flagged LP is not compared with the oracle): distinct values of the same signs
        lp, a, ns = scattered_lp(core, m, m // 2, seed=64500 + m)
        rng = np.random.default_rng(64900 + m)
        lp = dataclasses.replace(lp, x=rng.uniform(0.5, 1.5, m), z=-rng.uniform(0.5, 1.5, ns))
        out.append(Case(f"scattered start m={m}", lp, a, ns))
    for seed, kind in F4_TIES:
        a, b, c = make_lp(seed, kind, 30, 48)
        a = np.asarray(a, dtype=np.float64)
        out.append(Case(f"make_lp({seed}, {kind}) {a.shape[0]}x{a.shape[1]}",
                        core.CoreLP.from_inequality_form(a, b, c), a, a.shape[1]))
    return out


def oracle_run(case: Case, max_iter: int):
    """The CPU oracle's solve of the case from its starting state, at most max_iter pivots."""
    from oracle import oracle as ora

    m, ns = case.a.shape
    col_ptr, row_idx, val = ora.csc_from_dense(np.concatenate([case.a, np.eye(m)], axis=1))
    lp = case.lp
    sf = ora.StdForm(m=m, n=ns + m, col_ptr=col_ptr, row_idx=row_idx, val=val, c=np.asarray(lp.c, dtype=np.float64),
                     constant=0.0, basis=lp.basis, nonbasis=lp.nonbasis, x=lp.x, z=lp.z)
    return ora.simplex_solve(sf, max_iter=max_iter)
