"""The restart state of a warm LP of the FAST batch (csrc/k_batch_fast.hip, k_batch_fast_restart,
DESIGN 7l), written down again in plain numpy float64 on tests/batch_fast_reference.py's invert and
ftran, in the summation orders the kernel documents:

    W   = invert(B)                                    Gauss-Jordan, partial pivoting, swaps undone
    x_i = sum_j W[i][j] rhs[j]                         four interleaved partial sums, j ascending,
    y_r = sum_p W[p][r] c[basis[p]]                    (s0 + s1) + (s2 + s3): ftran's order, both
    z_k = -dz_k - c[N_k]                               dz_k = -y[row] for a slack; for a structural
                                                       column PL lanes sum their rows (stored entries
                                                       only, ascending), then an xor tree
    xbar = zbar = 1                                    PL = 16 / 32 / 64 for m <= 16 / <= 32 / above

It sets the bound of the GPU test (C_FAST_RESTART, 10 x its own worst D against the long-double
state: tests/state_check.py's rule) and is not a bit-for-bit target, as in DESIGN 7g.  all_cases()
puts the warm cases of tests/test_batch_from_host.py into one shape for the host and the GPU test.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from tests import batch_fast_reference as fr
from tests import state_check as sc

# Worst D of the transcribed restart over all_cases() against state_check.exact_state
# (tests/test_batch_fast_from_host.py prints and re-checks it), and the bound the GPU's restart state
# is held to: ten times that.
C_FAST_RESTART_OBSERVED = {"ragged": 6.705e-15, "mixed 24x40": 8.097e-15, "chunk 257 x 65x8": 4.760e-15,
                           "edges": 2.386e-15}
C_FAST_RESTART = 10 * max(C_FAST_RESTART_OBSERVED.values())


def lanes(m: int) -> int:
    """PL of the bucket an m-row LP runs in."""
    return 16 if m <= 16 else 32 if m <= 32 else 64


def inverse(a, codes_b):
    """W = B^-1 for the basis whose column codes are codes_b, or None where build_inverse reports a
    singular basis.  batch_fast_reference.invert's gather, with the codes a var_col may give."""
    a = np.asarray(a, dtype=np.float64)
    b = sc.columns(a, a.shape[0], codes_b)
    out = fr.eliminate(np.where(b != 0.0, b, 0.0))
    return None if out is None else fr.undo_swaps(*out)


def price(a, codes_n, y) -> np.ndarray:
    """dz = -N^T y as k_batch_fast's price() sums it."""
    a = np.asarray(a, dtype=np.float64)
    m = a.shape[0]
    pl = lanes(m)
    dz = np.empty(len(codes_n))
    for k, code in enumerate(codes_n):
        if code < 0:
            dz[k] = -y[-1 - code]
            continue
        col = a[:, code]
        acc = np.zeros(pl)
        for sub in range(min(pl, m)):
            s = 0.0
            for r in range(sub, m, pl):
                if col[r] != 0.0:
                    s = s + col[r] * -y[r]
            acc[sub] = s
        off = pl // 2
        while off > 0:
            acc = acc + acc[np.arange(pl) ^ off]
            off >>= 1
        dz[k] = acc[0]
    return dz


@dataclass
class FastRestart:
    x: np.ndarray
    z: np.ndarray
    singular: bool

    @property
    def state(self):
        return SimpleNamespace(x=self.x, z=self.z, xbar=np.ones(len(self.x)), zbar=np.ones(len(self.z)))


def restart(a, var_col, b2, c2, basis, nonbasis) -> FastRestart:
    """a: (m, ns); var_col: n codes or None (benchmark convention); b2: m, by row; c2: n, by variable."""
    a = np.asarray(a, dtype=np.float64)
    m, ns = a.shape
    basis, nonbasis = np.asarray(basis, dtype=np.int64), np.asarray(nonbasis, dtype=np.int64)
    c2 = np.asarray(c2, dtype=np.float64)
    codes = sc.var_codes(len(basis) + len(nonbasis), ns, var_col)
    with np.errstate(all="ignore"):
        w = inverse(a, codes[basis]) if var_col is not None else fr.invert(a, basis, ns)
        if w is None:
            return FastRestart(np.asarray(b2, dtype=np.float64).copy(), np.zeros(len(nonbasis)), True)
        x = fr.ftran(w, np.asarray(b2, dtype=np.float64))
        y = fr.ftran(np.ascontiguousarray(w.T), c2[basis])
        z = -price(a, codes[nonbasis], y) - c2[nonbasis]
    return FastRestart(x, z, bool(not np.isfinite(x).all() or not np.isfinite(z).all()))


@dataclass
class Warm:
    """One warm LP: the changed data, the start basis, the slack start of the changed LP (what
    state_check.exact_state defines the state by) and the STRICT reference (restart, continuation)."""
    name: str
    a: np.ndarray
    var_col: np.ndarray | None
    b2: np.ndarray        # by constraint row
    c2: np.ndarray        # by variable, all n
    constant: float
    basis: np.ndarray
    nonbasis: np.ndarray
    slack: dict
    ref: object
    want: object
    lp: object            # core.CoreLP of the changed data in slack-basis form

    @property
    def ns(self) -> int:
        return self.a.shape[1]

    def exact(self, basis=None, nonbasis=None):
        return sc.exact_state(self.a, self.ns, self.slack, self.basis if basis is None else basis,
                              self.nonbasis if nonbasis is None else nonbasis, self.var_col)

    def continuation(self, state):
        """The CPU oracle from `state` (x, z; xbar = zbar = 1) at the start basis."""
        from oracle import oracle as ora

        full = SimpleNamespace(basis=self.basis, nonbasis=self.nonbasis, x=state.x, z=state.z)
        sf = sc.stdform(self.a, self.ns, self.c2, full, self.var_col)
        sf.constant = float(self.constant)
        return ora.simplex_solve(sf, xbar=np.ones(len(self.basis)), zbar=np.ones(len(self.nonbasis)))


def _dense(name, a, b2, c2, basis, nonbasis, ref, want) -> Warm:
    from dantzig_amd import core
    from tests import batch_from_reference as bfr
    from tests import reopt_check as rc

    m = a.shape[0]
    return Warm(name, a, None, np.asarray(b2, dtype=np.float64), bfr.full_c(c2, m), 0.0,
                np.asarray(basis, dtype=np.int64), np.asarray(nonbasis, dtype=np.int64),
                rc.slack_start(a, b2, c2), ref, want, core.CoreLP.from_inequality_form(a, b2, c2))


def of_case(w, name=None) -> Warm:
    """A batch_from_reference.WarmCase."""
    return _dense(name or f"{w.a.shape[0]}x{w.a.shape[1]}", w.a, w.b2, w.c2, w.first.basis, w.ref.sf.nonbasis,
                  w.ref, w.want)


def edge_cases() -> list:
    """The four edge starts of tests/test_gpu_batch_from.py, in its order: all-slack, all-structural
    (planted 12x20), the KAT with the builder's var_col, nonbasis handed over reversed."""
    from dantzig_amd import core
    from tests import test_batch_from_host as h

    a, b2, c2, ref, want = h.slack_start_case()
    m, ns = a.shape
    out = [_dense("all-slack start", a, b2, c2, np.arange(ns, ns + m), np.arange(ns), ref, want)]
    p, b2, c2, ref, want = h.planted_case()
    out.append(_dense("all-structural start", p.a, b2, c2, p.basis, p.nonbasis, ref, want))
    f, x2, c2, first, ref, want = h.kat_case()
    rhs = np.empty(f.m)
    rhs[-1 - f.var_col[f.basis]] = x2
    slack = dict(basis=f.basis, nonbasis=f.nonbasis, x=x2, xbar=None, z=-c2[f.nonbasis], zbar=None)
    lp = core.CoreLP(a=f.a, c=c2, basis=f.basis, nonbasis=f.nonbasis, x=x2, z=f.z, var_col=f.var_col,
                     constant=f.constant)
    out.append(Warm("KAT non_standard_variables", np.asarray(f.a, dtype=np.float64), np.asarray(f.var_col), rhs,
                    np.asarray(c2, dtype=np.float64), float(f.constant), first.basis, first.nonbasis, slack, ref,
                    want, lp))
    out.append(of_case(h.permuted_case(), "permuted nonbasis"))
    return out


def all_cases() -> dict:
    """{family: [Warm]} over every warm case of tests/test_batch_from_host.py."""
    from tests import test_batch_from_host as h

    return {"ragged": [of_case(w) for w in h.ragged_cases()],
            "mixed 24x40": [of_case(w) for w in h.mixed_cases()],
            "chunk 257 x 65x8": [of_case(w) for w in h.chunk_cases()],
            "edges": edge_cases()}
