"""The CPU restatement of dzg_batch_solve_from (csrc/k_batch_restart.hip) for one LP: the restart
state its start basis defines for the changed data, and the oracle's continuation from it.  The
route is tests/test_gpu_reopt.py's _strict_restart_and_continuation, without a GPU:

    x = oracle.lu_solve(B, b')                       b' by constraint row
    z = duals_reference.core_duals(...).d[nonbasis]  LU::solve of B^T y = c_B, then neg_t_dot
    the continuation = oracle.simplex_solve from (basis, nonbasis, x, z, xbar = zbar = 1)

and the batch's workloads: the LPs the GPU tests and the host tests both use, by seed."""
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from oracle import oracle as ora
from tests import duals_reference as dref
from tests import reopt_check as rc
from tests import state_check as sc


@dataclass
class Restart:
    sf: "ora.StdForm"    # the changed LP in the restart state (basis, nonbasis, x, z)
    x: np.ndarray
    z: np.ndarray
    singular: bool       # a zero pivot in the LU of B or of B^T, or a non-finite entry of x or z


def zero_pivot(mat) -> bool:
    """Matrix::factorize leaves a zero pivot where it met it: any exact zero on the packed diagonal,
    the last entry included."""
    lu, _ = ora.lu_factorize(np.ascontiguousarray(mat))
    return bool((np.diag(lu) == 0.0).any())


def restart(a, var_col, b2, c2, basis, nonbasis, constant=0.0) -> Restart:
    """a: (m, ns); var_col: n codes or None (benchmark convention); b2: m, by row; c2: n, by variable."""
    a = np.asarray(a, dtype=np.float64)
    m, ns = a.shape
    basis, nonbasis = np.asarray(basis, dtype=np.int64), np.asarray(nonbasis, dtype=np.int64)
    n = len(basis) + len(nonbasis)
    codes = sc.var_codes(n, ns, var_col)
    bmat = sc.columns(a, m, codes[basis])
    with np.errstate(all="ignore"):
        x = ora.lu_solve(bmat, np.asarray(b2, dtype=np.float64))
        state = SimpleNamespace(basis=basis, nonbasis=nonbasis, x=x, z=np.zeros(len(nonbasis)))
        sf = sc.stdform(a, ns, c2, state, var_col)
        sf.constant = float(constant)
        z = dref.core_duals(sf, state).d[nonbasis]
    sf.z = z.copy()
    singular = (zero_pivot(bmat) or zero_pivot(bmat.T) or not np.isfinite(x).all() or not np.isfinite(z).all())
    return Restart(sf=sf, x=x, z=z, singular=bool(singular))


def continuation(r: Restart, max_iter: int = 1_000_000):
    """The oracle from the restart state: a SolveResult whose iterations and pivots count from 0."""
    return ora.simplex_solve(r.sf, max_iter=max_iter, xbar=np.ones(r.sf.m), zbar=np.ones(r.sf.n - r.sf.m))


def full_c(c, m):
    return np.concatenate([np.asarray(c, dtype=np.float64), np.zeros(m)])


def cold(a, b, c):
    """The oracle's cold solve of max c.x, A x <= b from the slack basis."""
    return ora.simplex_solve(ora.stdform_from_dense(a, b, c))


@dataclass
class WarmCase:
    """One LP of a warm batch: the data it was solved with first, the changed data, the oracle's cold
    result on the first data (the start basis) and the reference for the warm call."""
    a: np.ndarray
    b: np.ndarray
    c: np.ndarray
    b2: np.ndarray
    c2: np.ndarray
    first: "ora.SolveResult"
    ref: Restart
    want: "ora.SolveResult"


def warm_case(a, b, c, move_seed, scale=1.0, nonbasis_order=None) -> WarmCase:
    """Solve (a, b, c) cold with the oracle, move (b, c) with reopt_check.moved, restate the warm call.
    nonbasis_order: a permutation applied to the start's nonbasis before it is handed over."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    m = a.shape[0]
    first = cold(a, b, c)
    b2, c2 = rc.moved(move_seed, b, c, scale=scale)
    nonbasis = first.nonbasis if nonbasis_order is None else first.nonbasis[np.asarray(nonbasis_order)]
    ref = restart(a, None, b2, full_c(c2, m), first.basis, nonbasis)
    return WarmCase(a=a, b=np.asarray(b, dtype=np.float64), c=np.asarray(c, dtype=np.float64), b2=b2, c2=c2,
                    first=first, ref=ref, want=continuation(ref))
