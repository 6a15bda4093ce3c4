"""Helpers of tests/test_gpu_duals.py: seeded LPs at a chosen shape, seeded models of the modelling
surface, bit-for-bit comparisons, and the long-double dual vector of a basis."""
import numpy as np

import dantzig_amd as dz
from dantzig_amd import core


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def assert_bit_equal(got, want, what=""):
    """Equal bit for bit; zeros of either sign compare equal, and so do NaNs of any payload."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    same = (bits(got) == bits(want)) | ((got == 0.0) & (want == 0.0)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"{what}: {np.count_nonzero(~same)} of {same.size} values differ"


def assert_same_run(got, want, what=""):
    """status, iterations, the whole pivot log (mu bit for bit), basis, nonbasis, x, xbar, z, zbar,
    objective."""
    assert got.status == want.status, what
    assert got.iterations == want.iterations, what
    assert [p[:3] for p in got.pivots] == [tuple(p[:3]) for p in want.pivots], what
    assert_bit_equal([p[3] for p in got.pivots], [p[3] for p in want.pivots], f"{what} mu")
    assert np.asarray(got.basis).tolist() == np.asarray(want.basis).tolist(), what
    assert np.asarray(got.nonbasis).tolist() == np.asarray(want.nonbasis).tolist(), what
    for name in ("x", "xbar", "z", "zbar"):
        assert_bit_equal(getattr(got, name), getattr(want, name), f"{what} {name}")
    assert_bit_equal([got.objective], [want.objective], f"{what} objective")


def family(seed, kind, m, ns):
    """The data of tests/lp_families.make_lp's kinds at a chosen shape."""
    rng = np.random.default_rng(seed)
    if kind == 0:
        a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
        return np.array(a), b, c
    if kind == 1:
        return (rng.integers(-3, 4, (m, ns)).astype(np.float64),
                rng.integers(-2, 9, m).astype(np.float64), rng.integers(-4, 5, ns).astype(np.float64))
    return ((rng.uniform(size=(m, ns)) < 0.3).astype(np.float64),
            rng.integers(0, 4, m).astype(np.float64), rng.integers(-1, 6, ns).astype(np.float64))


def random_problem(rng, rows):
    """A small model with bounded, free and one-sided variables and <=, >=, == rows: (variables,
    Minimize or Maximize)."""
    nv = int(rng.integers(1, 8))
    kinds = rng.integers(0, 4, nv)
    vs = []
    for k in kinds:
        if k == 0:
            vs.append(dz.Variable.nonneg())
        elif k == 1:
            vs.append(dz.Variable.free())
        elif k == 2:
            vs.append(dz.Variable(lb=float(rng.integers(-3, 1)), ub=float(rng.integers(1, 5))))
        else:
            vs.append(dz.Variable(lb=None, ub=float(rng.integers(0, 4))))
    obj = sum(float(rng.integers(-3, 4)) * v for v in vs) + float(rng.integers(-2, 3))
    cons = []
    for _ in range(rows):
        idx = rng.choice(nv, size=int(rng.integers(1, nv + 1)), replace=False)
        lhs = sum(float(rng.integers(-3, 4)) * vs[i] for i in idx)
        rhs = float(rng.integers(-2, 8))
        op = int(rng.integers(0, 5))
        cons.append(lhs == rhs if op == 0 else (lhs >= rhs if op == 1 else lhs <= rhs))
    cls = dz.Minimize if rng.integers(0, 2) else dz.Maximize
    return vs, cls(obj).subject_to(cons)


def long_double_y(bmat, c_b, steps: int = 3):
    """y with B^T y = c_B: a double LU solve refined with residuals formed in long double, the way
    tests/state_check.py computes the state a basis defines."""
    import scipy.linalg as sla

    ld = np.longdouble
    lu = sla.lu_factor(bmat)
    b_ld, rhs = bmat.astype(ld), np.asarray(c_b, dtype=ld)
    y = sla.lu_solve(lu, rhs.astype(np.float64), trans=1).astype(ld)
    for _ in range(steps):
        y = y + sla.lu_solve(lu, (rhs - b_ld.T @ y).astype(np.float64), trans=1).astype(ld)
    return y
