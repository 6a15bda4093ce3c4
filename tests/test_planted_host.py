"""tests/planted.py on the CPU: every planted LP the GPU tests use ends where it was planted on the
CPU oracle, before its first pivot; numpy's own double-precision ranges pass the range checker, and
three ways of getting the winner or the last tile wrong do not."""
import functools

import numpy as np
import pytest

from oracle import oracle as ora
from tests import planted as pl
from tests import ranging_reference as rref
from tests import rays_reference as rayref

IDS = ["x".join(str(v) for v in case) for case in pl.OPTIMAL_CASES]


@functools.lru_cache(maxsize=None)
def _case(case):
    p = pl.optimal_case(*case)
    m, ns = p.a.shape
    cost, rhs = pl.unit_and_pair_directions(case[0], m, m + ns)
    y, d = pl.exact_duals(p.a, p.cc, p.basis, p.nonbasis)
    want = pl.reference_sides(p.a, p.basis, p.nonbasis, p.x, d, cost, rhs)
    _, d_np = pl.numpy_duals(p.a, p.cc, p.basis, p.nonbasis)
    yard = pl.reference_sides(p.a, p.basis, p.nonbasis, p.x, d_np, cost, rhs, exact=False)
    return p, cost, rhs, want, yard


def _arrays(side):
    return ([w.lo for w in side.ranges], [w.hi for w in side.ranges], [w.lo_var for w in side.ranges],
            [w.hi_var for w in side.ranges])


# ------------------------------------------------------------------ 1. the generator
@pytest.mark.parametrize("case", pl.OPTIMAL_CASES, ids=IDS)
def test_planted_optimum_invariants_and_oracle_verdict(case):
    m, ns, k, g = case
    p, cost, rhs, want, yard = _case(case)
    a, b, c, basis, nonbasis, x, z = p
    assert a.shape == (m, ns) and np.abs(a).max() <= 1.0
    assert sorted(basis.tolist() + nonbasis.tolist()) == list(range(m + ns))
    assert int((basis < ns).sum()) == k
    slack_at = np.flatnonzero(basis >= ns)
    if k > 0:
        assert (basis[slack_at] - ns != slack_at).all()          # no slack at its own row's position
        assert (np.diff(basis[basis < ns]) < 0).any() or k == 1  # S is not in order
    assert (nonbasis != np.sort(nonbasis)).any()
    assert (z > 0).all() and (x >= 0).all()
    assert int((x[basis < ns] == 0.0).sum()) == g and int((x[basis >= ns] == 0.0).sum()) == g
    assert p.zeros.tolist() == np.flatnonzero(x == 0.0).tolist()
    for v in (x[x != 0], z):
        assert ((v * 4 == np.round(v * 4)) & (v >= 0.25) & (v <= 2.0)).all()
    if g and m > 256:
        assert (p.zeros < 256).any() and (p.zeros >= 256).any()
    # the planted x is B^-1 b and the planted z the reduced costs, to rounding
    bm, nm, _ = pl.basis_columns(a, basis, nonbasis)
    assert np.abs(bm @ x - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    y_hat, d_hat = pl.exact_duals(a, p.cc, basis, nonbasis)
    assert float(np.abs(d_hat - z).max()) <= 1e-10
    res = ora.simplex_solve(pl.stdform(p))
    assert (res.status, res.iterations) == ("optimal", 0)
    # no direction is skipped: no long-double |delta| within a factor 2 of pivot_tol
    assert not any(want[0].near) and not any(want[1].near)


def test_sides_are_the_ranging_reference():
    # planted.reference_sides is tests/ranging_reference.ranges_from_inverse with the near-winners kept
    p, cost, rhs, want, yard = _case((33, 15, 9, 0))
    bm, nm, unit_rows = pl.basis_columns(p.a, p.basis, p.nonbasis)
    _, d_np = pl.numpy_duals(p.a, p.cc, p.basis, p.nonbasis)
    ref_c, ref_r, near_c, near_r = rref.ranges_from_inverse(np.linalg.solve(bm, np.eye(33)), nm, unit_rows,
                                                            p.basis, p.nonbasis, p.x, d_np, cost, rhs)
    assert yard[0].ranges == ref_c and yard[1].ranges == ref_r
    assert yard[0].near == near_c and yard[1].near == near_r


# ------------------------------------------------------------------ 2. the checker
@pytest.mark.parametrize("case", pl.OPTIMAL_CASES, ids=IDS)
def test_numpy_ranges_pass_the_checker(case):
    p, cost, rhs, want, yard = _case(case)
    rc = pl.check_ranges(*_arrays(yard[0]), want[0], yard[0], p.nonbasis, "cost")
    rr = pl.check_ranges(*_arrays(yard[1]), want[1], yard[1], p.basis, "rhs")
    assert rc["skipped"] == rr["skipped"] == 0
    assert rc["directions"] == len(cost) and rr["directions"] == len(rhs)
    if case[3]:
        assert rr["exact_ties"] >= 1  # some right-hand-side end is an exact tie of two or more positions


def _stand_in(deltas, clamped, variables, tol=rref.DEFAULT_TOL, keep=None, last_wins=False, positions=False):
    """The rule in double, with the three ways of getting it wrong as switches."""
    lo, hi, lo_var, hi_var = [], [], [], []
    clamped = np.asarray(clamped, dtype=np.float64)
    for delta in deltas:
        cand = np.abs(delta) > tol
        if keep is not None:
            cand &= keep
        with np.errstate(divide="ignore", invalid="ignore"):
            r = -(clamped / delta)
        for vals, vars_, picks, best_of, none in ((lo, lo_var, np.flatnonzero(cand & (delta > 0)), np.max, -np.inf),
                                                  (hi, hi_var, np.flatnonzero(cand & ~(delta > 0)), np.min, np.inf)):
            if not len(picks):
                vals.append(none)
                vars_.append(-1)
                continue
            best = best_of(r[picks])
            ties = picks[r[picks] == best]
            k = int(ties[-1] if last_wins else ties[0])
            vals.append(float(best))
            vars_.append(k if positions else int(variables[k]))
    return lo, hi, lo_var, hi_var


def _double_deltas(p, cost, rhs):
    bm, nm, unit_rows = pl.basis_columns(p.a, p.basis, p.nonbasis)
    inv = np.linalg.solve(bm, np.eye(len(p.basis)))
    _, d_np = pl.numpy_duals(p.a, p.cc, p.basis, p.nonbasis)
    return (list(pl.cost_deltas(inv, nm, unit_rows, p.basis, p.nonbasis, cost)), np.maximum(d_np, 0.0),
            list(pl.rhs_deltas(inv, rhs)), np.maximum(p.x, 0.0))


def test_checker_rejects_three_wrong_stand_ins():
    # ties: the degenerate plant, right-hand-side ranges
    p, cost, rhs, want, yard = _case((97, 161, 40, 6))
    dc, clamped_c, dr, clamped_r = _double_deltas(p, cost, rhs)
    good = _stand_in(dr, clamped_r, p.basis)
    assert [list(v) for v in good] == [list(v) for v in _arrays(yard[1])]
    pl.check_ranges(*good, want[1], yard[1], p.basis, "rhs")
    with pytest.raises(AssertionError, match="exact tie"):
        pl.check_ranges(*_stand_in(dr, clamped_r, p.basis, last_wins=True), want[1], yard[1], p.basis, "rhs")
    # winners reported as positions instead of variables
    with pytest.raises(AssertionError, match="winner"):
        pl.check_ranges(*_stand_in(dr, clamped_r, p.basis, positions=True), want[1], yard[1], p.basis, "rhs")
    with pytest.raises(AssertionError, match="winner"):
        pl.check_ranges(*_stand_in(dc, clamped_c, p.nonbasis, positions=True), want[0], yard[0], p.nonbasis, "cost")
    # the last column tile of 64 nonbasic positions dropped: q = 192 is three full tiles
    p, cost, rhs, want, yard = _case((128, 192, 50, 0))
    dc, clamped_c, _, _ = _double_deltas(p, cost, rhs)
    pl.check_ranges(*_stand_in(dc, clamped_c, p.nonbasis), want[0], yard[0], p.nonbasis, "cost")
    with pytest.raises(AssertionError):
        pl.check_ranges(*_stand_in(dc, clamped_c, p.nonbasis, keep=np.arange(192) < 128), want[0], yard[0],
                        p.nonbasis, "cost")


# ------------------------------------------------------------------ 3. the ray plants
@pytest.mark.parametrize("kind", pl.RAY_KINDS)
@pytest.mark.parametrize("shape", pl.RAY_SHAPES, ids=["x".join(map(str, s)) for s in pl.RAY_SHAPES])
def test_planted_rays_stop_before_the_first_pivot(shape, kind):
    m, ns, k = shape
    p = pl.ray_case(kind, *shape)
    assert int((p.basis < ns).sum()) == k
    assert (p.var >= ns) == kind.endswith("-slack")
    sf = pl.stdform(p)
    res = ora.simplex_solve(sf)
    assert (res.status, res.iterations) == (kind.split("-")[0], 0)
    ray = rayref.core_ray(sf, res, rhs0=p.b)  # the right-hand side of the rows, not the planted x
    assert (ray.pos, ray.var) == (p.pos, p.var)
    assert ray.proven and ray.violation == 0.0
    assert abs(abs(ray.value) - 1.0) <= 1e-9  # the planted reduced cost -1 / the planted x = -1
    if kind.startswith("unbounded"):
        assert p.nonbasis[p.pos] == p.var and p.z[p.pos] == -1.0 and (np.delete(p.z, p.pos) > 0).all()
        assert (ray.vec <= -0.25 + 1e-9).all()  # B^-1 a_j = -u, u >= 1/4
    else:
        assert p.basis[p.pos] == p.var and p.x[p.pos] == -1.0 and (np.delete(p.x, p.pos) > 0).all()
        assert (ray.vec <= -0.25 + 1e-9).all()  # dz = -N^T y, y.a_j >= 1/4 at every nonbasic j
