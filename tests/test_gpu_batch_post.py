"""Duals, ranging and rays behind a FAST batch on the GPU (dzg_batch_solve_post, csrc/k_batch_post.hip,
DESIGN 7n).  Planted cases (tests/planted.py, shapes of tests/batch_post_reference.py) enter through
start=(basis, nonbasis) on the slack-basis form, so the restart state of the planted basis is where
the solve stops before its first pivot; everything is measured against long double with numpy's
double-precision solve of the same basis as the yardstick (bound C_DUALS = 32, the metric and the
checks of tests/test_gpu_planted_postsolve.py; ranges are held to the winning variable).

Error ratios an MI355X shows (device error / numpy's error, bound 32; pytest -s prints them) are in
C_BATCH_POST_OBSERVED below."""
import copy
import functools

import numpy as np
import pytest

from dantzig_amd import core
from tests import batch_from_reference as bfr
from tests import batch_post_reference as bpr
from tests import duals_reference as dref
from tests import planted as pl
from tests import ranging_reference as rgref
from tests import rays_reference as rref
from tests import state_check as sc
from tests.lp_families import make_lp
from tests.duals_helpers import assert_bit_equal, assert_same_run, family
from tests.rays_helpers import LD, dense_ray_vectors, infeasible_lp, numpy_solve, refined_solve, unbounded_lp
from tests.test_gpu_duals import C_DUALS, _metric
from tests.test_gpu_planted_postsolve import RANGE_FIELDS, VAR_FIELDS, _check_both, _check_duals

pytestmark = pytest.mark.gpu

# (cost ranges, rhs ranges, y, d_N) per optimal shape, (d, y) per ray shape (the largest over the four
# kinds).  Where the ratio reads 0.000 the error is below the 1e-13 floor.
C_BATCH_POST_OBSERVED = {
    "2x3x1": (0.043, 0.000, 0.000, 0.000), "16x24x7": (0.682, 0.426, 0.193, 0.481),
    "17x12x6": (0.391, 0.213, 0.103, 0.187), "32x40x32": (0.335, 0.483, 0.451, 0.352),
    "33x15x9": (4.458, 0.444, 3.476, 4.109), "64x64x20": (0.860, 1.628, 0.840, 0.879),
    "65x8x5": (3.057, 0.044, 0.170, 0.170), "128x192x50": (0.759, 0.561, 1.095, 1.652),
    "128x130x128": (4.597, 2.746, 5.784, 12.071),
    "16x24x7 rays": (0.479, 0.516), "33x15x9 rays": (4.535, 0.402), "64x64x20 rays": (2.006, 1.206),
    "128x192x50 rays": (2.000, 0.556)}

IDS = ["x".join(map(str, s)) for s in bpr.SHAPES]
RAY_IDS = ["x".join(map(str, s)) for s in bpr.RAY_SHAPES]
FASTN = dict(numerics=core.FAST)


def _lp(p):
    return core.CoreLP.from_inequality_form(p.a, p.b, p.c)


def _with_ray(ranged, rayed):
    """solve_batch's ranging call carries no ray: one result with both calls' post-solves."""
    out = copy.copy(ranged)
    out.ray = rayed.ray
    return out


def _same_post(got, want, what):
    """Result and post-solve of two solves of one LP, bit for bit."""
    assert_same_run(got, want, what)
    assert (got.duals is None) == (want.duals is None) and (got.ray is None) == (want.ray is None), what
    assert (got.ranging is None) == (want.ranging is None), what
    if got.duals is not None:
        assert_bit_equal(got.duals.y, want.duals.y, what + " y")
        assert_bit_equal(got.duals.d, want.duals.d, what + " d")
        for f in ("primal_obj", "dual_obj", "primal_infeas", "dual_infeas", "z_diff"):
            assert_bit_equal([getattr(got.duals, f)], [getattr(want.duals, f)], f"{what} {f}")
    if got.ranging is not None:
        for f in RANGE_FIELDS:
            assert_bit_equal(getattr(got.ranging, f), getattr(want.ranging, f), f"{what} {f}")
        for f in VAR_FIELDS:
            assert getattr(got.ranging, f).tolist() == getattr(want.ranging, f).tolist(), f"{what} {f}"
    if got.ray is not None:
        assert_bit_equal(got.ray.d, want.ray.d, what + " ray d")
        assert_bit_equal(got.ray.y, want.ray.y, what + " ray y")
        assert_bit_equal([got.ray.mu, got.ray.value, got.ray.violation],
                         [want.ray.mu, want.ray.value, want.ray.violation], what + " ray scalars")
        assert (got.ray.kind, got.ray.var, got.ray.pos, got.ray.proven) == \
            (want.ray.kind, want.ray.var, want.ray.pos, want.ray.proven), what


# ------------------------------------------------------------------ 1. planted optima under FAST
@functools.lru_cache(maxsize=None)
def _optimal_batch():
    """Every optimal shape in one ragged call: (plants, requests, results)."""
    plants = [bpr.optimal_plant(s) for s in bpr.SHAPES]
    reqs = [pl.unit_and_pair_directions(p.a.shape[0], p.a.shape[0], sum(p.a.shape)) for p in plants]
    res = core.solve_batch_fast([_lp(p) for p in plants], start=[(p.basis, p.nonbasis) for p in plants],
                                duals=True, ranging=reqs, **FASTN)
    return plants, reqs, res


@pytest.mark.parametrize("shape", bpr.SHAPES, ids=IDS)
def test_planted_optimum_against_long_double(shape):
    plants, reqs, res = _optimal_batch()
    i = bpr.SHAPES.index(shape)
    p, (cost, rhs), r = plants[i], reqs[i], res[i]
    what = IDS[i]
    assert (r.status, r.numerics, r.iterations) == ("optimal", "fast", 0), what
    assert r.basis.tolist() == p.basis.tolist() and r.nonbasis.tolist() == p.nonbasis.tolist()
    exact = pl.exact_duals(p.a, p.cc, p.basis, p.nonbasis)
    numpy_ = pl.numpy_duals(p.a, p.cc, p.basis, p.nonbasis)
    ry, rd = _check_duals(r.duals, p.basis, p.nonbasis, exact, numpy_, what)
    want = pl.reference_sides(p.a, p.basis, p.nonbasis, r.x, exact[1], cost, rhs)
    yard = pl.reference_sides(p.a, p.basis, p.nonbasis, r.x, numpy_[1], cost, rhs, exact=False)
    rc, rr = _check_both(r.ranging, want, yard, p.basis, p.nonbasis, what)
    print(f'\nOBSERVED "{what}": ({rc["ratio"]:.3f}, {rr["ratio"]:.3f}, {ry:.3f}, {rd:.3f}),')
    # the ragged batch equals the case alone, bit for bit; asked twice gives the same bits
    alone = core.solve_batch_fast([_lp(p)], start=[(p.basis, p.nonbasis)], duals=True, ranging=[(cost, rhs)], **FASTN)[0]
    _same_post(r, alone, what + ": in the ragged batch and alone")
    # ... and the solve's result is what the call without the post-solve gives
    plain = core.solve_batch_fast([_lp(p)], start=[(p.basis, p.nonbasis)], **FASTN)[0]
    assert_same_run(alone, plain, what + ": with and without the post-solve")
    assert plain.duals is None and plain.ranging is None and plain.ray is None


def test_all_slack_basis_takes_the_permutation_path():
    rng = np.random.default_rng(3)
    a, b, c = rng.uniform(-1, 1, (20, 30)), rng.uniform(0.5, 2, 20), -rng.uniform(0.5, 2, 30)
    r = core.solve_batch_fast([core.CoreLP.from_inequality_form(a, b, c)], duals=True, ranging=True, rays=True,
                              **FASTN)[0]
    assert (r.status, r.iterations, r.refactors) == ("optimal", 0, 0)
    assert (r.duals.y == 0.0).all() and r.duals.dual_obj == 0.0 and r.duals.z_diff == 0.0 and r.ray is None
    assert_bit_equal(r.duals.d[:30], -c, "d_N = -c")
    ref = bpr.duals(a, b, np.concatenate([c, np.zeros(20)]), 0.0, r.basis, r.nonbasis, r.x, r.z)
    want_c, want_r = bpr.ranges(a, r.basis, r.nonbasis, r.x, ref.d, ref.w, [{j: 1.0} for j in range(50)],
                                [{i: 1.0} for i in range(20)])
    assert_bit_equal(r.ranging.cost_lo, [w.lo for w in want_c], "cost_lo")
    assert_bit_equal(r.ranging.cost_hi, [w.hi for w in want_c], "cost_hi")
    assert_bit_equal(r.ranging.rhs_lo, [w.lo for w in want_r], "rhs_lo")
    assert r.ranging.rhs_lo_var.tolist() == [w.lo_var for w in want_r]


# ------------------------------------------------------------------ 2. planted rays under FAST
@pytest.mark.parametrize("kind", pl.RAY_KINDS)
@pytest.mark.parametrize("shape", bpr.RAY_SHAPES, ids=RAY_IDS)
def test_planted_ray_against_long_double(shape, kind):
    m, ns, k = shape
    p = bpr.ray_plant(kind, shape)
    status = kind.split("-")[0]
    what = f"{m}x{ns}x{k} {kind}"
    r, again = core.solve_batch_fast([_lp(p)] * 2, start=[(p.basis, p.nonbasis)] * 2, duals=True, ranging=True,
                                     rays=True, **FASTN)
    _same_post(r, again, what + ": two places of one batch")
    assert (r.status, r.numerics, r.iterations) == (status, "fast", 0), what
    assert r.duals is None and r.ranging is None
    ray = r.ray
    assert (ray.pos, ray.var, ray.proven) == (p.pos, p.var, True), what
    assert ray.kind == ("primal" if status == "unbounded" else "farkas")
    # mu is the first-pivot ratio of the carried state, one division: the same bits
    want_pos, want_mu = bpr.first_pivot(r.z, r.zbar) if status == "unbounded" else bpr.first_pivot(r.x, r.xbar)
    assert want_pos == ray.pos
    assert_bit_equal([ray.mu], [want_mu], what + " mu")
    code = rref.PRIMAL if status == "unbounded" else rref.FARKAS
    d_hat, y_hat = dense_ray_vectors(p.a, p.basis, p.nonbasis, code, p.pos, refined_solve)
    d_np, y_np = dense_ray_vectors(p.a, p.basis, p.nonbasis, code, p.pos, numpy_solve)
    base_d, base_y = _metric(d_np, d_hat), _metric(y_np, y_hat)
    err_d, err_y = _metric(ray.d, d_hat), _metric(ray.y, y_hat)
    print(f'\nOBSERVED "{what}": ({err_d / max(base_d, 1e-13 / C_DUALS):.3f}, {err_y / max(base_y, 1e-13 / C_DUALS):.3f}),')
    assert err_d <= max(C_DUALS * base_d, 1e-13), (err_d, base_d)
    assert err_y <= max(C_DUALS * base_y, 1e-13), (err_y, base_y)
    value_hat = float(p.cc.astype(LD) @ d_hat) if code == rref.PRIMAL else float(np.asarray(p.b, dtype=LD) @ y_hat)
    tol = max(C_DUALS * base_d, C_DUALS * base_y, 1e-13)
    assert abs(ray.value - value_hat) <= tol * max(1.0, abs(value_hat)), (ray.value, value_hat)
    assert ray.violation == 0.0


# ------------------------------------------------------------------ 3. an exact tie
@pytest.mark.parametrize("dup_first", [False, True])
def test_exact_tie_goes_to_the_lower_nonbasic_position(dup_first):
    """One nonbasic structural column and its cost duplicated: both copies have the same delta and the
    same reduced cost in any arithmetic, so wherever one of them blocks a cost range the other ties."""
    p = bpr.optimal_plant((16, 24, 7))
    m, ns = p.a.shape
    # a nonbasic structural that blocks a cost range of a basic structural (by the CPU restatement)
    st = bpr.restart_of(p)
    ref = bpr.duals(p.a, p.b, p.cc, 0.0, p.basis, p.nonbasis, st.x, st.z)
    ends = bpr.ranges(p.a, p.basis, p.nonbasis, st.x, ref.d, ref.w, [{int(v): 1.0} for v in p.basis if v < ns], [])[0]
    j = next(int(v) for w in ends for v in (w.lo_var, w.hi_var) if 0 <= v < ns)
    a = np.concatenate([p.a, p.a[:, [j]]], axis=1)
    c = np.concatenate([p.c, [p.c[j]]])
    shift = lambda v: np.where(np.asarray(v) < ns, v, np.asarray(v) + 1)  # the slacks move up by one
    basis, nonbasis = shift(p.basis), shift(p.nonbasis)
    nonbasis = np.concatenate([[ns], nonbasis]) if dup_first else np.concatenate([nonbasis, [ns]])
    lower = int(ns if dup_first else j)
    cost = [{int(v): 1.0} for v in basis if v < ns]
    r = core.solve_batch_fast([core.CoreLP.from_inequality_form(a, p.b, c)], start=[(basis, nonbasis)],
                              ranging=[(cost, [])], **FASTN)[0]
    assert (r.status, r.iterations) == ("optimal", 0)
    assert_bit_equal([r.duals.d[j]], [r.duals.d[ns]], "the two copies' reduced costs")
    blocked = [v for v in r.ranging.cost_lo_var.tolist() + r.ranging.cost_hi_var.tolist() if v in (j, ns)]
    assert blocked, "no cost range of a basic structural is blocked by the duplicated column"
    assert set(blocked) == {lower}, (blocked, lower)


# ------------------------------------------------------------------ 4. solved, not planted, cold under AUTO
def _oracle_refs(a, b, c, g):
    m, ns = a.shape
    sf = sc.stdform(a, ns, bfr.full_c(c, m), g)
    return sf, dref.core_duals(sf, g, rhs0=b)


def test_solved_lps_under_auto_against_the_references():
    """FAST results against duals_reference / ranging_reference / rays_reference on the final basis.
    Bound: the references are double-precision solves themselves, so a value is held to
    max(C_DUALS x numpy's error, 1e-13) + the reference's own error, both against long double (the
    triangle inequality on the metric of tests/test_gpu_duals.py).  LPs AUTO handed to STRICT equal
    solve_batch's post-solves bit for bit."""
    data = [family(31 + i, i % 3, 24 + 9 * i, 40 + 5 * i) for i in range(6)]
    data += [unbounded_lp(5, 20, 30), infeasible_lp(6, 33, 40), unbounded_lp(7, 70, 90), infeasible_lp(8, 64, 64)]
    # tests/test_gpu_batch_fast.py's tie family: AUTO hands most of these to STRICT
    data += [make_lp(9300 + i, 1, 4, 65) for i in range(12)]
    lps = [core.CoreLP.from_inequality_form(*d) for d in data]
    got = core.solve_batch_fast(lps, duals=True, ranging=True, rays=True)
    s_rg = core.solve_batch(lps, ranging=True)
    s_ry = core.solve_batch(lps, duals=True, rays=True)
    seen = set()
    for k, ((a, b, c), g) in enumerate(zip(data, got)):
        what = f"LP {k} ({g.status}, {g.numerics})"
        m, ns = a.shape
        if g.numerics == "strict":
            assert_same_run(g, s_rg[k], what)
            _same_post(g, _with_ray(s_rg[k], s_ry[k]), what + ": solve_batch's")
            continue
        seen.add(g.status)
        cc = bfr.full_c(c, m)
        if g.status == "optimal":
            sf, ref = _oracle_refs(a, b, c, g)
            y_hat, d_hat = pl.exact_duals(a, cc, g.basis, g.nonbasis)
            y_np, d_np = pl.numpy_duals(a, cc, g.basis, g.nonbasis)
            tol_y = max(C_DUALS * _metric(y_np, y_hat), 1e-13) + _metric(ref.y, y_hat)
            tol_d = max(C_DUALS * _metric(d_np, d_hat), 1e-13) + _metric(ref.d[g.nonbasis], d_hat)
            assert _metric(g.duals.y, ref.y) <= tol_y and _metric(g.duals.d, ref.d) <= tol_d, what
            assert abs(g.duals.dual_obj - ref.dual_obj) <= 1e-9 * max(1.0, abs(ref.dual_obj)), what
            # ranges against long double with the planted checker (which holds them to the winner too)
            cost, rhs = [{j: 1.0} for j in range(m + ns)], [{i: 1.0} for i in range(m)]
            want = pl.reference_sides(a, g.basis, g.nonbasis, g.x, d_hat, cost, rhs)
            yard = pl.reference_sides(a, g.basis, g.nonbasis, g.x, d_np, cost, rhs, exact=False)
            rg = g.ranging
            pl.check_ranges(rg.cost_lo, rg.cost_hi, rg.cost_lo_var, rg.cost_hi_var, want[0], yard[0], g.nonbasis, what)
            pl.check_ranges(rg.rhs_lo, rg.rhs_hi, rg.rhs_lo_var, rg.rhs_hi_var, want[1], yard[1], g.basis, what)
            ref_rg = rgref.CoreRanging(sf, g, ref)
            for j in (0, m + ns - 1):
                w = ref_rg.cost({j: 1.0})
                assert (int(rg.cost_lo_var[j]), int(rg.cost_hi_var[j])) == (w.lo_var, w.hi_var), (what, j)
        elif g.status in ("unbounded", "infeasible"):
            sf = sc.stdform(a, ns, cc, g)
            ref = rref.core_ray(sf, g, rhs0=b)
            ray = g.ray
            assert ray is not None and (ray.pos, ray.var, ray.proven) == (ref.pos, ref.var, ref.proven), what
            code = rref.PRIMAL if g.status == "unbounded" else rref.FARKAS
            d_hat, y_hat = dense_ray_vectors(a, g.basis, g.nonbasis, code, ref.pos, refined_solve)
            d_np, y_np = dense_ray_vectors(a, g.basis, g.nonbasis, code, ref.pos, numpy_solve)
            tol_d = max(C_DUALS * _metric(d_np, d_hat), 1e-13) + _metric(ref.d, d_hat)
            tol_y = max(C_DUALS * _metric(y_np, y_hat), 1e-13) + _metric(ref.y, y_hat)
            assert _metric(ray.d, ref.d) <= tol_d and _metric(ray.y, ref.y) <= tol_y, what
            assert_bit_equal([ray.mu], [ref.mu], what + " mu")
            assert abs(ray.value - ref.value) <= (tol_d + tol_y) * max(1.0, abs(ref.value)) * (m + ns), what
            assert ray.violation == ref.violation == 0.0, what
    assert {"optimal", "unbounded", "infeasible"} <= seen, seen  # FAST itself produced every kind
    handed = [g for g in got if g.numerics == "strict"]
    assert handed and any(g.duals is not None and g.ranging is not None for g in handed)  # AUTO's copy-back ran


# ------------------------------------------------------------------ 5. numerics=STRICT through the new call
def test_strict_cold_is_solve_batch_bit_for_bit():
    data = [family(41 + i, i % 3, 20 + 7 * i, 30 + 5 * i) for i in range(4)] + [unbounded_lp(5, 20, 30),
                                                                                 infeasible_lp(6, 33, 40)]
    lps = [core.CoreLP.from_inequality_form(*d) for d in data]
    got = core.solve_batch_fast(lps, numerics=core.STRICT, duals=True, ranging=True, rays=True)
    s_rg = core.solve_batch(lps, ranging=True)
    s_ry = core.solve_batch(lps, duals=True, rays=True)
    for k, g in enumerate(got):
        assert g.numerics == "strict"
        _same_post(g, _with_ray(s_rg[k], s_ry[k]), f"LP {k}")


def test_strict_warm_ranging_and_rays_are_the_references_on_the_final_state():
    """A start basis composes with ranging and rays through the new call: k_duals_small, k_ranging_small
    and k_rays_small on the final state, bit for bit the CPU references there (as
    tests/test_gpu_batch_from.py has it for duals)."""
    plants = [bpr.optimal_plant((33, 15, 9)), bpr.ray_plant("unbounded", (33, 15, 9)),
              bpr.ray_plant("infeasible-slack", (16, 24, 7))]
    lps = [_lp(p) for p in plants]
    got = core.solve_batch_fast(lps, start=[(p.basis, p.nonbasis) for p in plants], numerics=core.STRICT,
                                duals=True, ranging=True, rays=True)
    for k, (p, g) in enumerate(zip(plants, got)):
        what = f"LP {k} ({g.status})"
        m, ns = p.a.shape
        assert g.numerics == "strict"
        sf = sc.stdform(p.a, ns, p.cc, g)
        if g.status == "optimal":
            ref = dref.core_duals(sf, g, rhs0=p.b)
            assert_bit_equal(g.duals.y, ref.y, what + " y")
            assert_bit_equal(g.duals.d, ref.d, what + " d")
            rg = rgref.CoreRanging(sf, g, ref)
            for j in range(m + ns):
                w = rg.cost({j: 1.0})
                assert_bit_equal([g.ranging.cost_lo[j], g.ranging.cost_hi[j]], [w.lo, w.hi], f"{what} cost {j}")
                assert (int(g.ranging.cost_lo_var[j]), int(g.ranging.cost_hi_var[j])) == (w.lo_var, w.hi_var)
            for i in range(m):
                w = rg.rhs({i: 1.0})
                assert_bit_equal([g.ranging.rhs_lo[i], g.ranging.rhs_hi[i]], [w.lo, w.hi], f"{what} rhs {i}")
                assert (int(g.ranging.rhs_lo_var[i]), int(g.ranging.rhs_hi_var[i])) == (w.lo_var, w.hi_var)
        else:
            ref = rref.core_ray(sf, g, rhs0=p.b)
            assert g.ray is not None and g.duals is None and g.ranging is None
            assert_bit_equal(g.ray.d, ref.d, what + " ray d")
            assert_bit_equal(g.ray.y, ref.y, what + " ray y")
            assert_bit_equal([g.ray.value, g.ray.violation, g.ray.mu], [ref.value, ref.violation, ref.mu], what)
            assert (g.ray.pos, g.ray.var, g.ray.proven) == (ref.pos, ref.var, ref.proven)
    assert [g.status for g in got] == ["optimal", "unbounded", "infeasible"]


# ------------------------------------------------------------------ 6. the handle against the stateless call
def _moved(lp, seed, scale=1e-2):
    rng = np.random.default_rng(seed)
    m, ns = lp.m, lp.n_struct
    b = np.asarray(lp.x) * (1.0 + scale * rng.uniform(-1, 1, m))
    c = np.asarray(lp.c).copy()
    c[:ns] = c[:ns] * (1.0 + scale * rng.uniform(-1, 1, ns))
    return b, c


@pytest.mark.parametrize("numerics", [core.FAST, core.AUTO, core.STRICT], ids=["fast", "auto", "strict"])
def test_handle_equals_the_stateless_call(numerics):
    data = [family(51 + i, i % 3, 12 + 11 * i, 20 + 9 * i) for i in range(6)]
    data += [unbounded_lp(5, 20, 30), infeasible_lp(6, 33, 40)] + [make_lp(9300 + i, 1, 4, 65) for i in range(4)]
    lps = [core.CoreLP.from_inequality_form(*d) for d in data]
    kw = dict(duals=True, ranging=True, rays=True)
    with core.BatchSolver(lps, numerics=numerics) as h, core.BatchSolver(lps, numerics=numerics) as plain:
        first = h.solve(**kw)
        want = core.solve_batch_fast(lps, numerics=numerics, **kw)
        for k, (g, w) in enumerate(zip(first, want)):
            _same_post(g, w, f"cold LP {k}")
        # with and without the post-solve: the same res bits, and the next re-solve is unchanged
        for k, (g, w) in enumerate(zip(first, plain.solve())):
            assert_same_run(g, w, f"cold LP {k}: with and without")
            assert w.duals is None and w.ranging is None and w.ray is None
        changes = [(i,) + _moved(lps[i], 70 + i) for i in range(len(lps))]
        for hh in (h, plain):
            hh.update_many([(i, b, c) for i, b, c in changes])
        now = [core.CoreLP.from_inequality_form(d[0], b, c[:d[0].shape[1]]) for d, (_, b, c) in zip(data, changes)]
        warm = h.solve(**kw)
        for k, (g, w) in enumerate(zip(warm, plain.solve())):
            assert_same_run(g, w, f"warm LP {k}: after a solve with and one without the post-solve")
        want = core.solve_batch_fast(now, start=first, numerics=numerics, **kw)
        for k, (g, w) in enumerate(zip(warm, want)):
            _same_post(g, w, f"warm LP {k}")
        # a subset, in another order, asked twice
        which = [7, 2, 9, 0]
        sub = h.solve(which=which, **kw)
        again = h.solve(which=which, **kw)
        want = core.solve_batch_fast([now[i] for i in which], start=[warm[i] for i in which], numerics=numerics, **kw)
        for k, (g, a, w) in enumerate(zip(sub, again, want)):
            _same_post(g, w, f"which[{k}]")
            assert g.basis.tolist() == a.basis.tolist()
            for f in ("duals", "ranging", "ray"):
                assert (getattr(g, f) is None) == (getattr(a, f) is None)
            if g.duals is not None:
                assert_bit_equal(g.duals.y, a.duals.y, f"which[{k}] asked twice: y")
                assert_bit_equal(g.ranging.cost_lo, a.ranging.cost_lo, f"which[{k}] asked twice: cost_lo")
            if g.ray is not None:
                assert_bit_equal(g.ray.d, a.ray.d, f"which[{k}] asked twice: ray d")
    if numerics == core.AUTO:
        assert {g.numerics for g in first} == {"fast", "strict"}


# ------------------------------------------------------------------ 7. bucket 3's second chunk
def test_257_lps_of_65x8_equal_the_same_lp_alone():
    plants = [pl.planted_optimal(900 + i, 65, 8, 5) for i in range(4)]
    lps = [_lp(plants[i % 4]) for i in range(257)]
    start = [(plants[i % 4].basis, plants[i % 4].nonbasis) for i in range(257)]
    got = core.solve_batch_fast(lps, start=start, duals=True, ranging=True, log=False, **FASTN)
    alone = [core.solve_batch_fast([lps[i]], start=[start[i]], duals=True, ranging=True, log=False, **FASTN)[0]
             for i in range(4)]
    for i, g in enumerate(got):
        assert g.status == "optimal" and g.ranging is not None
        _same_post(g, alone[i % 4], f"LP {i}")


# ------------------------------------------------------------------ 8. the modelling surface
def _surface_models():
    import dantzig_amd as dz
    from tests.test_batch_from_host import session_problems

    problems = [p for p, _, _ in session_problems()]
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    problems.append(dz.Maximize(x + y).subject_to([x - y <= 1.0]))              # unbounded
    problems.append(dz.Maximize(x).subject_to([x + y <= 1.0, x >= 2.0]))        # infeasible
    return problems


class _Var:
    """A model's variable as Solution.reduced_cost / objective_range look it up."""

    def __init__(self, rust_variable):
        self._v = rust_variable

    def to_rust_variable(self):
        return self._v


def _variables(batch, i):
    return [_Var(v) for v in batch._models[i].order]


def _close(got, want, what):
    """The surface's own bound, NOT the metric of groups 1, 2 and 4 (32 x numpy's error against long
    double): two double-precision results of a model have no long-double yardstick at this level, so a
    value computed twice -- by the batch's post-solve and by the single solver's -- is held to
    tests/rays_helpers.TOL_VALUE, 1e-9 relative, the tolerance the project's model-level tests use for a
    well-conditioned model.  The core-level accuracy behind these values is what groups 1, 2 and 4
    check, and the STRICT session is checked bit for bit below."""
    from tests.rays_helpers import TOL_VALUE
    if np.isinf(want) or np.isinf(got):
        assert got == want, (what, got, want)
    else:
        assert abs(got - want) <= TOL_VALUE * max(1.0, abs(want)), (what, got, want)


@pytest.mark.parametrize("mode", ["fast", "resident", "strict"])
def test_sessions_answer_duals_ranges_and_rays(mode):
    import dantzig_amd as dz
    from dantzig_amd.exceptions import InfeasibleError, UnboundedError

    problems = _surface_models()
    kw = dict(fast=True) if mode == "fast" else dict(resident=True) if mode == "resident" else {}
    with dz.sessions(problems, **kw) as batch:
        got = batch.solve(duals=True, ranging=True, rays=True, return_exceptions=True)
        with dz.sessions(problems, **kw) as other:
            plain = other.solve(return_exceptions=True)
    assert isinstance(got[-2], UnboundedError) and isinstance(got[-1], InfeasibleError)
    assert got[-2].ray is not None and got[-2].ray.proven and got[-1].ray is not None and got[-1].ray.proven
    assert got[-2].ray.objective_rate > 0.0
    if mode == "strict":  # the first call is solve_many's, bit for bit
        many_rg = dz.solve_many(problems, duals=True, ranging=True, return_exceptions=True)
        many_ry = dz.solve_many(problems, rays=True, return_exceptions=True)
        assert repr(got[-2].ray) == repr(many_ry[-2].ray) and repr(got[-1].ray) == repr(many_ry[-1].ray)
    for i, p in enumerate(problems[:-2]):
        g = got[i]
        assert g.objective_value == plain[i].objective_value, i  # the post-solve does not move the solve
        want = p.solve(duals=True, ranging=True)
        _close(g.objective_value, want.objective_value, f"model {i} objective")
        cert = g.certificate
        assert cert.source == "fresh" and abs(cert.gap) <= 1e-9 * max(1.0, abs(cert.primal_objective)), (i, cert)
        for c in p.constraints:
            _close(g.dual(c), want.dual(c), f"model {i} dual")
            for a, b in zip((g.rhs_range(c).lo, g.rhs_range(c).hi), (want.rhs_range(c).lo, want.rhs_range(c).hi)):
                _close(a, b, f"model {i} rhs_range")
        for v in _variables(batch, i):
            _close(g.reduced_cost(v), want.reduced_cost(v), f"model {i} reduced cost")
            for a, b in zip((g.objective_range(v).lo, g.objective_range(v).hi),
                            (want.objective_range(v).lo, want.objective_range(v).hi)):
                _close(a, b, f"model {i} objective_range")
        if mode == "strict":
            m = many_rg[i]
            assert g.objective_value == m.objective_value
            for c in p.constraints:
                assert g.dual(c) == m.dual(c) and g.rhs_range(c) == m.rhs_range(c), i
            for v in _variables(batch, i):
                assert g.reduced_cost(v) == m.reduced_cost(v) and g.objective_range(v) == m.objective_range(v), i
