"""The FAST route of duals(), ranging() and ray() (csrc/k_ranging.hip, csrc/k_rays.hip, the k_drift_y
reuse of dzg_solver_duals) on bases built to order (tests/planted.py): every handle starts in its
final state and stops before its first pivot, so the shapes, the number of basic structurals, the
places of the slacks, the ties and the entering or leaving variable are chosen, not met by accident.
Everything is measured against long double with numpy's double-precision solve of the same basis as
the yardstick (bound C_DUALS = 32, the metric of tests/test_gpu_duals.py); the ranges are held to the
winning variable as well as to the endpoint (planted.check_ranges).

Error ratios an MI355X shows (device error / numpy's error, bound 32; pytest -s prints them) are in
C_PLANTED_OBSERVED below."""
import functools

import numpy as np
import pytest

from dantzig_amd import core
from tests import planted as pl
from tests import ranging_reference as rgref
from tests import rays_reference as rref
from tests.duals_helpers import assert_bit_equal, family as _family
from tests.rays_helpers import LD, dense_ray_vectors, numpy_solve, refined_solve
from tests.test_gpu_duals import C_DUALS, _metric, _same_state
from tests.test_gpu_ranging import _assert_same_duals

pytestmark = pytest.mark.gpu

# (cost ranges, rhs ranges, y, d_N) per optimal case, (cost, rhs) per pivot_tol, (d, y) per ray case
# (the largest over the four kinds of a shape), (cost, rhs, y, d_N) per ending of the 97x161 solve.  No
# direction was skipped in any case.  Where the ratio reads 0.000 the error is below the 1e-13 floor.
C_PLANTED_OBSERVED = {
    "64x64x20": (0.288, 0.659, 0.344, 0.339), "128x192x50": (0.205, 0.854, 0.406, 0.587),
    "33x15x9": (0.832, 0.178, 0.559, 0.627), "8x4200x6": (0.924, 0.100, 0.227, 0.458),
    "300x520x120": (1.032, 1.008, 1.211, 1.012), "70x140x1": (0.036, 0.002, 0.000, 0.018),
    "70x140x63": (0.428, 0.717, 0.461, 0.343), "70x140x64": (0.505, 1.662, 0.694, 0.627),
    "70x140x65": (2.839, 1.529, 6.318, 6.146), "70x140x70": (3.025, 1.047, 2.456, 2.405),
    "97x161x40 degenerate 6": (0.904, 0.000, 1.407, 0.984), "300x520x120 degenerate 8": (0.251, 0.000, 0.449, 0.291),
    "33x15x9 pivot_tol 1.183e-06": (1.599, 0.532), "33x15x9 pivot_tol 7.849e-03": (0.564, 0.089),
    "64x64x20 rays": (0.222, 0.015), "33x15x9 rays": (0.096, 0.020), "300x520x120 rays": (0.004, 0.001),
    "97x161 no refactorisation": (2.263, 1.636, 1.994, 2.634), "97x161 refactor_interval 17": (2.263, 1.663, 1.994, 2.634),
    "97x161 resumed at half": (2.263, 1.636, 1.994, 2.634)}

FAST = dict(numerics=core.FAST, refactor_interval=-1)
IDS = ["x".join(str(v) for v in case) for case in pl.OPTIMAL_CASES]
RANGE_FIELDS = ("cost_lo", "cost_hi", "rhs_lo", "rhs_hi")
VAR_FIELDS = ("cost_lo_var", "cost_hi_var", "rhs_lo_var", "rhs_hi_var")


def _same_ranges(r, again, what, cost=slice(None), rhs=slice(None)):
    """r equals again[cost] / again[rhs] bit for bit and in *_var."""
    for name in RANGE_FIELDS + VAR_FIELDS:
        part = cost if name.startswith("cost") else rhs
        got, want = getattr(r, name), getattr(again, name)[part]
        if name in VAR_FIELDS:
            assert got.tolist() == want.tolist(), f"{what} {name}"
        else:
            assert_bit_equal(got, want, f"{what} {name}")


@functools.lru_cache(maxsize=None)
def _reference(case, tol=0.0):
    """The planted LP of a case, its directions and the long-double and numpy sides: computed once."""
    p = pl.optimal_case(*case)
    m, ns = p.a.shape
    cost, rhs = pl.unit_and_pair_directions(case[0], m, m + ns)
    y_hat, d_hat = pl.exact_duals(p.a, p.cc, p.basis, p.nonbasis)
    y_np, d_np = pl.numpy_duals(p.a, p.cc, p.basis, p.nonbasis)
    want = pl.reference_sides(p.a, p.basis, p.nonbasis, p.x, d_hat, cost, rhs)
    yard = pl.reference_sides(p.a, p.basis, p.nonbasis, p.x, d_np, cost, rhs, exact=False)
    return p, cost, rhs, (y_hat, d_hat), (y_np, d_np), want, yard


def _check_duals(du, basis, nonbasis, exact, numpy_, what):
    """y and d_N against long double, the metric and bound of test_fast_fresh_duals_against_long_double."""
    (y_hat, d_hat), (y_np, d_np) = exact, numpy_
    assert du.source == "fresh" and (du.d[basis] == 0.0).all(), what
    base_y, base_d = _metric(y_np, y_hat), _metric(d_np, d_hat)
    err_y, err_d = _metric(du.y, y_hat), _metric(du.d[nonbasis], d_hat)
    ratio_y, ratio_d = err_y / max(base_y, 1e-13 / C_DUALS), err_d / max(base_d, 1e-13 / C_DUALS)
    print(f"\n{what}: y error {err_y:.3e} (ratio {ratio_y:.3f}), d_N error {err_d:.3e} (ratio {ratio_d:.3f})")
    assert err_y <= max(C_DUALS * base_y, 1e-13), (what, err_y, base_y)
    assert err_d <= max(C_DUALS * base_d, 1e-13), (what, err_d, base_d)
    assert du.primal_infeas <= 1e-9 and du.dual_infeas <= 1e-9, what
    # the dual objective is taken over the right-hand side of the rows, whatever state the handle started in
    gap = abs(du.primal_obj - du.dual_obj)
    print(f"{what}: primal {du.primal_obj!r}, dual {du.dual_obj!r}, gap {gap:.3e}")
    tol_gap = max(C_DUALS * base_y, C_DUALS * base_d, 1e-13)
    assert gap <= tol_gap * max(1.0, abs(du.primal_obj)), (what, du.primal_obj, du.dual_obj)
    return ratio_y, ratio_d


def _check_both(r, want, yard, basis, nonbasis, what):
    rc = pl.check_ranges(r.cost_lo, r.cost_hi, r.cost_lo_var, r.cost_hi_var, want[0], yard[0], nonbasis,
                         what + " cost")
    rr = pl.check_ranges(r.rhs_lo, r.rhs_hi, r.rhs_lo_var, r.rhs_hi_var, want[1], yard[1], basis, what + " rhs")
    print(f"\n{what}: {rc['directions']} cost + {rr['directions']} rhs directions, "
          f"{rc['skipped'] + rr['skipped']} skipped: cost error {rc['err']:.3e} (ratio {rc['ratio']:.3f}), "
          f"rhs error {rr['err']:.3e} (ratio {rr['ratio']:.3f}), exact ties {rc['exact_ties']} + {rr['exact_ties']}")
    assert rc["skipped"] == rr["skipped"] == 0, what  # (the planted cases skip none: tests/test_planted_host.py)
    assert (r.cost_lo <= 0.0).all() and (r.cost_hi >= 0.0).all() and (r.rhs_lo <= 0.0).all() \
        and (r.rhs_hi >= 0.0).all(), what
    return rc, rr


# ------------------------------------------------------------------ 1. ranging and duals
# shapes: m = 64 and 128 (the last K tile of k_range_cost_mfma is full, Y has no zero padding),
# m = 33 and 8 (one partial K tile), q = 39 (waves with no position), q = 108 / 270 (ragged), q = 4200
# (66 column tiles: the second trip of k_range_finish), q = 192 (the last column tile is full),
# m = 300 (two row tiles of k_range_rhs_fast); k = 1, 63, 64, 65 and k = m (no basic slack)
@pytest.mark.parametrize("case", pl.OPTIMAL_CASES, ids=IDS)
def test_planted_ranging_and_duals_against_long_double(case):
    m, ns, k, g = case
    p, cost, rhs, exact, numpy_, want, yard = _reference(case)
    what = IDS[pl.OPTIMAL_CASES.index(case)]
    with core.Solver(pl.core_lp(core, p), **FAST) as s:
        assert s.run(0) == "optimal"
        before = s.result(log=False)
        r = s.ranging(cost, rhs)
        after = s.result(log=False)
        again = s.ranging(cost, rhs)
        du = s.duals()
    assert before.iterations == 0 and before.dense_columns == k
    assert before.basis.tolist() == p.basis.tolist() and before.nonbasis.tolist() == p.nonbasis.tolist()
    assert_bit_equal(before.x, p.x, "the carried x is the planted x")
    _same_state(before, after, f"{what}: result() around ranging()")
    _same_ranges(r, again, f"{what}: second call")
    _assert_same_duals(r.duals, du, f"{what}: the duals of ranging() and of duals()")
    rc, rr = _check_both(r, want, yard, p.basis, p.nonbasis, what)
    _check_duals(du, p.basis, p.nonbasis, exact, numpy_, what)
    if g:
        # the test must not pass vacuously: some right-hand-side end is an exact tie of >= 2 positions
        assert rr["exact_ties"] >= 1, rr
        if m > 256:  # ... and one of them is decided across the two row tiles of k_range_rhs_fast
            across = [i for i, w in enumerate(want[1].ranges) for pos, _, zero in (want[1].close_lo[i], want[1].close_hi[i])
                      if len(pos) >= 2 and zero.all() and pos.min() < 256 <= pos.max()]
            assert across, what


# ------------------------------------------------------------------ 2. direction counts
# RC_DIRS = 32 directions per workgroup of k_range_cost_mfma, DZG_RANGE_CHUNK = 256 per launch
def test_direction_counts_equal_slices_of_the_whole_request():
    case = (128, 192, 50, 0)
    p, cost, rhs = _reference(case)[:3]
    cost, rhs = cost[:320], rhs[:128]  # the unit directions
    with core.Solver(pl.core_lp(core, p), **FAST) as s:
        assert s.run(0) == "optimal"
        whole = s.ranging(cost, rhs)
        for count in (1, 32, 33, 256, 257, 320):
            _same_ranges(s.ranging(cost[:count], []), whole, f"{count} cost directions", cost=slice(0, count),
                         rhs=slice(0, 0))
        for count in (1, 128):
            _same_ranges(s.ranging([], rhs[:count]), whole, f"{count} rhs directions", cost=slice(0, 0),
                         rhs=slice(0, count))
        # a slice that does not start at direction 0 of its chunk
        _same_ranges(s.ranging(cost[250:290], rhs[100:]), whole, "directions 250..289", cost=slice(250, 290),
                     rhs=slice(100, 128))


# ------------------------------------------------------------------ 3. pivot_tol
def _tolerances(p, cost, rhs, d_hat):
    """Two values of pivot_tol in gaps of the long-double |delta| of these directions: no |delta|
    within a factor 2 of either, and some |delta| between the default 1e-9 and each."""
    import math

    bm, nm, unit_rows = pl.basis_columns(p.a, p.basis, p.nonbasis)
    inv = rgref.refined_inverse(bm)
    sizes = np.concatenate([np.abs(d) for d in pl.cost_deltas(inv, nm, unit_rows, p.basis, p.nonbasis, cost)] +
                           [np.abs(d) for d in pl.rhs_deltas(inv, rhs)]).astype(np.float64)
    sizes = np.sort(sizes[sizes > 1e-15])  # (a delta that is zero by structure is zero to the inverse's rounding)
    gaps = [math.sqrt(lo * hi) for lo, hi in zip(sizes[:-1], sizes[1:]) if hi / lo >= 4.5]
    return gaps[-2:], sizes


def test_non_default_pivot_tol():
    case = (33, 15, 9, 0)
    p, _, _, exact, numpy_, _, _ = _reference(case)
    ns = 15
    # unit directions of the basic structurals and of the tight rows at three scales, so that their
    # deltas come in three bands with room for a tolerance between them
    scales = (1.0, 1e-4, 1e-8)
    cost = [{int(j): scales[i % 3]} for i, j in enumerate(j for j in p.basis if j < ns)]
    rhs = [{int(j - ns): scales[i % 3]} for i, j in enumerate(j for j in p.nonbasis if j >= ns)]
    tols, sizes = _tolerances(p, cost, rhs, exact[1])
    assert len(tols) == 2 and tols[0] != tols[1], tols
    default = pl.reference_sides(p.a, p.basis, p.nonbasis, p.x, exact[1], cost, rhs)
    with core.Solver(pl.core_lp(core, p), **FAST) as s:
        assert s.run(0) == "optimal"
        for tol in tols:
            assert not ((sizes >= tol / 2) & (sizes <= 2 * tol)).any()
            assert ((sizes > 2e-9) & (sizes < tol)).any()  # a candidate of the default tolerance is none of this one
            want = pl.reference_sides(p.a, p.basis, p.nonbasis, p.x, exact[1], cost, rhs, tol=tol)
            yard = pl.reference_sides(p.a, p.basis, p.nonbasis, p.x, numpy_[1], cost, rhs, tol=tol, exact=False)
            changed = sum(len(a[0]) != len(b[0]) or w.lo != v.lo or w.hi != v.hi
                          for side, other in zip(want, default)
                          for a, b, w, v in zip(side.close_lo + side.close_hi, other.close_lo + other.close_hi,
                                                side.ranges * 2, other.ranges * 2))
            r = s.ranging(cost, rhs, pivot_tol=tol)
            rc, rr = _check_both(r, want, yard, p.basis, p.nonbasis, f"33x15x9 pivot_tol {tol:.3e}")
            print(f"pivot_tol {tol:.3e}: {int((sizes < tol).sum())} of {len(sizes)} deltas are no candidates, "
                  f"{changed} ends differ from the default's")


# ------------------------------------------------------------------ 4. rays
@pytest.mark.parametrize("kind", pl.RAY_KINDS)
@pytest.mark.parametrize("shape", pl.RAY_SHAPES, ids=["x".join(map(str, s)) for s in pl.RAY_SHAPES])
def test_planted_rays_against_long_double(shape, kind):
    m, ns, k = shape
    p = pl.ray_case(kind, *shape)
    status = kind.split("-")[0]
    what = f"{m}x{ns}x{k} {kind}"
    with core.Solver(pl.core_lp(core, p), **FAST) as s:
        assert s.run(0) == status
        before = s.result(log=False)
        ray = s.ray()
        after = s.result(log=False)
        again = s.ray()
    assert before.iterations == 0 and before.dense_columns == k
    _same_state(before, after, f"{what}: result() around ray()")
    assert_bit_equal(ray.d, again.d, "second call d")
    assert_bit_equal(ray.y, again.y, "second call y")
    assert_bit_equal([ray.mu, ray.value, ray.violation], [again.mu, again.value, again.violation],
                     "second call scalars")
    assert (ray.var, ray.pos, ray.proven, ray.kind) == (again.var, again.pos, again.proven, again.kind)
    assert (ray.pos, ray.var) == (p.pos, p.var), what  # the planted ones
    assert (ray.var >= ns) == kind.endswith("-slack")
    if status == "unbounded":
        assert ray.kind == "primal" and (ray.y == 0.0).all()
    else:
        assert ray.kind == "farkas"
    kind_code = rref.PRIMAL if status == "unbounded" else rref.FARKAS
    d_hat, y_hat = dense_ray_vectors(p.a, p.basis, p.nonbasis, kind_code, p.pos, refined_solve)
    d_np, y_np = dense_ray_vectors(p.a, p.basis, p.nonbasis, kind_code, p.pos, numpy_solve)
    base_d, base_y = _metric(d_np, d_hat), _metric(y_np, y_hat)
    tol_d, tol_y = max(C_DUALS * base_d, 1e-13), max(C_DUALS * base_y, 1e-13)
    err_d, err_y = _metric(ray.d, d_hat), _metric(ray.y, y_hat)
    ratio_d, ratio_y = err_d / max(base_d, 1e-13 / C_DUALS), err_y / max(base_y, 1e-13 / C_DUALS)
    if kind_code == rref.PRIMAL:
        value_hat = float(p.cc.astype(LD) @ d_hat)
    else:
        value_hat = float(np.asarray(p.b, dtype=LD) @ y_hat)  # the right-hand side of the rows
    print(f"\n{what}: d error {err_d:.3e} (ratio {ratio_d:.3f}), y error {err_y:.3e} (ratio {ratio_y:.3f}), "
          f"value {ray.value!r} (long double {value_hat!r}), violation {ray.violation:.3e}, proven {ray.proven}")
    assert err_d <= tol_d, (err_d, tol_d)
    assert err_y <= tol_y, (err_y, tol_y)
    assert abs(abs(value_hat) - 1.0) <= 1e-9  # the planted reduced cost -1 / the planted x = -1
    assert abs(ray.value - value_hat) <= max(tol_d, tol_y) * max(1.0, abs(value_hat)), (ray.value, value_hat)
    # (value = rhs0 . y over the rows' right-hand side B0 x0: taken over the planted x by position, as
    # it was at first, 64x64x20 infeasible came back with value +22.5 against -1 and proven False)
    assert ray.violation == 0.0 and ray.proven, what
    if m <= 64:  # the STRICT handle forms value from the same right-hand side
        with core.Solver(pl.core_lp(core, p), numerics=core.STRICT) as s:
            assert s.run(0) == status
            strict = s.ray()
        assert (strict.pos, strict.var, strict.proven) == (p.pos, p.var, True), what
        assert abs(strict.value - value_hat) <= 1e-9


# ------------------------------------------------------------------ 5. the other endings of a solve
def test_postsolve_after_refactorised_and_resumed_solves():
    m, ns = 97, 161
    a, b, c = _family(21, 0, m, ns)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    cc = np.asarray(lp.c, dtype=np.float64)
    ends = {}

    def post(s, what):
        assert s.run(0) == "optimal"
        before = s.result(log=False)
        cost = [{int(j): 1.0} for j in before.basis if j < ns]
        cost += [{int(j): 1.0} for j in before.nonbasis[:32]]
        rhs = [{r: 1.0} for r in range(m)]
        pending = s.debug_inverse(0, 0)[1]["neta"]
        du = s.duals()
        r = s.ranging(cost, rhs)
        after = s.result(log=False)
        _same_state(before, after, f"{what}: result() around duals() and ranging()")
        _assert_same_duals(r.duals, du, what)
        exact = pl.exact_duals(a, cc, before.basis, before.nonbasis)
        numpy_ = pl.numpy_duals(a, cc, before.basis, before.nonbasis)
        _check_duals(du, before.basis, before.nonbasis, exact, numpy_, what)
        # the handle's own carried x
        want = pl.reference_sides(a, before.basis, before.nonbasis, before.x, exact[1], cost, rhs)
        yard = pl.reference_sides(a, before.basis, before.nonbasis, before.x, numpy_[1], cost, rhs, exact=False)
        assert sum(want[0].near) + sum(want[1].near) <= pl.SKIP_CAP * (len(cost) + len(rhs))
        for got, w, y, variables, name in ((("cost_lo", "cost_hi", "cost_lo_var", "cost_hi_var"), want[0], yard[0],
                                            before.nonbasis, "cost"),
                                           (("rhs_lo", "rhs_hi", "rhs_lo_var", "rhs_hi_var"), want[1], yard[1],
                                            before.basis, "rhs")):
            res = pl.check_ranges(*(getattr(r, f) for f in got), w, y, variables, f"{what} {name}")
            print(f"\n{what} {name}: error {res['err']:.3e} (ratio {res['ratio']:.3f}), {res['skipped']} skipped")
        ends[what] = (before, pending)
        return before

    with core.Solver(lp, **FAST) as s:
        whole = post(s, "no refactorisation")
    with core.Solver(lp, numerics=core.FAST, refactor_interval=17) as s:
        periodic = post(s, "refactor_interval 17")
    assert periodic.refactors >= 1 and ends["refactor_interval 17"][1] > 0  # etas pending at the optimum
    half = whole.iterations // 2
    assert half >= 10
    with core.Solver(lp, **FAST) as s:
        s.run(half)
        middle = s.result(log=False)
    assert middle.status != "optimal" and half <= middle.iterations < whole.iterations
    with core.Solver(core.resumed_from(lp, middle), **FAST) as s:
        resumed = post(s, "resumed at half")
    assert resumed.iterations == whole.iterations - middle.iterations
    for other in (periodic, resumed):  # (not bit-equal: the compact slot order may depend on history)
        assert other.basis.tolist() == whole.basis.tolist() and other.nonbasis.tolist() == whole.nonbasis.tolist()
