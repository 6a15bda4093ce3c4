"""The calls on a finished solver (duals(), ranging(), ray()) give the same bits whatever was called
before them on the same handle: each works on scratch buffers that the others fill too, and none may
depend on what another left there.  Two handles built from one LP take different call sequences and
must agree bit for bit; ray() called twice must repeat itself, its second call starting from the
buffers its first one filled."""
import dataclasses

import numpy as np
import pytest

from dantzig_amd import core
from tests.duals_helpers import family
from tests.rays_helpers import infeasible_lp, unbounded_lp

pytestmark = pytest.mark.gpu

STRICT_OPTS = dict(numerics=core.STRICT)
FAST_OPTS = dict(numerics=core.FAST, refactor_interval=-1)


def _assert_same_bits(got, want, what):
    """Every field of two result dataclasses: arrays of doubles by their bits, the rest by value."""
    assert type(got) is type(want), what
    for f in dataclasses.fields(got):
        g, w = getattr(got, f.name), getattr(want, f.name)
        if dataclasses.is_dataclass(g):
            _assert_same_bits(g, w, f"{what}.{f.name}")
        elif isinstance(g, np.ndarray) and g.dtype == np.float64:
            assert w.dtype == np.float64 and g.shape == w.shape, f"{what}.{f.name}"
            assert np.array_equal(g.view(np.int64), w.view(np.int64)), f"{what}.{f.name} differs in its bits"
        elif isinstance(g, np.ndarray):
            assert g.dtype == w.dtype and np.array_equal(g, w), f"{what}.{f.name} differs"
        elif isinstance(g, float):
            assert np.float64(g).view(np.int64) == np.float64(w).view(np.int64), f"{what}.{f.name}: {g!r} != {w!r}"
        else:
            assert g == w, f"{what}.{f.name}: {g!r} != {w!r}"


# 24 x 40 (STRICT) and 97 x 161 (FAST): an odd number of structural basics and a single-wave tail, the
# shapes of tests/test_gpu_reopt.py and tests/test_gpu_duals.py
@pytest.mark.parametrize("opts,seed,m,ns", [(STRICT_OPTS, 31, 24, 40), (FAST_OPTS, 21, 97, 161)],
                         ids=["strict-24x40", "fast-97x161"])
def test_ranging_and_duals_do_not_depend_on_earlier_calls(opts, seed, m, ns):
    a, b, c = family(seed, 0, m, ns)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    what = f"{m} x {ns}"
    with core.Solver(lp, **opts) as sa, core.Solver(lp, **opts) as sb:
        assert sa.run(0) == "optimal" and sb.run(0) == "optimal", what
        rg_a = sa.ranging()
        sb.duals()
        sb.duals()
        rg_b = sb.ranging()
        du_b = sb.duals()
        res_a, res_b = sa.result(log=False), sb.result(log=False)
    assert rg_a.duals is not None and rg_b.duals is not None and rg_a.duals.source == "fresh", what
    assert len(rg_a.cost_lo) == m + ns and len(rg_a.rhs_lo) == m, what
    _assert_same_bits(rg_b, rg_a, what + ": ranging() after duals(), duals() against ranging() alone")
    _assert_same_bits(du_b, rg_a.duals, what + ": duals() after ranging() against the duals of ranging() alone")
    assert res_a.status == res_b.status == "optimal", what
    assert res_a.iterations == res_b.iterations > 0, what


# 8 x 17 (STRICT) and 97 x 161 (FAST), the two families of tests/rays_helpers.py
@pytest.mark.parametrize("make,status", [(unbounded_lp, "unbounded"), (infeasible_lp, "infeasible")],
                         ids=["unbounded", "infeasible"])
@pytest.mark.parametrize("opts,m,ns", [(STRICT_OPTS, 8, 17), (FAST_OPTS, 97, 161)], ids=["strict-8x17", "fast-97x161"])
def test_a_second_ray_is_the_first(opts, m, ns, make, status):
    a, b, c = make(0, m, ns)
    what = f"{m} x {ns} {status}"
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), **opts) as s:
        assert s.run(0) == status, what
        before = s.result(log=False)
        first = s.ray()
        second = s.ray()
        after = s.result(log=False)
    assert first.kind == ("primal" if status == "unbounded" else "farkas"), what
    _assert_same_bits(second, first, what + ": the second ray() against the first")
    assert after.status == before.status == status and after.iterations == before.iterations, what
