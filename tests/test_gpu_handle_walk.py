"""Live handles walked through random reoptimize / extend / remove / run sequences beside a host mirror
(tests/handle_walk.py; tests/test_handle_walk_host.py checks the mirror and the walks on the CPU).

One core.Solver per walk is driven through the recipe and compared with the mirror after EVERY step.

STRICT: dims, basis, nonbasis, status, iterations and the pivot log (kind, entering, leaving) equal the
mirror's; x, z, xbar, zbar, the objective and every mu bit for bit.  After every extend and remove
debug_matrix() and, where it is kept, debug_matrix_rows() are the mirror's `a` bit for bit with the sign
of zero included (every added block carries a -0.0); the maps of a remove are core.reduced_lp's and
removable() the mirror's masks before it.  At an optimal end duals() is duals_reference.core_duals bit
for bit, at the other ends ray() has the kind of the verdict and is proven.

FAST (refactor_interval=-1, near ties counted): lists, dims, maps, masks and both matrix copies as
above.  After every restart xbar = zbar = 1, state_drift == 0.0 and D (reopt_check.restart_drift against
the long-double state of the basis) <= reopt_check.C_RESTART; after every stop D against the long-double
state reached from the handle's last restart state <= state_check.C_STATE_SHORT; at every end the
mirror's verdict, its objective to 1e-9, the certificate or a proven ray.  A walk without a near tie has
the mirror's pivot log throughout; at most one walk may report one.

Worst D per walk on an MI355X (pytest -s prints them): WORST_D_OBSERVED below, (restart, carried); no
walk reported a near tie.  A walk that runs on with the planted column of -1 or the planted parallel pair
of rows can: FAST then decides exact ties its own way (60x70 seeds 4, 8 and 52 of the recipe do; seed 8
ends `singular` where the mirror says infeasible).  Such seeds are not used.
"""
import numpy as np
import pytest

from dantzig_amd import core
from tests import duals_reference as dref
from tests import extend_check as ec
from tests import handle_walk as hw
from tests import reopt_check as rc
from tests import state_check as sc
from tests.duals_helpers import assert_bit_equal, bits

pytestmark = pytest.mark.gpu

STRICT_OPTS = dict(numerics=core.STRICT)
FAST_OPTS = dict(numerics=core.FAST, refactor_interval=-1, near_tie_action=core.NEAR_TIE_COUNT)
TOL = 1e-9          # test_gpu_extend.py's
TERMINAL = ("optimal", "unbounded", "infeasible")
RAY_KIND = {"unbounded": "primal", "infeasible": "farkas"}

# walk -> (worst restart D, worst carried D) as an MI355X showed them; the bounds are C_RESTART = 3.5e-12
# and C_STATE_SHORT = 5e-11
WORST_D_OBSERVED = {"14x20 seed 1": (4.918e-16, 4.858e-15), "14x20 seed 2": (1.549e-15, 7.759e-15),
                    "14x20 seed 55": (1.399e-16, 1.710e-15), "14x20 seed 119": (2.351e-16, 1.693e-15),
                    "60x70 seed 59": (3.273e-14, 1.543e-12), "60x70 seed 59 seven launches": (3.273e-14, 1.543e-12)}

_copies = {"strict": 0, "fast": 0}     # comparisons of the row-major copy
_tied = set()                          # FAST walks that reported a near tie


def _same_bits(got, want, what):
    """Bit for bit with the sign of zero included."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, what
    same = bits(got) == bits(want)
    assert same.all(), f"{what}: {np.count_nonzero(~same)} of {same.size} values differ"


def _same_log(got, want, what, upto=None):
    got, want = got[:upto], want[:upto]
    assert [p[:3] for p in got] == [p[:3] for p in want], what + " pivot log"


def _matrices(s, mir, res, numerics, what):
    _same_bits(s.debug_matrix(), mir.lp.a, what + " debug_matrix")
    at = s.debug_matrix_rows()
    assert (at is not None) == bool(res.price_rows_copy), what
    if at is not None:
        _copies[numerics] += 1
        _same_bits(at, mir.lp.a, what + " debug_matrix_rows")


def _before(s, mir, op, what):
    if op.call == "remove":
        got, want = s.removable(), mir.removable()
        assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist(), what + " removable"


def _maps(op, got, want, what):
    if op.call == "remove":
        assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist(), what + " maps"
    else:
        assert got == want, (what, got, want)       # run: the status; the others: None


def check_strict(s, mir, op, got, want, what):
    """Everything a STRICT handle shows after `op`, against the mirror."""
    _maps(op, got, want, what)
    assert s.dims() == mir.dims(), what
    res = s.result()
    assert res.basis.tolist() == mir.basis.tolist() and res.nonbasis.tolist() == mir.nonbasis.tolist(), what
    assert (res.status, res.iterations) == (mir.status, mir.iterations), (what, res.status, res.iterations)
    for name in ("x", "z", "xbar", "zbar"):
        assert_bit_equal(getattr(res, name), getattr(mir, name), f"{what} {name}")
    assert_bit_equal([res.objective], [mir.objective], what + " objective")
    assert len(res.pivots) == len(mir.pivots), what
    _same_log(res.pivots, mir.pivots, what)
    assert_bit_equal([p[3] for p in res.pivots], [p[3] for p in mir.pivots], what + " mu")
    if op.call in ("extend", "remove"):
        _matrices(s, mir, res, "strict", what)
    if op.call == "run" and mir.status == "optimal":
        ref = dref.core_duals(mir.stdform(), mir, rhs0=mir.lp.x)
        du = s.duals()
        assert du.source == "fresh", what
        assert_bit_equal(du.y, ref.y, what + " y")
        assert_bit_equal(du.d, ref.d, what + " d")
        assert_bit_equal([du.dual_obj, du.primal_obj], [ref.dual_obj, mir.objective], what + " objectives")
        assert_bit_equal([du.primal_infeas, du.dual_infeas, du.z_diff],
                         [ref.primal_infeas, ref.dual_infeas, ref.z_diff], what + " scalars")
    elif op.call == "run" and mir.status in RAY_KIND:
        ray = s.ray()
        assert ray.kind == RAY_KIND[mir.status] and ray.proven, (what, ray.kind, ray.proven, ray.violation)


def _strict_walk(a, b, c, ops, name, **opts):
    mir = hw.Mirror(a, b, c, max_iter=opts.get("max_iter", 0))
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), **STRICT_OPTS, **opts) as s:
        for step, op in enumerate(ops):
            what = f"{name} step {step} {op.kind}"
            _before(s, mir, op, what)
            got, want = hw.apply(s, op), hw.apply(mir, op)
            check_strict(s, mir, op, got, want, what)
        return mir, s.result()


@pytest.mark.parametrize("walk", hw.SMALL, ids=lambda w: w.name)
def test_strict_handle_is_the_mirror_after_every_step(walk):
    a, b, c, ops = hw.recipe_of(walk)
    mir, res = _strict_walk(a, b, c, ops, walk.name)
    assert res.status == "optimal" and res.numerics == "strict"
    print(f"{walk.name}: {len(ops)} steps, {res.iterations} pivots, {mir.runs} runs, ends {mir.dims()}")


# ---------------------------------------------------------------------- FAST
def _fast_walk(walk, **opts):
    a, b, c, ops = hw.recipe_of(walk)
    mir = hw.Mirror(a, b, c)
    worst = {"restart": 0.0, "carried": 0.0}
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), **FAST_OPTS, **opts) as s:
        begun = mir.lp                  # the state the handle's pivots began from: its own last restart state
        for step, op in enumerate(ops):
            what = f"{walk.name} step {step} {op.kind}"
            tied = walk.name in _tied
            if not tied:
                _before(s, mir, op, what)
            got, want = hw.apply(s, op), hw.apply(mir, op)
            res = s.result()
            if res.near_ties > 0 and not tied:
                print(f"{what}: near tie at pivot {res.first_near_tie}")
                _tied.add(walk.name)
                tied = True
            assert len(_tied) <= 1, ("more than one walk reports a near tie", _tied)
            assert res.numerics == "fast", what
            assert s.dims() == mir.dims(), what
            assert res.iterations == len(res.pivots), what
            if not tied:
                _maps(op, got, want, what)
                assert res.basis.tolist() == mir.basis.tolist() and res.nonbasis.tolist() == mir.nonbasis.tolist(), what
                assert (res.status, res.iterations) == (mir.status, mir.iterations), (what, res.status)
                _same_log(res.pivots, mir.pivots, what)
            else:
                _same_log(res.pivots, mir.pivots, what, upto=res.first_near_tie)
            if op.call in ("extend", "remove"):
                _matrices(s, mir, res, "fast", what)
            if op.call != "run":
                assert res.status == "running", what
                assert (res.xbar == 1.0).all() and (res.zbar == 1.0).all(), what
                assert res.state_drift == 0.0, what
                ex = hw.exact_restart(mir, res.basis, res.nonbasis)
                assert max(ex.err["x"], ex.err["z"]) * 1e2 <= rc.C_RESTART, (what, ex.err)
                if tied:                # its own basis: the host's double-precision restart there is the yardstick
                    own = hw.host_restart(mir, res.basis, res.nonbasis)
                    assert rc.restart_drift(ex, own)["D"] <= rc.C_RESTART / 10, (what, "the handle's own basis")
                d = rc.restart_drift(ex, res)
                worst["restart"] = max(worst["restart"], d["D"])
                assert d["D"] <= rc.C_RESTART, (what, d)
                begun = hw.snapshot(res)
            else:
                lp = mir.lp
                d = sc.exact_state(lp.a, lp.n_struct, begun, res.basis, res.nonbasis, lp.var_col).drift(res)
                worst["carried"] = max(worst["carried"], d["D"])
                assert d["D"] <= sc.C_STATE_SHORT, (what, d)
                assert res.status == mir.status or (tied and mir.status == "iter_limit"), (what, res.status, mir.status)
                if res.status in TERMINAL:
                    assert res.status == mir.status, (what, res.status, mir.status)
                    if res.status == "optimal":
                        scale = max(1.0, abs(mir.objective))
                        assert abs(res.objective - mir.objective) <= TOL * scale, (what, res.objective, mir.objective)
                        ec.check_certificate(mir.lp, res, TOL)
                    else:
                        ray = s.ray()
                        assert ray.kind == RAY_KIND[res.status] and ray.proven, (what, ray.kind, ray.violation)
        res = s.result()
    assert res.status == "optimal"
    print(f"{walk.name} {opts}: {res.iterations} pivots, near_ties {res.near_ties}, worst restart D "
          f"{worst['restart']:.3e}, worst carried D {worst['carried']:.3e}")
    return res, worst


@pytest.mark.parametrize("walk", hw.WALKS, ids=lambda w: w.name)
def test_fast_handle_follows_the_mirror_after_every_step(walk):
    _fast_walk(walk)


def test_fast_60x70_walk_with_seven_launches():
    _fast_walk(hw.LARGE, seven_launches=1)


def test_the_row_major_copy_was_compared():
    """(runs after the walks above; on its own it walks once first)  The row-wise pricing pass and its copy
    of the matrix belong to FAST; a STRICT handle keeps none, which _matrices asserts at every step."""
    if not _copies["fast"]:
        _fast_walk(hw.LARGE)
    assert _copies["fast"] >= 1 and _copies["strict"] == 0, _copies


# ---------------------------------------------------------------------- opts.max_iter bounds the total
def test_max_iter_bounds_the_total_across_the_calls():
    a, b, c, ops, total = hw.capped(hw.CAPPED)
    mir, res = _strict_walk(a, b, c, ops, "max_iter", max_iter=total)
    assert (mir.status, mir.iterations) == ("iter_limit", total)
    assert (res.status, res.iterations) == ("iter_limit", total)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), **FAST_OPTS, max_iter=total) as s:
        for op in ops:
            hw.apply(s, op)
        res = s.result()
    assert (res.status, res.iterations) == ("iter_limit", total), (res.status, res.iterations)
