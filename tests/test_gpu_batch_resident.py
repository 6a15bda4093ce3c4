"""A batch kept resident on the GPU between solves (csrc/k_batch_resident.hip, dzg_batch,
core.BatchSolver, dantzig_amd.sessions(resident=True)).

The feature is defined by one sentence: a solve on the handle is, result for result and bit for bit,
the stateless dzg_batch_solve_fast_from on the handle's current data from each LP's last basis.  Every
test here holds the handle to that sentence: the stateless calls (core.solve_batch for STRICT,
core.solve_batch_fast for FAST and AUTO) are the reference, beside the CPU oracle's continuations of
tests/test_batch_from_host.py, whose cases and seeds these are.  FAST runs with near_tie_action =
COUNT, as in tests/test_gpu_batch_fast_from.py; AUTO is the default of both sides."""
import collections

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import core
from tests import batch_resident_walk as walk
from tests import reopt_check as rc
from tests import test_batch_from_host as h
from tests.duals_helpers import assert_bit_equal, assert_same_run

pytestmark = pytest.mark.gpu

STOP = dict(epsilon=1e300)
NUMERICS = {"strict": dict(numerics=core.STRICT),
            "fast": dict(numerics=core.FAST, near_tie_action=core.NEAR_TIE_COUNT),
            "auto": dict(numerics=core.AUTO)}


def _lp(a, b, c):
    return core.CoreLP.from_inequality_form(a, b, c)


def _full(c, m):
    return walk.full_c(c, m)


def _stateless(opts, lps, start=None, **kw):
    if opts.get("numerics") == core.STRICT:
        return core.solve_batch(lps, start=start, **opts, **kw)
    return core.solve_batch_fast(lps, start=start, **opts, **kw)


def assert_same_result(got, want, what):
    """assert_same_run and everything else a CoreResult of a batch carries."""
    assert_same_run(got, want, what)
    assert got.numerics == want.numerics, what
    assert (got.near_ties, got.refactors, got.first_near_tie, got.dense_columns) == \
        (want.near_ties, want.refactors, want.first_near_tie, want.dense_columns), what
    assert_bit_equal([got.max_pivot_error, got.min_margin], [want.max_pivot_error, want.min_margin], what)
    assert (got.margins is None) == (want.margins is None), what
    if want.margins is not None:
        assert_bit_equal(got.margins, want.margins, what + " margins")


def assert_same_results(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert_same_result(g, w, f"{what}, LP {k}")


# ------------------------------------------------------------------ 1. ragged batch, three numerics
@pytest.mark.parametrize("name", list(NUMERICS))
def test_first_and_second_solve_of_a_ragged_batch_are_the_stateless_calls(name):
    opts = NUMERICS[name]
    cases = h.ragged_cases()
    lps, lps2 = [_lp(w.a, w.b, w.c) for w in cases], [_lp(w.a, w.b2, w.c2) for w in cases]
    with core.BatchSolver(lps, **opts) as s:
        first = s.solve()
        want_first = _stateless(opts, lps)
        assert_same_results(first, want_first, f"{name}: first solve")
        s.update_many([(i, w.b2, _full(w.c2, w.a.shape[0]), None) for i, w in enumerate(cases)])
        second = s.solve()
        assert_same_results(second, _stateless(opts, lps2, start=want_first), f"{name}: after the change")
        if name == "strict":
            for w, r in zip(cases, second):
                assert_same_run(r, w.want, f"oracle continuation {w.a.shape}")
    # the restart state itself: with epsilon = 1e300 the first status test ends the solve
    with core.BatchSolver(lps, **opts, **STOP) as s:
        for i, w in enumerate(cases):
            s.set_start(i, (w.first.basis, w.first.nonbasis))
        s.update_many([(i, w.b2, _full(w.c2, w.a.shape[0]), None) for i, w in enumerate(cases)])
        stopped = s.solve()
        start = [(w.first.basis, w.first.nonbasis) for w in cases]
        assert_same_results(stopped, _stateless(opts, lps2, start=start, **STOP), f"{name}: restart state")
        for w, r in zip(cases, stopped):
            what = f"{name}: restart state {w.a.shape}"
            assert (r.status, r.iterations, r.pivots) == ("optimal", 0, []), (what, r.status, r.iterations)
            assert r.basis.tolist() == w.ref.sf.basis.tolist() and r.nonbasis.tolist() == w.ref.sf.nonbasis.tolist()
            assert (r.xbar == 1.0).all() and (r.zbar == 1.0).all(), what
            if name == "strict":
                assert_bit_equal(r.x, w.ref.x, what + " x")
                assert_bit_equal(r.z, w.ref.z, what + " z")


# ------------------------------------------------------------------ 2. a chain of changes
@pytest.mark.parametrize("name", list(NUMERICS))
def test_a_chain_of_changes_leaves_nothing_stale(name):
    opts = NUMERICS[name]
    cases = h.ragged_cases()
    lps = [_lp(w.a, w.b, w.c) for w in cases]
    with core.BatchSolver(lps, **opts) as s:
        got = s.solve()
        prev = _stateless(opts, lps)
        steps = [("b2 only", lambda w: (w.b2, None), lambda w: (w.b2, w.c)),
                 ("c2 only", lambda w: (None, w.c2), lambda w: (w.b2, w.c2)),
                 ("back", lambda w: (w.b, w.c), lambda w: (w.b, w.c)),
                 ("unchanged", None, lambda w: (w.b, w.c))]
        for what, change, now in steps:
            if change is not None:
                s.update_many([(i, change(w)[0], None if change(w)[1] is None else _full(change(w)[1], w.a.shape[0]),
                                None) for i, w in enumerate(cases)])
            got = s.solve()
            want = _stateless(opts, [_lp(w.a, *now(w)) for w in cases], start=prev)
            assert_same_results(got, want, f"{name}: {what}")
            prev = want


# ------------------------------------------------------------------ 3. which
@pytest.mark.parametrize("name", ["strict", "auto"])
def test_solving_a_subset_leaves_the_others_and_their_pending_updates_alone(name):
    opts = NUMERICS[name]
    cases = h.ragged_cases()
    lps, lps2 = [_lp(w.a, w.b, w.c) for w in cases], [_lp(w.a, w.b2, w.c2) for w in cases]
    odd, even = list(range(1, 8, 2)), list(range(0, 8, 2))
    with core.BatchSolver(lps, **opts) as s:
        s.solve()
        first = _stateless(opts, lps)
        s.update_many([(i, w.b2, _full(w.c2, w.a.shape[0]), None) for i, w in enumerate(cases)])
        got_odd = s.solve(which=odd[::-1])                       # (res[k] belongs to which[k])
        want_odd = _stateless(opts, [lps2[i] for i in odd[::-1]], start=[first[i] for i in odd[::-1]])
        assert_same_results(got_odd, want_odd, f"{name}: the odd LPs")
        got_even = s.solve(which=even)
        at_once = _stateless(opts, lps2, start=first)
        assert_same_results(got_even, [at_once[i] for i in even], f"{name}: the even LPs, later")
        # and all of them again: everyone stands at its optimum, with its own data
        again = s.solve()
        assert_same_results(again, _stateless(opts, lps2, start=at_once), f"{name}: all again")


# ------------------------------------------------------------------ 4. more LPs than one launch takes
def test_a_bucket_that_needs_two_launches():
    cases = h.chunk_cases()
    assert len(cases) == 257 and cases[0].a.shape == (65, 8)
    with core.BatchSolver([_lp(w.a, w.b, w.c) for w in cases], numerics=core.STRICT) as s:
        for i, w in enumerate(cases):
            s.set_start(i, (w.first.basis, w.first.nonbasis))
        s.update_many([(i, w.b2, _full(w.c2, 65), None) for i, w in enumerate(cases)])
        got = s.solve()
    for k, (w, g) in enumerate(zip(cases, got)):
        assert_same_run(g, w.want, f"LP {k}")


# ------------------------------------------------------------------ 5. a singular start
@pytest.mark.parametrize("name", list(NUMERICS))
def test_a_singular_start_ends_singular_and_the_next_solve_is_cold(name):
    opts = NUMERICS[name]
    ragged = {w.a.shape: w for w in h.ragged_cases()}
    left, right = ragged[(16, 24)], ragged[(17, 24)]
    for a, basis, nonbasis in h.singular_cases():
        lps = [_lp(left.a, left.b2, left.c2), _lp(a, np.ones(a.shape[0]), np.ones(a.shape[1])),
               _lp(right.a, right.b2, right.c2)]
        start = [(left.first.basis, left.first.nonbasis), (basis, nonbasis), (right.first.basis, right.first.nonbasis)]
        with core.BatchSolver(lps, **opts) as s:
            for i, st in enumerate(start):
                s.set_start(i, st)
            got = s.solve()
            what = f"{name}: duplicated column {a.shape}"
            assert (got[1].status, got[1].iterations, got[1].pivots) == ("singular", 0, []), (what, got[1].status)
            assert got[1].basis.tolist() == basis.tolist() and got[1].nonbasis.tolist() == nonbasis.tolist(), what
            assert_same_results(got, _stateless(opts, lps, start=start), what)
            for k in (0, 2):
                assert_same_result(got[k], _stateless(opts, [lps[k]], start=[start[k]])[0], f"{what}: neighbour {k}")
            # its next solve is cold; set_start(None) makes a healthy LP cold as well
            s.set_start(2, None)
            again = s.solve()
            cold = _stateless(opts, lps)
            assert_same_result(again[1], cold[1], what + ": cold after the singular end")
            assert_same_result(again[2], cold[2], what + ": set_start(None)")
            assert_same_result(again[0], _stateless(opts, [lps[0]], start=[got[0]])[0], what + ": warm neighbour")


# ------------------------------------------------------------------ 6. AUTO hand-over on the modelling surface
def test_resident_sessions_are_the_stateless_sessions_over_three_calls():
    data = [core.gen_dense_lp(seed=seed, m=m, n_struct=ns) for seed, m, ns in h.SESSION_SEEDS]
    models = [h._dense_model(a, b, c) for a, b, c in data]
    moved = [{p.constraints[i]: float(v) for i, v in enumerate(rc.moved(seed + 1000, b, c)[0])}
             for p, (seed, _, _), (_, b, c) in zip(models, h.SESSION_SEEDS, data)]
    back = [{p.constraints[i]: float(v) for i, v in enumerate(b)} for p, (_, b, _) in zip(models, data)]
    with dz.sessions(models, fast=True, resident=True) as res:
        ref = dz.sessions(models, fast=True)
        for call, rhs in enumerate((None, moved, back)):
            got, want = res.solve(rhs=rhs), ref.solve(rhs=rhs)
            for k, (g, w) in enumerate(zip(got, want)):
                assert g.objective_value == w.objective_value, (call, k)
                assert g._solution._values == w._solution._values, (call, k)
            for k, (a, b) in enumerate(zip(res._models, ref._models)):
                assert_same_result(a.last, b.last, f"call {call}, model {k}")
        assert res.pivots == ref.pivots and res.cold == ref.cold == [6, 0, 0]
        assert res.strict_fallbacks == ref.strict_fallbacks
        assert res.rebuilds == 0
    print(f"pivots per call: {ref.pivots}; handed to STRICT per call: {ref.strict_fallbacks}")
    assert sum(ref.strict_fallbacks) >= 1, "the stateless side showed no fallback: pick other models"


# ------------------------------------------------------------------ 7. failing calls change nothing
def test_failing_calls_change_nothing_and_two_handles_do_not_disturb_each_other():
    cases = h.ragged_cases()[2:6]
    lps, lps2 = [_lp(w.a, w.b, w.c) for w in cases], [_lp(w.a, w.b2, w.c2) for w in cases]
    opts = NUMERICS["auto"]
    first = _stateless(opts, lps)
    s, other = core.BatchSolver(lps, **opts), core.BatchSolver(lps[::-1], **opts)
    try:
        s.solve()
        other.solve()
        good = [(i, w.b2, _full(w.c2, w.a.shape[0]), None) for i, w in enumerate(cases)]
        nan = np.array(cases[1].b2)
        nan[3] = np.nan
        for bad, needle in (([good[0], (1, nan, None, None)], r"b\[3\]"),
                            ([good[0], good[1], good[0]], "twice"),
                            ([good[0], (4, cases[0].b2, None, None)], "out of range"),
                            ([good[0], (1, None, None, float("inf"))], "constant")):
            with pytest.raises(ValueError, match=needle):
                s.update_many(bad)
        with pytest.raises(ValueError, match="twice"):
            s.solve(which=[0, 0])
        with pytest.raises(ValueError, match="out of range"):
            s.solve(which=[0, 4])
        assert_same_results(s.solve(), _stateless(opts, lps, start=first), "after the refused calls")
        s.update_many(good)
        want = _stateless(opts, lps2, start=first)
        assert_same_results(s.solve(), want, "after the good update")
        # the other handle saw none of it; closing one leaves the other usable
        assert_same_results(other.solve(), _stateless(opts, lps[::-1], start=first[::-1]), "the other handle")
        other.close()
        assert_same_results(s.solve(), _stateless(opts, lps2, start=want), "after the other closed")
    finally:
        s.close()
        other.close()
    with pytest.raises(ValueError, match="closed"):
        s.solve()


# ------------------------------------------------------------------ 8. traffic
def traffic_bound(shapes, changed, listed):
    """(the cap on a solve's host-to-device bytes, the bytes of the matrices): 8 bytes per entry of the
    changed arrays, 512 per listed LP for its control block and list entries, 4096 for the call."""
    return (8 * sum(shapes[i][0] + shapes[i][0] + shapes[i][1] for i in changed) + 512 * listed + 4096,
            8 * sum(m * ns for m, ns in shapes))


def test_a_solve_uploads_the_changed_arrays_and_little_else():
    cases = h.ragged_cases()
    shapes = [w.a.shape for w in cases]
    changed = [1, 4, 6]
    cap, matrices = traffic_bound(shapes, changed, len(cases))
    assert cap < matrices, (cap, matrices)
    with core.BatchSolver([_lp(w.a, w.b, w.c) for w in cases]) as s:
        s.solve()
        s.update_many([(i, cases[i].b2, None, None) for i in changed])
        s.solve()
        up, down, ms = s.traffic()
    print(f"host to device {up} B (cap {cap} B, matrices {matrices} B), device to host {down} B, "
          f"stage + restart {ms:.3f} ms")
    assert 0 < up <= cap < matrices
    assert down > 0 and ms > 0.0


# ------------------------------------------------------------------ 9. random walk
@pytest.mark.parametrize("name,seed", [("strict", 11), ("auto", 12)])
def test_random_walk_against_the_stateless_calls(name, seed):
    opts = NUMERICS[name]
    data, ops = walk.recipe(seed, count=12, steps=30)
    assert max(a.shape[0] for a, _, _ in data) <= 33 and len(data) == 12
    mirror = walk.Mirror(data, **opts)
    seen = collections.Counter()
    with core.BatchSolver(mirror.lps(), **opts) as s:
        for step, op in enumerate(ops):
            seen[op.kind] += 1
            if op.call == "solve":
                got, want = s.solve(*op.args), mirror.solve(*op.args)
                assert_same_results(got, want, f"{name}, seed {seed}, step {step} ({op.kind})")
            else:
                getattr(s, op.call)(*op.args)
                getattr(mirror, op.call)(*op.args)
    print(f"{name}, seed {seed}: {dict(seen)}")
    assert seen["subset"] >= 2 and seen["solve all"] >= 2 and sum(seen[k] for k in ("b", "c", "both")) >= 3
