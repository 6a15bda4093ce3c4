"""FAST batches re-optimised from their last bases on the GPU (csrc/k_batch_fast.hip,
k_batch_fast_restart, dzg_batch_solve_fast_from, core.solve_batch_fast(start=...),
dantzig_amd.sessions(fast=True)).

The restart state of a warm LP lies within C_FAST_RESTART of the long-double state its start basis
defines for the changed data (tests/batch_fast_from_reference.py sets the bound on the CPU), in every
bucket and at every block size, and the pivots that follow are the STRICT reference's wherever FAST
met no near tie; cold and warm LPs mix in one call without touching each other, bit for bit; a
singular start ends singular without a pivot; AUTO hands what FAST gave up on to the STRICT batch
from the same start.  The cases are tests/test_batch_from_host.py's; tests/test_batch_fast_from_host.py
checks on the CPU that the oracle continued from the transcribed restart state stays on the
reference's path in all of them.

FAST runs with near_tie_action = COUNT unless a test says otherwise.  The restart state is read
after a stop before the first pivot (epsilon = 1e300), as in tests/test_gpu_batch_from.py."""
import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import core
from tests import batch_fast_from_reference as ffr
from tests import reopt_check as rc
from tests import state_check as sc
from tests import test_batch_from_host as h
from tests.duals_helpers import assert_bit_equal, assert_same_run
from tests.lp_families import log3, make_lp

pytestmark = pytest.mark.gpu

FAST = dict(numerics=core.FAST, near_tie_action=core.NEAR_TIE_COUNT)
STOP = dict(epsilon=1e300)


def _starts(cases):
    return [(w.basis, w.nonbasis) for w in cases]


def assert_same_fast_run(got, want, what):
    """assert_same_run and what a FAST result carries beside it."""
    assert_same_run(got, want, what)
    assert got.numerics == want.numerics == "fast", what
    assert (got.near_ties, got.refactors, got.first_near_tie) == (want.near_ties, want.refactors,
                                                                 want.first_near_tie), what
    assert_bit_equal([got.max_pivot_error, got.min_margin], [want.max_pivot_error, want.min_margin], what)
    assert_bit_equal(got.margins, want.margins, what + " margins")


def assert_follows(g, want, what):
    assert g.status == want.status, (what, g.status, want.status)
    assert log3(g.pivots) == log3(want.pivots), f"{what}: pivot sequence differs from the reference's"
    assert g.basis.tolist() == want.basis.tolist() and g.nonbasis.tolist() == want.nonbasis.tolist(), what
    assert abs(g.objective - want.objective) <= 1e-9 * max(1.0, abs(want.objective)), what


def _follow_unless_flagged(cases, got):
    """Every LP without a near tie follows its reference; at most one in eight is flagged."""
    flagged = 0
    for w, g in zip(cases, got):
        assert g.numerics == "fast" and g.iterations >= 1, w.name
        assert g.margins is not None and len(g.margins) == g.iterations, w.name
        if g.near_ties > 0:
            flagged += 1
            continue
        assert_follows(g, w.want, w.name)
    assert 8 * flagged <= len(cases), f"{flagged} of {len(cases)} LPs had a near tie"
    return flagged


@pytest.fixture(scope="module")
def ragged():
    return [ffr.of_case(w) for w in h.ragged_cases()]


# ------------------------------------------------------------------ 1. restart state and continuation
def test_restart_state_and_continuation_in_every_bucket_and_at_the_edge_starts(ragged):
    cases = ragged + ffr.edge_cases()
    assert [w.a.shape for w in ragged] == [(1, 3), (2, 3), (16, 24), (17, 24), (33, 40), (64, 40), (65, 72), (128, 40)]
    assert [w.name for w in cases[8:]] == ["all-slack start", "all-structural start", "KAT non_standard_variables",
                                          "permuted nonbasis"]
    assert (cases[9].basis < cases[9].ns).all() and cases[10].var_col is not None
    lps, start = [w.lp for w in cases], _starts(cases)
    stopped = core.solve_batch_fast(lps, start=start, **FAST, **STOP)
    full = core.solve_batch_fast(lps, start=start, **FAST)
    for w, s in zip(cases, stopped):
        assert (s.status, s.iterations, s.pivots) == ("optimal", 0, []), (w.name, s.status, s.iterations)
        assert s.basis.tolist() == w.basis.tolist() and s.nonbasis.tolist() == w.nonbasis.tolist(), w.name
        assert (s.xbar == 1.0).all() and (s.zbar == 1.0).all(), w.name
        d = rc.restart_drift(w.exact(), s)
        print(f"{w.name}: restart D = {d['D']:.3e} (x {d['x']:.3e}, z {d['z']:.3e}), refactors {s.refactors}")
        assert d["D"] <= ffr.C_FAST_RESTART, (w.name, d)
    slack = cases[8]
    assert_bit_equal(stopped[8].x, slack.b2, "all-slack start x")
    assert_bit_equal(stopped[8].z, -slack.c2[slack.nonbasis], "all-slack start z")
    assert stopped[8].refactors == 0
    assert_same_fast_run(full[8], core.solve_batch_fast([slack.lp], **FAST)[0], "all-slack start = cold")
    for w, g in zip(cases, full):
        print(f"{w.name}: {g.status} {g.iterations} pivots (reference {w.want.iterations}), near_ties {g.near_ties}, "
              f"refactors {g.refactors}")
    _follow_unless_flagged(cases, full)


# ------------------------------------------------------------------ 2. cold and warm in one call
def test_cold_and_warm_lps_mix_in_one_call_and_do_not_notice_their_place(ragged):
    by_shape = {w.a.shape: w for w in ragged}
    cases = [ffr.of_case(w) for w in h.mixed_cases()] + [by_shape[(65, 72)], by_shape[(2, 3)], by_shape[(33, 40)]]
    lps = [w.lp for w in cases]
    start = [None if k % 2 == 0 else (w.basis, w.nonbasis) for k, w in enumerate(cases)]
    got = core.solve_batch_fast(lps, start=start, **FAST)
    cold = core.solve_batch_fast(lps, **FAST)
    back = core.solve_batch_fast(lps[::-1], start=start[::-1], **FAST)[::-1]
    for k, (w, g) in enumerate(zip(cases, got)):
        what = f"LP {k} {w.name}"
        if start[k] is None:
            assert_same_fast_run(g, cold[k], what + " cold")
        else:
            assert g.refactors >= 1, what
            alone = core.solve_batch_fast([lps[k]], start=[start[k]], **FAST)[0]
            assert_same_fast_run(g, alone, what + " warm, alone")
        assert_same_fast_run(back[k], g, what + " in the reversed batch")
    for k, (g, r) in enumerate(zip(core.solve_batch_fast(lps, start=[None] * len(lps), **FAST), cold)):
        assert_same_fast_run(g, r, f"LP {k} with start = None")


# ------------------------------------------------------------------ 3. more LPs than one launch takes
def test_a_bucket_that_needs_two_restart_launches():
    cases = [ffr.of_case(w) for w in h.chunk_cases()]
    assert len(cases) == 257 and cases[0].a.shape == (65, 8)
    got = core.solve_batch_fast([w.lp for w in cases], start=_starts(cases), **FAST)
    flagged = _follow_unless_flagged(cases, got)
    print(f"257 x 65x8: {sum(g.iterations for g in got)} pivots warm, {flagged} flagged for a near tie")


# ------------------------------------------------------------------ 4. singular starts
def test_singular_starts_end_singular_in_fast_and_go_to_strict_under_auto(ragged):
    by_shape = {w.a.shape: w for w in ragged}
    left, right = by_shape[(16, 24)], by_shape[(17, 24)]
    sing = h.singular_cases()
    lps = [left.lp] + [core.CoreLP.from_inequality_form(a, np.ones(a.shape[0]), np.ones(a.shape[1]))
                       for a, _, _ in sing] + [right.lp]
    start = [(left.basis, left.nonbasis)] + [(b, nb) for _, b, nb in sing] + [(right.basis, right.nonbasis)]
    got = core.solve_batch_fast(lps, start=start, **FAST)
    for (a, basis, nonbasis), g in zip(sing, got[1:3]):
        what = f"duplicated column {a.shape}"
        assert (g.status, g.iterations, g.pivots) == ("singular", 0, []), (what, g.status, g.iterations)
        assert g.basis.tolist() == basis.tolist() and g.nonbasis.tolist() == nonbasis.tolist(), what
        assert g.numerics == "fast"
    for k in (0, 3):
        assert_same_fast_run(got[k], core.solve_batch_fast([lps[k]], start=[start[k]], **FAST)[0], f"neighbour {k}")
    auto = core.solve_batch_fast(lps, start=start)
    strict = core.solve_batch(lps, start=start)
    for k in (1, 2):
        assert auto[k].numerics == "strict" and auto[k].status == "singular", k
        assert_same_run(auto[k], strict[k], f"LP {k} under AUTO")
    # a result that ended singular is no start: the next call solves that LP cold
    again = core.solve_batch_fast(lps, start=got, **FAST)
    for k in (1, 2):
        assert_same_fast_run(again[k], core.solve_batch_fast([lps[k]], **FAST)[0], f"LP {k} after its singular end")


# ------------------------------------------------------------------ 5. AUTO hands over warm
AUTO_SEEDS = [9400 + i for i in range(16)]


def test_auto_hands_the_flagged_lps_to_strict_from_the_same_start():
    """Seeds 9400..9415 (the kind-2 seeds of test_gpu_batch_fast.py), b moved by integers in -1..2
    drawn from default_rng(5): on an MI355X 15 of the 16 were re-solved in STRICT (all but 9405)."""
    data = [make_lp(seed, 2, 16, 32) for seed in AUTO_SEEDS]
    first = core.solve_batch([core.CoreLP.from_inequality_form(*d) for d in data], max_iter=4096)
    rng = np.random.default_rng(5)
    lps = [core.CoreLP.from_inequality_form(a, b + rng.integers(-1, 3, len(b)).astype(np.float64), c)
           for a, b, c in data]
    auto = core.solve_batch_fast(lps, start=first, max_iter=4096)
    strict = core.solve_batch(lps, start=first, max_iter=4096)
    redo = [k for k, r in enumerate(auto) if r.numerics == "strict"]
    print(f"AUTO, warm: {len(redo)} of {len(lps)} re-solved in STRICT ({[AUTO_SEEDS[k] for k in redo]}); "
          f"pivots {[r.iterations for r in auto]}")
    for k, (g, s) in enumerate(zip(auto, strict)):
        if g.numerics == "fast":
            assert g.near_ties == 0 and g.status not in ("near_tie", "singular", "panic"), (k, g.status)
        else:
            assert_same_run(g, s, f"LP {k} (seed {AUTO_SEEDS[k]})")
    assert redo, "no LP was handed to STRICT: pick other seeds"


# ------------------------------------------------------------------ 6. launch and rebuild boundaries
def test_launch_and_rebuild_boundaries_after_a_restart(ragged):
    by_shape = {w.a.shape: w for w in ragged}
    cases = [by_shape[(33, 40)], by_shape[(65, 72)]]
    lps, start = [w.lp for w in cases], _starts(cases)
    often = core.solve_batch_fast(lps, start=start, pivots_per_launch=3, refactor_every=2, **FAST)
    default = core.solve_batch_fast(lps, start=start, **FAST)
    for w, g, d in zip(cases, often, default):
        print(f"{w.name}: {g.iterations} pivots, {g.refactors} refactors ({d.refactors} by default), "
              f"near_ties {g.near_ties}")
        if g.near_ties == 0:
            assert_follows(g, w.want, w.name)
        assert g.refactors > d.refactors, w.name


# ------------------------------------------------------------------ 7. the carried state
def test_carried_state_after_a_warm_solve_stays_within_the_short_solve_bound(ragged):
    """D of tests/state_check.py on the final basis, under both definitions a warm solve has: x and z
    against the state the final basis defines for the changed LP (its slack start), and all four
    vectors against the state it defines for the restart state the pivots began from (xbar = zbar =
    1 at the start basis, which is where a warm LP's xbar and zbar are defined)."""
    w = {c.a.shape: c for c in ragged}[(128, 40)]
    s = core.solve_batch_fast([w.lp], start=_starts([w]), **FAST, **STOP)[0]
    g = core.solve_batch_fast([w.lp], start=_starts([w]), **FAST)[0]
    assert g.status == "optimal" and g.iterations >= 1
    lp = rc.restart_drift(w.exact(g.basis, g.nonbasis), g)
    begun = dict(basis=w.basis, nonbasis=w.nonbasis, x=s.x, xbar=None, z=s.z, zbar=None)
    d = sc.exact_state(w.a, w.ns, begun, g.basis, g.nonbasis).drift(g)
    print(f"128 x 40: {g.iterations} pivots from the restart; against the changed LP D = {lp['D']:.3e} "
          f"(x {lp['x']:.3e}, z {lp['z']:.3e}); against the restart state D = {d['D']:.3e} (x {d['x']:.3e}, "
          f"xbar {d['xbar']:.3e}, z {d['z']:.3e}, zbar {d['zbar']:.3e})")
    assert lp["D"] <= sc.C_STATE_SHORT, lp
    assert d["D"] <= sc.C_STATE_SHORT, d


# ------------------------------------------------------------------ 8. the modelling surface
def test_sessions_fast_agrees_with_sessions_over_three_calls():
    data = [core.gen_dense_lp(seed=seed, m=m, n_struct=ns) for seed, m, ns in h.SESSION_SEEDS]
    models = [h._dense_model(a, b, c) for a, b, c in data]
    moved = [{p.constraints[i]: float(v) for i, v in enumerate(rc.moved(seed + 1000, b, c)[0])}
             for p, (seed, _, _), (_, b, c) in zip(models, h.SESSION_SEEDS, data)]
    back = [{p.constraints[i]: float(v) for i, v in enumerate(b)} for p, (_, b, _) in zip(models, data)]
    fast, ref = dz.sessions(models, fast=True), dz.sessions(models)
    for call, rhs in enumerate((None, moved, back)):
        got, want = fast.solve(rhs=rhs), ref.solve(rhs=rhs)
        strict = [st.last.numerics == "strict" for st in fast._models]
        assert fast.strict_fallbacks[call] == sum(strict)
        for k, (g, w) in enumerate(zip(got, want)):
            assert abs(g.objective_value - w.objective_value) <= 1e-9 * max(1.0, abs(w.objective_value)), (call, k)
            gv, wv = g._solution._values, w._solution._values
            assert gv.keys() == wv.keys(), (call, k)
            for key, v in wv.items():
                assert abs(gv[key] - v) <= 1e-9 * max(1.0, abs(v)), (call, k, gv[key], v)
            if not strict[k]:
                assert fast.pivots[call][k] == ref.pivots[call][k], (call, k)
    assert fast.cold == ref.cold == [6, 0, 0]
    assert ref.strict_fallbacks == [] and len(fast.strict_fallbacks) == 3
    print(f"pivots per call: {fast.pivots}; handed to STRICT per call: {fast.strict_fallbacks}")
