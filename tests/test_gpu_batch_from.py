"""Batches re-optimised from their last bases on the GPU (csrc/k_batch_restart.hip,
dzg_batch_solve_from, core.solve_batch(start=...), dantzig_amd.sessions).

The restart state of a warm LP is the CPU oracle's lu_solve / neg_t_dot bit for bit and the pivots
that follow are the oracle's from that state (tests/batch_from_reference.py), in every bucket and at
every block size; cold and warm LPs mix in one call without touching each other; a singular start
ends singular without a pivot; duals compose; SessionBatch carries each model's basis from call to
call.  The cases and their seeds are tests/test_batch_from_host.py's, which checks on the CPU that
every continuation here takes at least one pivot.

The restart state is read after a stop before the first pivot: with epsilon = 1e300 the optimality
test of Simplex::status passes at once, so the call returns the state the restart kernel wrote."""
import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi, core
from tests import batch_from_reference as bfr
from tests import duals_reference as dref
from tests import state_check as sc
from tests import test_batch_from_host as h
from tests.duals_helpers import assert_bit_equal, assert_same_run
from tests.optimality import certificate

pytestmark = pytest.mark.gpu

STOP = dict(epsilon=1e300)


def _lp(a, b, c):
    return core.CoreLP.from_inequality_form(a, b, c)


def _assert_restart_state(r, ref, what):
    assert (r.status, r.iterations, r.pivots) == ("optimal", 0, []), (what, r.status, r.iterations)
    assert r.basis.tolist() == ref.sf.basis.tolist() and r.nonbasis.tolist() == ref.sf.nonbasis.tolist(), what
    assert_bit_equal(r.x, ref.x, what + " x")
    assert_bit_equal(r.z, ref.z, what + " z")
    assert (r.xbar == 1.0).all() and (r.zbar == 1.0).all(), what


def _stopped_and_full(lps, start, **kw):
    return core.solve_batch(lps, start=start, **STOP, **kw), core.solve_batch(lps, start=start, **kw)


# ------------------------------------------------------------------ 1. every bucket, every block size
def test_restart_state_and_continuation_are_the_oracles_over_a_ragged_batch():
    cases = h.ragged_cases()
    assert [w.a.shape for w in cases] == [(1, 3), (2, 3), (16, 24), (17, 24), (33, 40), (64, 40), (65, 72), (128, 40)]
    cold = core.solve_batch([_lp(w.a, w.b, w.c) for w in cases])
    for w, r in zip(cases, cold):
        assert_same_run(r, w.first, f"cold {w.a.shape}")
    lps = [_lp(w.a, w.b2, w.c2) for w in cases]
    stopped, full = _stopped_and_full(lps, cold)
    for w, s, r in zip(cases, stopped, full):
        what = f"{w.a.shape[0]}x{w.a.shape[1]}"
        _assert_restart_state(s, w.ref, what)
        assert r.iterations >= 1, what
        assert_same_run(r, w.want, what)
        print(f"{what}: {w.first.iterations} pivots cold, {r.iterations} after the change")


# ------------------------------------------------------------------ 2. kernel edges on the start basis
def test_start_bases_at_the_kernels_edges():
    a, b2, c2, slack_ref, slack_want = h.slack_start_case()
    p, pb2, pc2, planted_ref, planted_want = h.planted_case()
    f, x2, kc2, first, kat_ref, kat_want = h.kat_case()
    w = h.permuted_case()
    lps = [_lp(a, b2, c2), _lp(p.a, pb2, pc2),
           core.CoreLP(a=f.a, c=kc2, basis=f.basis, nonbasis=f.nonbasis, x=x2, z=f.z, var_col=f.var_col,
                       constant=f.constant),
           _lp(w.a, w.b2, w.c2)]
    start = [(np.arange(24, 41), np.arange(24)), (p.basis, p.nonbasis), (first.basis, first.nonbasis),
             (w.first.basis, w.ref.sf.nonbasis)]
    assert (p.basis < 20).all()                                           # all m basics structural
    assert w.ref.sf.nonbasis.tolist() == w.first.nonbasis[::-1].tolist()  # handed over in reverse
    stopped, full = _stopped_and_full(lps, start)
    refs = [("all-slack start", slack_ref, slack_want), ("all-structural start", planted_ref, planted_want),
            ("KAT non_standard_variables", kat_ref, kat_want), ("permuted nonbasis", w.ref, w.want)]
    for (what, ref, want), s, r in zip(refs, stopped, full):
        _assert_restart_state(s, ref, what)
        assert r.iterations >= 1, what
        assert_same_run(r, want, what)
    # the all-slack start is the cold solve of the same LP
    assert_same_run(full[0], core.solve_batch([lps[0]])[0], "all-slack start = cold")


# ------------------------------------------------------------------ 3. cold and warm in one call
def _mixed():
    ragged = {w.a.shape: w for w in h.ragged_cases()}
    cases = list(h.mixed_cases()) + [ragged[(65, 72)], ragged[(2, 3)], ragged[(33, 40)]]
    lps = [_lp(w.a, w.b2, w.c2) for w in cases]
    start = [None if k % 2 == 0 else (w.first.basis, w.first.nonbasis) for k, w in enumerate(cases)]
    return cases, lps, start


def test_cold_and_warm_lps_mix_in_one_call():
    cases, lps, start = _mixed()
    got = core.solve_batch(lps, start=start)
    cold = core.solve_batch(lps)
    for k, (w, g) in enumerate(zip(cases, got)):
        what = f"LP {k} {w.a.shape}"
        if start[k] is None:
            assert_same_run(g, cold[k], what + " cold")
        else:
            alone = core.solve_batch([lps[k]], start=[start[k]])[0]
            assert_same_run(g, alone, what + " warm, alone")
            assert_same_run(g, w.want, what + " warm, reference")
    back = core.solve_batch(lps[::-1], start=start[::-1])[::-1]
    for k, (g, r) in enumerate(zip(got, back)):
        assert_same_run(r, g, f"LP {k} in the reversed batch")
    # every entry None, and no start at all: dzg_batch_solve's results
    for k, (g, r) in enumerate(zip(core.solve_batch(lps, start=[None] * len(lps)), cold)):
        assert_same_run(g, r, f"LP {k} with start = None")


# ------------------------------------------------------------------ 4. more LPs than one launch takes
def test_a_bucket_that_needs_two_restart_launches():
    cases = h.chunk_cases()
    assert len(cases) == 257 and cases[0].a.shape == (65, 8)
    lps = [_lp(w.a, w.b2, w.c2) for w in cases]
    got = core.solve_batch(lps, start=[(w.first.basis, w.first.nonbasis) for w in cases])
    for k, (w, g) in enumerate(zip(cases, got)):
        assert_same_run(g, w.want, f"LP {k}")
    print(f"257 x 65x8: {sum(g.iterations for g in got)} pivots warm, at most {max(g.iterations for g in got)}")


# ------------------------------------------------------------------ 5. a singular start
def test_a_singular_start_ends_singular_and_leaves_its_neighbours_alone():
    ragged = {w.a.shape: w for w in h.ragged_cases()}
    left, right = ragged[(16, 24)], ragged[(17, 24)]
    sing = h.singular_cases()
    lps = [_lp(left.a, left.b2, left.c2)]
    start = [(left.first.basis, left.first.nonbasis)]
    for a, basis, nonbasis in sing:
        lps.append(_lp(a, np.ones(a.shape[0]), np.ones(a.shape[1])))
        start.append((basis, nonbasis))
    lps.append(_lp(right.a, right.b2, right.c2))
    start.append((right.first.basis, right.first.nonbasis))
    got = core.solve_batch(lps, start=start)
    for (a, basis, nonbasis), g in zip(sing, got[1:3]):
        what = f"duplicated column {a.shape}"
        assert (g.status, g.iterations, g.pivots) == ("singular", 0, []), (what, g.status, g.iterations)
        assert g.basis.tolist() == basis.tolist() and g.nonbasis.tolist() == nonbasis.tolist(), what
    assert_same_run(got[0], left.want, "left neighbour")
    assert_same_run(got[3], right.want, "right neighbour")
    # a result that ended singular is no start: the next call solves that LP cold
    again = core.solve_batch(lps, start=got)
    for k in (1, 2):
        assert_same_run(again[k], core.solve_batch([lps[k]])[0], f"LP {k} after its singular end")


# ------------------------------------------------------------------ 6. duals compose
def test_duals_of_a_warm_batch_are_the_references():
    cases = h.mixed_cases()
    lps = [_lp(w.a, w.b2, w.c2) for w in cases]
    start = [(w.first.basis, w.first.nonbasis) for w in cases]
    got = core.solve_batch(lps, start=start, duals=True)
    for k, (w, g) in enumerate(zip(cases, got)):
        what = f"LP {k}"
        m, ns = w.a.shape
        assert_same_run(g, w.want, what)
        du = g.duals
        assert du is not None and du.source == "fresh", what
        ref = dref.core_duals(sc.stdform(w.a, ns, bfr.full_c(w.c2, m), g), g, rhs0=w.b2)
        assert_bit_equal(du.y, ref.y, what + " y")
        assert_bit_equal(du.d, ref.d, what + " d")
        assert_bit_equal([du.dual_obj, du.primal_obj], [ref.dual_obj, g.objective], what + " objectives")
        assert_bit_equal([du.primal_infeas, du.dual_infeas, du.z_diff],
                         [ref.primal_infeas, ref.dual_infeas, ref.z_diff], what + " scalars")
        cert = certificate(w.a, w.b2, w.c2, g.basis)
        scale = max(1.0, abs(cert["primal_obj"]))
        assert cert["primal_infeas"] <= 1e-9 and cert["dual_infeas"] <= 1e-9, (what, cert)
        assert abs(cert["primal_obj"] - cert["dual_obj"]) <= 1e-9 * scale, (what, cert)
        assert abs(g.objective - cert["primal_obj"]) <= 1e-9 * scale, (what, cert)


# ------------------------------------------------------------------ 7. the modelling surface
def _rhs(problem, new_b):
    return {problem.constraints[i]: b for i, b in new_b.items()}


def test_session_batch_carries_every_models_basis_from_call_to_call():
    probs, refs = h.session_problems(), h.session_reference()
    batch = dz.sessions([p for p, _, _ in probs])
    first = batch.solve()
    for k, ((p, _, _), sol) in enumerate(zip(probs, first)):
        with p.session() as session:     # the values are mapped as Session.solve maps them
            alone = session.solve()
        assert sol._solution._values == alone._solution._values, k
        assert sol.objective_value == alone.objective_value, k
    second = batch.solve(rhs=[_rhs(p, new_b) for p, new_b, _ in probs])
    for k, ((_, _, written), sol) in enumerate(zip(probs, second)):
        want = written.solve().objective_value
        assert abs(sol.objective_value - want) <= 1e-9 * max(1.0, abs(want)), (k, sol.objective_value, want)
    assert batch.pivots[0] == [first_.iterations for first_, _, _, _ in refs]
    assert batch.pivots[1] == [want.iterations for _, _, want, _ in refs]
    assert batch.cold == [8, 0]
    print(f"pivots per call: {batch.pivots}")
    # an infeasible change: that model's exception, its index in the message, and the batch goes on
    k_bad, bad_b, back_b = h.SESSION_INFEASIBLE
    rhs = [None] * 8
    rhs[k_bad] = _rhs(probs[k_bad][0], bad_b)
    with pytest.raises(dz.exceptions.InfeasibleError, match=f"model {k_bad}"):
        batch.solve(rhs=rhs)
    rhs[k_bad] = _rhs(probs[k_bad][0], back_b)      # (changes accumulate: only this row goes back)
    third = batch.solve(rhs=rhs, return_exceptions=True)
    for k, (s2, s3) in enumerate(zip(second, third)):
        assert not isinstance(s3, Exception), (k, s3)
        assert abs(s3.objective_value - s2.objective_value) <= 1e-9 * max(1.0, abs(s2.objective_value)), k
    assert batch.cold == [8, 0, 0, 0] and len(batch.pivots) == 4
    assert [n for k, n in enumerate(batch.pivots[3]) if k != k_bad] == [0] * 7   # nothing moved there
