"""tests/exact_shadow.py is right, and the LP groups of tests/test_gpu_near_tie_exact.py hold what
that file needs -- both established from the CPU oracle's logs alone, before a GPU is involved.

The shadow follows the oracle's pivot log in exact rational arithmetic.  Where exact arithmetic says a
pivot is clear-cut (not delicate, exact margin at least 1e-6) the float oracle must have taken exactly
that pivot; where the shadow reached the end its x and z must be the oracle's; a shadow whose
runner-up forgets one position must be caught by the same comparison.
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as ora
from tests import exact_shadow as es
from tests.lp_families import log3

_oracle_cache = {}


def oracle_run(name):
    """[(tag, a, b, c, oracle result, ShadowRun along the oracle's log)] of a group."""
    if name not in _oracle_cache:
        out = []
        for tag, a, b, c in es.group_lps(name):
            r = ora.simplex_solve(ora.stdform_from_dense(a, b, c), max_iter=es.GROUPS[name]["cap"])
            out.append((tag, a, b, c, r, es.follow_cached(tag, a, b, c, log3(r.pivots))))
        _oracle_cache[name] = out
    return _oracle_cache[name]


def oracle_disagreements(steps, log):
    """Pivots exact arithmetic calls clear-cut at which the oracle did something else."""
    return [j for j, (s, p) in enumerate(zip(steps, log))
            if not s.must_flag and s.margin >= es.NO_SPURIOUS_ABOVE and s.decision != p]


# ---------------------------------------------------------------------------------- by hand, 3 x 4
A34 = [[4, 1, 0, 2], [0, 2, 1, 1], [-1, 1, 3, 0]]
B34 = [1, 2, 2]


def test_hand_case_with_a_known_margin_of_one_third():
    """Slack basis: the z side's ratios are the costs (3, 2, 1, -1), the x side's are -b = (-1, -2, -2).
    primal = -1 < dual = 3: a primal step with mu = 3, column 0 enters with margin (3 - 2) / 3; the
    comparison's margin is (3 - -1) / 3; the ratio test has dx = (4, 0, -1) over x + 3 xbar = (4, 5, 5):
    one positive ratio, no competitor.  M = 1/3, and the pivot is (primal, 0, slack of row 0 = 4)."""
    sh = es.Shadow(A34, B34, [3, 2, 1, -1])
    s = sh.decide()
    assert (s.kind, s.mu, s.first_z, s.first_x, s.ratio_set) == (es.PRIMAL, 3, {0}, {0}, {0})
    assert s.margin == Fraction(1, 3) and not s.delicate and s.decision == (es.PRIMAL, 0, 4)
    assert sh.pivot(0, 4)
    # t = x_0 / dx_0 = 1/4; x = (t, 2 - 0 t, 2 + t); s = z_0 / dz_0 = -3 / -4; z = z - s dz, z_0 = s
    assert sh.x == [Fraction(1, 4), 2, Fraction(9, 4)] and sh.basis == [0, 5, 6] and sh.nonbasis == [4, 1, 2, 3]
    assert sh.z == [Fraction(3, 4), -2 + Fraction(3, 4), -1, 1 + Fraction(3, 2)]
    assert sh.xbar == [Fraction(1, 4), 1, Fraction(5, 4)] and sh.zbar == [Fraction(-1, 4), Fraction(3, 4), 1, Fraction(1, 2)]


def test_hand_case_with_a_known_tie():
    """Costs (3, 3, 1, -1): columns 0 and 1 tie for entering.  Margin 0, delicate, no unique decision,
    and the tied codes are reported; the reference takes the lower position."""
    s = es.Shadow(A34, B34, [3, 3, 1, -1]).decide()
    assert s.first_z == {0, 1} and s.margin == 0 and s.reasons == {"tie"} and s.decision is None
    assert s.tie_codes == {0, 1} and s.entering_set == {0, 1} and s.leaving_set == {4}
    run = es.follow(A34, B34, [3, 3, 1, -1], [(es.PRIMAL, 0, 4)])
    assert run.stopped_at is None and len(run.steps) == 1 and run.terminal is not None
    # a pivot element that is exactly zero (column 0, row 1) stops the shadow
    assert es.follow(A34, B34, [3, 3, 1, -1], [(es.PRIMAL, 0, 5)]).stopped_at == 0
    # identical columns and rows are twins; nothing else is
    assert es.twin_classes([[1, 1, 2], [1, 1, 2], [0, 0, 5]], [7, 7, 7], [4, 4, 4]) == {0: 0, 1: 0, 3: 1, 4: 1}


def test_margin_formula_is_dzg_margin():
    assert es.rel_margin(Fraction(3), Fraction(2)) == Fraction(1, 3)
    assert es.rel_margin(Fraction(1), Fraction(-4)) == Fraction(5, 4)
    assert es.rel_margin(Fraction(0), Fraction(0)) == 0 and es.rel_margin(Fraction(2), Fraction(2)) == 0
    assert es.rel_margin(Fraction(2), None) == es.INF
    assert es.argmax_set([(Fraction(1), 4), (Fraction(1), 2), (Fraction(0), 0)])[0] == {2, 4}


# ---------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("name", sorted(es.GROUPS))
def test_shadow_agrees_with_the_oracle(name):
    bad_pivot, bad_state, bad_verdict = [], [], []
    for tag, a, b, c, r, run in oracle_run(name):
        log = log3(r.pivots)
        bad_pivot += [(tag, j) for j in oracle_disagreements(run.steps, log)]
        if run.stopped_at is not None:
            continue
        for got, want in ((r.x, run.x), (r.z, run.z)):
            want = np.array([float(v) for v in want])
            # (1e-9 of the value where it is above 1: x and z reach 1e5 on LPs that end unbounded)
            gap = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            if want.size and gap.max() > 1e-9:
                bad_state.append((tag, float(gap.max())))
        assert r.basis.tolist() == run.basis and r.nonbasis.tolist() == run.nonbasis
        t = run.terminal
        if r.status != "iter_limit" and not t.must_flag and not t.opt_edge and r.status != t.verdict:
            bad_verdict.append((tag, r.status, t.verdict))
    assert not bad_pivot, f"the oracle left the exact path at a clear-cut pivot: {bad_pivot}"
    assert not bad_state, f"final x / z differ from the oracle's by more than 1e-9: {bad_state}"
    assert not bad_verdict, f"(oracle, exact) verdicts: {bad_verdict}"


@pytest.mark.parametrize("name", sorted(es.GROUPS))
def test_groups_hold_what_the_gpu_tests_need(name):
    """At least 40 delicate and 150 clear-cut pivots, at most 10 % unchecked behind a zero pivot
    element, and no exact margin in (0, 1e-6): claims C and D rest on that gap."""
    delicate = clean = unchecked = total = 0
    smallest = es.INF
    for tag, a, b, c, r, run in oracle_run(name):
        total += len(r.pivots)
        unchecked += len(r.pivots) - len(run.steps)
        steps = run.steps + ([run.terminal] if run.terminal is not None else [])
        delicate += sum(s.must_flag for s in run.steps)
        clean += sum(not s.must_flag for s in run.steps)
        smallest = min([smallest] + [s.margin for s in steps if s.margin > 0])
    print(f"{name}: {total} pivots, {delicate} delicate, {clean} clear-cut, {unchecked} unchecked, "
          f"smallest non-zero exact margin {float(smallest):.3e}")
    assert delicate >= 40 and clean >= 150 and 10 * unchecked <= total
    assert smallest >= es.NO_SPURIOUS_ABOVE


def test_solver_group_has_ties_between_twins_and_every_bucket_its_rows():
    firsts = 0
    for tag, a, b, c, r, run in oracle_run("solver"):
        twins = es.twin_classes(a.tolist(), b.tolist(), c.tolist())
        firsts += any(s.reasons == {"tie"} and len({twins.get(v, -1 - v) for v in s.tie_codes}) == 1
                      for s in run.steps)
    assert firsts >= 4
    for name, lo, hi in (("batch16", 8, 16), ("batch32", 17, 32), ("batch64", 33, 64), ("batch72", 65, 72)):
        rows = [a.shape[0] for _, a, _, _ in es.group_lps(name)]
        assert len(rows) >= 64 and lo <= min(rows) and max(rows) <= hi
        assert all(a.shape[1] <= 100 for _, a, _, _ in es.group_lps(name))


# ---------------------------------------------------------------------------------- the check bites
@pytest.mark.parametrize("seed, skip", [(9126, 7), (9184, 9)])
def test_a_shadow_that_loses_one_runner_up_is_caught(seed, skip):
    """The mutant's runner-up never looks at one position (what a reduction that drops a lane or a
    partial does).  A tie with the candidate there then looks like a clear-cut pivot with the margin to
    the next candidate.  On these family-1 LPs the float oracle, whose tied ratios round differently,
    takes the tied candidate at that very position: the comparison of test_shadow_agrees_with_the_oracle
    passes with the shadow as it is and fails with the mutant."""
    from tests.lp_families import make_lp

    a, b, c = make_lp(seed, 1, 8, 25)
    log = log3(ora.simplex_solve(ora.stdform_from_dense(a, b, c), max_iter=40).pivots)
    data = (a.tolist(), b.tolist(), c.tolist())
    assert not oracle_disagreements(es.follow(*data, log).steps, log)
    assert oracle_disagreements(es.follow(*data, log, skip_runner_up=skip).steps, log)
