"""The inverse W = B^-1 the batched FAST solver keeps in LDS (csrc/k_batch_fast.hip), read back by
dzg_debug_batch_fast_inverse -- the production kernel body with an epilogue that copies W out -- and
checked against the basis it claims to invert: R = W B - I in long double, all rows
(tests/inverse_check.py), at a bound that is 10x what a float64 transcription of the documented
algorithm leaves on the same inputs (tests/batch_fast_reference.py,
tests/test_batch_fast_inverse_host.py).

max_pivot_error agrees for any matrix in W, and pivot parity with the oracle is not checked for a
flagged LP; these tests look at the matrix: right after build_inverse in every bucket and at sizes
below the bucket's largest (scattered bases, row exchanges whose inverse is exact), after runs of
rank-1 updates with and without rebuilds inside the launch, and on singular bases."""
import functools

import numpy as np
import pytest

from tests import batch_fast_reference as bf
from tests import inverse_check as ic
from tests.lp_families import log3
from tests.test_gpu_batch import assert_same_run

pytestmark = pytest.mark.gpu

F6, F7 = "6 batch inverse", "7 batch updates"
WORST = {}  # family -> worst residual / bound ratio seen (printed at the end: pytest -s)


@pytest.fixture(scope="module")
def core():
    from dantzig_amd import core as c

    yield c
    for fam, r in sorted(WORST.items()):
        print(f"batch inverse residual / bound, worst of family {fam}: {r:.3e} (C = {ic.C_INVERSE[fam]})")


def check(case, w, basis, family, what=""):
    ratio = ic.residual(w, np.arange(case.m), case.a, basis, case.ns)
    worst = float(ratio.max())
    WORST[family] = max(WORST.get(family, 0.0), worst)
    assert worst <= ic.C_INVERSE[family], (family, case.name, what, worst, np.flatnonzero(ratio > ic.C_INVERSE[family])[:8])
    return worst


# ------------------------------------------------------------------ 1. fresh inversion
def test_fresh_inversion_in_every_bucket(core):
    """Families 1 and 2 in one call with no pivot: W is what build_inverse made of the starting
    basis.  Most LPs are smaller than their bucket's largest (ld = m | 1 < mmax + 1 in the carve-up);
    the 128-, 33-, 17- and 16-row members in a call of their own (33 and 17 now the largest of their
    buckets) and the 32-row ones in another come out bit for bit the same."""
    cases = bf.family1(core) + bf.family2(core)
    got = core.debug_batch_fast_inverse([c.lp for c in cases], 0)
    assert len(got) == len(cases)
    per_m = {}
    for c, (r, w) in zip(cases, got):
        assert (r.status, r.iterations, r.numerics) == ("iter_limit", 0, "fast"), (c.name, r.status, r.iterations)
        assert r.basis.tolist() == c.lp.basis.tolist() and r.nonbasis.tolist() == c.lp.nonbasis.tolist(), c.name
        assert r.refactors == 1, (c.name, r.refactors)  # every start basis has a structural column
        assert r.pivots == [] and np.array_equal(r.x, c.lp.x) and np.array_equal(r.z, c.lp.z), c.name
        assert w.shape == (c.m, c.m) and np.isfinite(w).all(), c.name
        worst = check(c, w, c.lp.basis, F6)
        per_m[c.m] = max(per_m.get(c.m, 0.0), worst)
        if c.exact is not None:
            assert np.array_equal(w, c.exact), (c.name, np.count_nonzero(w != c.exact))
    print("fresh inversion, worst ratio by rows: " + ", ".join(f"{m}: {r:.3g}" for m, r in sorted(per_m.items())))
    for rows in ((128, 33, 17, 16), (32,)):
        idx = [i for i, c in enumerate(cases) if c.m in rows]
        assert {cases[i].m for i in idx} == set(rows)
        again = core.debug_batch_fast_inverse([cases[i].lp for i in idx], 0)
        for i, (r, w) in zip(idx, again):
            assert np.array_equal(w, got[i][1]), (cases[i].name, "W depends on the LP's company")
            assert_same_run(r, got[i][0], cases[i].name)


def test_an_all_slack_start_is_written_directly(core):
    """refactors counts eliminations only: a slack basis (in any order) is a permutation."""
    cases = [c for c in bf.family4(core) if c.name.startswith("slack start")]
    lp0 = cases[0].lp
    perm = np.random.default_rng(5).permutation(lp0.m)
    import dataclasses

    shuffled = dataclasses.replace(lp0, basis=lp0.basis[perm].copy(), x=lp0.x[perm].copy())
    got = core.debug_batch_fast_inverse([c.lp for c in cases] + [shuffled], 0)
    for c, (r, w) in zip(cases, got):
        assert (r.status, r.iterations, r.refactors) == ("iter_limit", 0, 0), c.name
        assert np.array_equal(w, np.eye(c.m)), c.name
    r, w = got[-1]
    assert r.refactors == 0 and np.array_equal(w, np.eye(lp0.m)[perm])  # W[p][r] = 1 where basis[p] is row r's slack


# ------------------------------------------------------------------ 2. after pivots
@functools.lru_cache(maxsize=None)
def _family4():
    from dantzig_amd import core

    cases = bf.family4(core)
    return cases, [bf.oracle_run(c, max(bf.F4_STOPS_REBUILT)) for c in cases]


@functools.lru_cache(maxsize=None)
def _run(stop, every):
    """Family 4 stopped after `stop` pivots, one call (shared by the tests below)."""
    from dantzig_amd import core

    cases, _ = _family4()
    return core.debug_batch_fast_inverse([c.lp for c in cases], stop, refactor_every=every,
                                         near_tie_action=core.NEAR_TIE_COUNT)


NO_REBUILD = 1 << 20
STOPS = [(s, bf.F4_REFACTOR) for s in bf.F4_STOPS_REBUILT] + [(s, NO_REBUILD) for s in bf.F4_STOPS_PLAIN]


@pytest.mark.parametrize("stop,every", STOPS)
def test_inverse_after_a_run_of_pivots(core, stop, every):
    """The W one launch leaves after `stop` pivots -- rank-1 updates, rebuilt every 8 pivots or not
    at all -- inverts the basis the result reports; where nothing was flagged the pivots so far are
    the oracle's.  The integer and 0/1 LPs bring slacks back in (FTRAN of a slack is a column of W)."""
    cases, oracle = _family4()
    flagged = []
    for c, w_or, (r, w) in zip(cases, oracle, _run(stop, every)):
        what = f"{c.name} stop {stop} every {every}"
        assert r.iterations <= stop and r.numerics == "fast", what
        assert r.status not in ("running", "singular"), (what, r.status)
        if r.status == "iter_limit":
            assert r.iterations == stop, what
        assert np.isfinite(w).all(), what
        check(c, w, r.basis, F7, what)
        if every == bf.F4_REFACTOR and r.iterations == stop and stop > every:
            assert r.refactors >= stop // every, (what, r.refactors)
        if every == NO_REBUILD:
            assert r.refactors == (0 if c.name.startswith(("slack", "make_lp")) else 1), (what, r.refactors)
        want = log3(w_or.pivots)[:stop]
        if r.near_ties > 0:  # certified up to the first flagged pivot only
            flagged.append(c.name)
            assert 0 <= r.first_near_tie <= r.iterations, what
            assert log3(r.pivots)[:r.first_near_tie] == want[:r.first_near_tie], what
            continue
        assert log3(r.pivots) == want, f"{what}: pivot sequence differs from the oracle's"
        if len(want) < stop:
            assert r.status == w_or.status, (what, r.status, w_or.status)
    print(f"stop {stop} every {every}: flagged {flagged}")
    # the integer LPs meet exact ties by construction; of the 14 continuous ones at most 1 in 8
    assert sum(not name.startswith("make_lp") for name in flagged) <= 1, flagged


def test_slacks_enter_in_the_update_family(core):
    cases, _ = _family4()
    for c, (r, _) in zip(cases, _run(max(bf.F4_STOPS_REBUILT), bf.F4_REFACTOR)):
        if c.name.startswith("make_lp"):
            assert any(e >= c.ns for _, e, _, _ in r.pivots), f"{c.name}: no entering variable is a slack"


def test_a_rebuild_that_falls_due_at_the_budget_runs_before_the_launch_ends(core):
    """refactor_every = 8: after 7 pivots W is the start's inverse and seven updates; the rebuild due
    after the 8th runs at the top of the next step, before the budget ends the launch, so the budget
    8 returns a fresh inverse and the budget 9 the same rebuild and one update: one rebuild more than
    the budget 7, both within the bound (asserted by test_inverse_after_a_run_of_pivots)."""
    cases, _ = _family4()
    n = 0
    for c, (r7, _), (r8, w8), (r9, w9) in zip(cases, _run(7, 8), _run(8, 8), _run(9, 8)):
        if r9.iterations < 9:
            continue
        n += 1
        assert r8.refactors == r7.refactors + 1 == r9.refactors, (c.name, r7.refactors, r8.refactors, r9.refactors)
        assert log3(r9.pivots)[:8] == log3(r8.pivots), c.name
        check(c, w8, r8.basis, F7, "budget 8")
        check(c, w9, r9.basis, F7, "budget 9")
        assert not np.array_equal(w8, w9), c.name
    assert n >= 14


# ------------------------------------------------------------------ 3. singular bases
def test_singular_bases_end_singular_and_auto_hands_them_to_strict(core):
    """A zero pivot in build_inverse: an all-zero basic column, two equal basic columns, a zero row
    whose slack is nonbasic.  FAST ends the LP before its first pivot; its neighbours in the batch
    do not notice; AUTO solves it again in STRICT."""
    sing = bf.family3(core)
    regular = [c for c in bf.family1(core) if c.m in (16, 17, 33, 65, 128) and "seed 0" in c.name
               and f"k={c.m // 2} " in c.name]
    assert len(regular) == 5
    lps, is_sing = [], []
    for i, c in enumerate(sing):  # a regular LP after every third singular one
        lps.append(c.lp)
        is_sing.append(True)
        if i % 3 == 2 and i // 3 < len(regular):
            lps.append(regular[i // 3].lp)
            is_sing.append(False)
    assert is_sing.count(False) == len(regular)
    fast = core.solve_batch_fast(lps, numerics=core.FAST, max_iter=200)
    alone = iter(core.solve_batch_fast([c.lp for c in regular], numerics=core.FAST, max_iter=200))
    names = iter(c.name for c in sing)
    for r, s in zip(fast, is_sing):
        if s:
            name = next(names)
            assert (r.status, r.iterations, r.numerics) == ("singular", 0, "fast"), (name, r.status, r.iterations)
            assert r.refactors == 1 and r.pivots == [], (name, r.refactors)
        else:
            a = next(alone)
            assert r.iterations > 0
            assert_same_run(r, a, "a regular LP among singular ones")
            assert (r.refactors, r.near_ties) == (a.refactors, a.near_ties)
    hook = core.debug_batch_fast_inverse([c.lp for c in sing], 0)
    assert [(r.status, r.iterations, r.refactors) for r, _ in hook] == [("singular", 0, 1)] * len(sing)
    auto = core.solve_batch_fast(lps, numerics=core.AUTO, max_iter=200)
    idx = [i for i, s in enumerate(is_sing) if s]
    strict = core.solve_batch([lps[i] for i in idx], max_iter=200)
    for i, w in zip(idx, strict):
        assert auto[i].numerics == "strict", i
        assert_same_run(auto[i], w, f"singular LP {i} under AUTO")
