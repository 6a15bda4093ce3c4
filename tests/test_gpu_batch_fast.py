"""The batched FAST solver on the GPU (dzg_batch_solve_fast, core.solve_batch_fast,
solve_many(fast=True)): one workgroup per LP with the explicit basis inverse in LDS follows the CPU
oracle pivot for pivot wherever no decision came within rounding of a tie, says so where one did,
and under AUTO hands exactly those LPs to the STRICT batch."""
import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import core
from oracle import oracle as ora
from tests import state_check as sc
from tests.lp_families import log3, make_lp
from tests.rays_helpers import infeasible_lp, unbounded_lp
from tests.test_gpu_batch import assert_bit_equal, assert_same_run

pytestmark = pytest.mark.gpu

# bucket and wave edges (16 / 32 / 64 / 128 rows), q not a multiple of 64, q < 2m
SHAPES = [(1, 3), (15, 40), (16, 16), (17, 20), (33, 64), (64, 128), (65, 100), (127, 130), (128, 256)]
SEEDS = (3, 4)


def _dense(seed, m, ns):
    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    return np.array(a), np.array(b), np.array(c)


def _oracle(data, **kw):
    return ora.simplex_solve(ora.stdform_from_dense(*data), **kw)


class _Edges:
    """The kind-0 batch of test 1, solved once: data, LPs, FAST results (COUNT) and the oracle's."""

    def __init__(self):
        self.key = [(m, ns, s) for (m, ns) in SHAPES for s in SEEDS]
        self.data = [_dense(1000 * m + s, m, ns) for (m, ns, s) in self.key]
        self.lps = [core.CoreLP.from_inequality_form(*d) for d in self.data]
        self.got = core.solve_batch_fast(self.lps, numerics=core.FAST, near_tie_action=core.NEAR_TIE_COUNT)
        self.want = [_oracle(d) for d in self.data]

    def at(self, m, ns, seed=SEEDS[0]):
        return self.key.index((m, ns, seed))


@pytest.fixture(scope="module")
def edges():
    return _Edges()


def assert_follows_oracle(g, w, what):
    assert g.status == w.status, (what, g.status, w.status)
    assert log3(g.pivots) == log3(w.pivots), f"{what}: pivot sequence differs from the reference's"
    assert g.basis.tolist() == w.basis.tolist() and g.nonbasis.tolist() == w.nonbasis.tolist(), what
    assert abs(g.objective - w.objective) <= 1e-9 * max(1.0, abs(w.objective)), what
    assert np.allclose(g.x, w.x, rtol=1e-9, atol=1e-9), what


def test_pivot_parity_at_the_kernels_edges(edges):
    flagged = 0
    for (m, ns, s), g, w in zip(edges.key, edges.got, edges.want):
        what = f"{m} x {ns} seed {s}"
        print(f"{what}: {g.status} {g.iterations} pivots, near_ties {g.near_ties}, min_margin {g.min_margin:.3e}, "
              f"max_pivot_error {g.max_pivot_error:.3e}, refactors {g.refactors}")
        assert g.numerics == "fast"
        if g.near_ties > 0:
            flagged += 1
            continue
        assert g.first_near_tie == -1
        assert_follows_oracle(g, w, what)
        assert g.margins is not None and len(g.margins) == g.iterations
        assert g.iterations == 0 or g.min_margin == np.min(g.margins)
    assert 8 * flagged <= len(edges.key), f"{flagged} of {len(edges.key)} LPs had a near tie"


def test_unbounded_infeasible_and_empty_lps_end_as_the_oracle_says():
    data = [unbounded_lp(11, 33, 50), unbounded_lp(12, 128, 140), infeasible_lp(13, 33, 50),
            infeasible_lp(14, 128, 140), (np.zeros((0, 3)), np.zeros(0), np.array([1.0, -1.0, 0.0]))]
    lps = [core.CoreLP.from_inequality_form(*d) for d in data]
    got = core.solve_batch_fast(lps, numerics=core.FAST)
    want = [_oracle(d) for d in data]
    assert [w.status for w in want] == ["unbounded", "unbounded", "infeasible", "infeasible", "panic"]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.status == w.status, (i, g.status, w.status, g.near_ties)
        if g.near_ties == 0:
            assert log3(g.pivots) == log3(w.pivots), i


def test_refactorisation_inside_and_between_launches(edges):
    """One shape per bucket.  The 15-, 17- and 33-row LPs end in 21-108 pivots, fewer than the default
    refactor_every: only refactor_every = 3 puts the one-wave elimination and the row updates at 16
    and 32 lanes a row on their path.  One of those may be left out, by name, if it was flagged."""
    skipped = []
    for shapes, every, short in ((((128, 256), (65, 100)), 8, 5), (((15, 40), (17, 20), (33, 64)), 3, 2)):
        idx = [edges.at(*sh) for sh in shapes]
        lps = [edges.lps[i] for i in idx]
        often = core.solve_batch_fast(lps, numerics=core.FAST, refactor_every=every, pivots_per_launch=short)
        inside = core.solve_batch_fast(lps, numerics=core.FAST, refactor_every=every, pivots_per_launch=40)
        for i, a, b in zip(idx, often, inside):
            w, d = edges.want[i], edges.got[i]
            runs = (("every launch", a), ("inside a launch", b), ("defaults", d))
            for name, g in runs:
                print(f"{edges.key[i]} {name}: {g.iterations} pivots, {g.refactors} refactors, near_ties {g.near_ties}")
            if every == 3 and any(g.near_ties > 0 for _, g in runs):
                skipped.append(edges.key[i])
                continue
            for name, g in runs:
                assert g.status == w.status == "optimal" and log3(g.pivots) == log3(w.pivots), (edges.key[i], name)
            assert a.refactors >= a.iterations // every
            assert b.refactors >= b.iterations // every
            assert d.refactors < a.refactors
    assert len(skipped) <= 1, f"flagged and left out: {skipped}"


def test_carried_state_stays_within_the_short_solve_bound(edges):
    """D of tests/state_check.py on the final basis.  Observed on an MI355X: see DESIGN.md 7g."""
    for m, ns in ((128, 256), (64, 128), (17, 20)):
        i = edges.at(m, ns)
        a = edges.data[i][0]
        g = edges.got[i]
        ex = sc.exact_state(a, ns, edges.lps[i], g.basis, g.nonbasis)
        d = ex.drift(g)
        print(f"{m} x {ns}: {g.iterations} pivots, D = {d['D']:.3e} (x {d['x']:.3e}, xbar {d['xbar']:.3e}, "
              f"z {d['z']:.3e}, zbar {d['zbar']:.3e}), helper error {max(ex.err.values()):.1e}")
        assert d["D"] <= sc.C_STATE_SHORT, (m, ns, d)


# 64 LPs of kind 1 from seed 9300 on and 64 of kind 2 from seed 9400 on, m in 4..64
TIE_SEEDS = [(9300 + i, 1) for i in range(64)] + [(9400 + i, 2) for i in range(64)]


def test_auto_hands_the_flagged_lps_to_strict():
    data = [make_lp(seed, kind, 4, 65) for seed, kind in TIE_SEEDS]
    lps = [core.CoreLP.from_inequality_form(*d) for d in data]
    auto = core.solve_batch_fast(lps, numerics=core.AUTO, max_iter=4096)
    redo = [i for i, r in enumerate(auto) if r.numerics == "strict"]
    kept = [i for i, r in enumerate(auto) if r.numerics == "fast"]
    print(f"AUTO: {len(redo)} of {len(lps)} re-solved in STRICT, {len(kept)} stayed FAST: "
          f"{[TIE_SEEDS[i] for i in kept]}")
    assert redo and kept and len(redo) + len(kept) == len(lps)
    strict = dict(zip(redo, core.solve_batch([lps[i] for i in redo], max_iter=4096)))
    for i in redo:
        assert_same_run(auto[i], strict[i], f"LP {i} (seed {TIE_SEEDS[i]})")
    for i in kept:
        w = _oracle(data[i], max_iter=4096)
        assert auto[i].near_ties == 0, i
        assert auto[i].status == w.status and log3(auto[i].pivots) == log3(w.pivots), (i, TIE_SEEDS[i])
    # the same batch told to stop: the flagged LPs end before the pivot that was flagged, on the
    # reference's path so far, and no later than where FAST left to itself first leaves that path
    stop = core.solve_batch_fast(lps, numerics=core.FAST, near_tie_action=core.NEAR_TIE_STOP, max_iter=4096)
    count = core.solve_batch_fast(lps, numerics=core.FAST, near_tie_action=core.NEAR_TIE_COUNT, max_iter=4096)
    for i in redo:
        s, c, w = stop[i], count[i], log3(strict[i].pivots)
        assert s.status in ("near_tie", "singular", "panic"), (i, s.status)
        mine = log3(c.pivots)
        div = next((k for k in range(min(len(mine), len(w))) if mine[k] != w[k]), min(len(mine), len(w)))
        assert s.iterations <= div, (i, s.iterations, div)
        assert log3(s.pivots) == w[:s.iterations], i
        if s.status == "near_tie":
            assert c.first_near_tie == s.iterations, (i, c.first_near_tie, s.iterations)
    for i in kept:
        assert stop[i].status == auto[i].status and stop[i].pivots == auto[i].pivots, i


def test_an_lp_does_not_notice_its_place_in_the_batch():
    lps = [core.CoreLP.from_inequality_form(*_dense(7000 + i, 128, 48)) for i in range(257)]
    got = core.solve_batch_fast(lps, numerics=core.FAST)  # one more than the 128-row bucket's grid
    alone = core.solve_batch_fast([lps[256]], numerics=core.FAST)[0]
    assert got[256].iterations > 0
    assert_same_run(got[256], alone, "LP 256 alone and in a batch of 257")
    assert_bit_equal(got[256].margins, alone.margins, "margins")
    assert (got[256].near_ties, got[256].refactors) == (alone.near_ties, alone.refactors)
    assert_bit_equal([got[256].max_pivot_error, got[256].min_margin], [alone.max_pivot_error, alone.min_margin])


def test_limit_and_resume_from_a_structural_basis(edges):
    for m, ns in ((128, 256), (33, 64), (15, 40), (17, 20)):
        i = edges.at(m, ns)
        lp, w = edges.lps[i], edges.want[i]
        half = w.iterations // 2
        assert half >= 2
        part = core.solve_batch_fast([lp], numerics=core.FAST, max_iter=half)[0]
        assert part.status == "iter_limit" and part.iterations == half
        rest = core.solve_batch_fast([core.resumed_from(lp, part)], numerics=core.FAST)[0]
        assert rest.refactors >= 1  # the launch started by inverting a basis that is not all slack
        assert rest.status == w.status
        assert log3(part.pivots) + log3(rest.pivots) == log3(w.pivots), (m, ns)


def _surface_models():
    out = []
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    out.append(([x, y], dz.Maximize(3 * x + 2 * y).subject_to([x + y <= 4, x + 3 * y <= 6, x <= 3])))
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    out.append(([x, y], dz.Minimize(2 * x + 3 * y).subject_to([x + y == 5, x - y <= 1])))           # equality
    x, y = dz.Variable.free(), dz.Variable.nonneg()
    out.append(([x, y], dz.Minimize(x + 2 * y).subject_to([x >= -3.5, x + y >= 1.25])))            # free
    x, y = dz.Variable(lb=-1.0, ub=2.5), dz.Variable(lb=0.5, ub=4.0)
    out.append(([x, y], dz.Maximize(1.5 * x - 0.25 * y).subject_to([x + y <= 5.75])))             # bounds
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    out.append(([x, y], dz.Maximize(x + y).subject_to([x + y <= 1, x + y >= 2])))                  # infeasible
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    out.append(([x, y], dz.Maximize(x + y).subject_to([x - y <= 1])))                              # unbounded
    x, y, z = dz.Variable.nonneg(), dz.Variable.free(), dz.Variable(lb=None, ub=3.0)
    out.append(([x, y, z], dz.Maximize(0.7 * x + 1.1 * y + 0.3 * z).subject_to(
        [x + 2 * y + z <= 7.5, 3 * x - y <= 4.25, y - z <= 2.125, x + y + z == 6.5])))
    vs = [dz.Variable.nonneg() for _ in range(6)]
    rng = np.random.default_rng(5)
    cons = [sum(float(rng.uniform(0.1, 1)) * v for v in vs) <= float(rng.uniform(1, 2)) for _ in range(5)]
    out.append((vs, dz.Maximize(sum(float(rng.uniform(0.1, 1)) * v for v in vs)).subject_to(cons)))
    return out


def test_solve_many_fast_agrees_with_solve():
    items = _surface_models()
    got = dz.solve_many([p for _, p in items], fast=True, return_exceptions=True)
    kinds = set()
    for i, ((vs, p), g) in enumerate(zip(items, got)):
        try:
            w = p.solve()
        except Exception as e:  # noqa: BLE001
            print(f"model {i}: {type(e).__name__}: {e}")
            assert type(g) is type(e), (i, g, e)
            kinds.add(type(e).__name__)
            continue
        assert not isinstance(g, Exception), (i, g)
        kinds.add("optimal")
        assert abs(g.objective_value - w.objective_value) <= 1e-9 * max(1.0, abs(w.objective_value)), i
        for v in vs:
            assert abs(g[v] - w[v]) <= 1e-9 * max(1.0, abs(w[v])), (i, g[v], w[v])
    assert kinds >= {"optimal", "InfeasibleError", "UnboundedError"}, kinds
