"""The basis inverse FAST numerics keeps, read back (dzg_debug_basis_inverse) and checked against the
basis it claims to invert: R = Binv B - I in long double, row by row (tests/inverse_check.py).

max_pivot_error compares two evaluation orders of the same bilinear form e_p^T Binv a_q and agrees to
rounding for any matrix in Binv; these tests are what checks that Binv is B^-1 -- after the blocked
LU refactorisation (scattered bases: the row permutation of k_refactor.hip), after eta appends and
rank-64 flushes (one GPU, chain and seven launches), after compact-column appends and deletes
(slacks entering and leaving), on the sparse-basis path (X = A[R, S]^-1) and on row-sharded ranks,
whose stitched slices must be the single-GPU inverse bit for bit."""
import numpy as np
import pytest

from tests import inverse_check as ic
from tests.batch_fast_reference import scattered_lp

pytestmark = pytest.mark.gpu

WORST = {}  # family -> worst residual / bound ratio seen (printed at the end: pytest -s)


@pytest.fixture(scope="module")
def core():
    from dantzig_amd import core as c

    yield c
    for fam, r in sorted(WORST.items()):
        print(f"inverse residual / bound, worst of family {fam}: {r:.3e}")


def read_rows(s, rows):
    """The rows `rows` (ascending) of s's inverse, fetched range by range."""
    rows = np.asarray(rows, dtype=np.int64)
    out, info, i = [], None, 0
    while i < len(rows):
        j = i
        while j + 1 < len(rows) and rows[j + 1] == rows[j] + 1:
            j += 1
        blk, info = s.debug_inverse(int(rows[i]), int(rows[j]) + 1)
        out.append(blk)
        i = j + 1
    return np.concatenate(out) if out else np.zeros((0, s._lp.m)), info


def check(s, a, ns, family, recent_count=4, every_below=400, seed=0, extra=()):
    """Residual check of s's inverse at its current basis; returns (rows, inverse rows, info)."""
    r = s.result(log=recent_count > 0)
    m = len(r.basis)
    recent = ic.last_pivot_positions(r.basis, r.pivots, recent_count) + list(extra)
    rows = ic.sample_rows(m, r.basis, ns, recent, seed=seed, every_below=every_below)
    binv, info = read_rows(s, rows)
    assert info["neta"] < 64, info
    assert info["k"] == int(np.count_nonzero(r.basis < ns)), (info, "k != structural basics")
    ratio = ic.residual(binv, rows, a, r.basis, ns)
    worst = float(ratio.max())
    WORST[family] = max(WORST.get(family, 0.0), worst)
    bad = rows[ratio > ic.C_INVERSE[family]]
    assert worst <= ic.C_INVERSE[family], (family, worst, bad[:8], info, r.iterations)
    return rows, binv, info


# ------------------------------------------------------------------ 1. refactorisation, scattered bases
def _ks(m):
    return sorted({k for k in (1, 7, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 449, m - 1, m)
                   if 1 <= k <= m})


@pytest.mark.parametrize("m,k", [(m, k) for m in (700, 701, 1037, 2100) for k in _ks(m)])
def test_refactorisation_of_scattered_bases_is_the_inverse(core, m, k):
    """The blocked LU of k_refactor.hip on a basis whose structural columns sit at random positions
    (drow, dslot and the scatter of Binv0's rows are not the identity): right after the factorisation
    at creation, 48 pivots later (eta file), and after a second refactorisation there."""
    lp, a, ns = scattered_lp(core, m, k, seed=7000 + 3 * m + k)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=-1, poll_interval=16) as s:
        r = s.result(log=False)
        assert r.refactors == 1 and r.iterations == 0
        _, _, info = check(s, a, ns, "1 refactorisation", every_below=0, seed=k)
        assert info["neta"] == 0 and info["k"] == k
        assert s.run(48) == "iter_limit"
        check(s, a, ns, "1 refactorisation", every_below=0, seed=k + 1)
        s.refactor()
        r = s.result(log=False)
        assert r.refactors == 2 and r.iterations == 48
        _, _, info = check(s, a, ns, "1 refactorisation", every_below=0, seed=k + 2)
        assert info["neta"] == 0


@pytest.mark.parametrize("m,k", [(701, 449), (1037, 129)])
def test_refactorisation_with_another_row_stride(core, monkeypatch, m, k):
    """The same with the compact inverse's row stride changed (DZG_LDB_PAD): no kernel may assume it."""
    monkeypatch.setenv("DZG_LDB_PAD", "48")
    lp, a, ns = scattered_lp(core, m, k, seed=7100 + m + k)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=-1, poll_interval=16) as s:
        check(s, a, ns, "1 refactorisation", every_below=0, seed=k)
        assert s.run(48) == "iter_limit"
        s.refactor()
        check(s, a, ns, "1 refactorisation", every_below=0, seed=k + 1)


# ------------------------------------------------------------------ 2. eta file and flush
STOPS = (1, 63, 64, 65, 127, 128, 129, 200)


def _run_stops(s, a, ns, family, stops=STOPS, every_below=400):
    """Cumulative stops; the rows read at each (all of them on small LPs)."""
    done, seen = 0, []
    for stop in stops:
        status = s.run(stop - done)
        r = s.result(log=False)
        done = r.iterations
        seen.append((done, check(s, a, ns, family, every_below=every_below, seed=done)))
        if status != "iter_limit":
            break
    return seen


@pytest.mark.parametrize("poll", [5, 16, 50])
def test_eta_file_and_flush_from_the_slack_basis(core, monkeypatch, poll):
    """From the slack basis k grows by one per pivot, so every batch runs with the flush grid at its
    k_hint bound; stops after 1, 63, 64, 65, 127, 128, 129, 200 pivots cut the batches (poll 5, 16,
    50) around the flushes at 64 and 128.  The chain (default), the seven-launch iteration and the
    chain handing over at k = 24 (DZG_CHAIN_KCAP) must all hold B^-1 -- the same bits at every stop."""
    m, ns = 256, 512
    a, b, c = core.gen_dense_lp(seed=4242, m=m, n_struct=ns)
    a = np.asarray(a)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    runs = {}
    for variant in ("chain", "seven", "kcap"):
        if variant == "kcap":
            monkeypatch.setenv("DZG_CHAIN_KCAP", "24")
        opts = dict(seven_launches=1) if variant == "seven" else {}
        with core.Solver(lp, numerics=core.FAST, refactor_interval=-1, poll_interval=poll, **opts) as s:
            runs[variant] = _run_stops(s, a, ns, "2 eta file")
        monkeypatch.delenv("DZG_CHAIN_KCAP", raising=False)
    assert [it for it, _ in runs["chain"]] == list(STOPS)
    for variant in ("seven", "kcap"):
        assert [it for it, _ in runs[variant]] == list(STOPS)
        for (it, (rows, binv, _)), (_, (rows0, binv0, _)) in zip(runs[variant], runs["chain"]):
            assert np.array_equal(rows, rows0)
            assert np.array_equal(binv, binv0), (variant, it)


@pytest.mark.parametrize("seed,kind", [(9600, 1), (9601, 2), (9602, 1), (9603, 2), (9604, 0)])
@pytest.mark.parametrize("seven", [0, 1])
def test_eta_file_where_slacks_enter_and_leave(core, seed, kind, seven):
    """Integer and 0/1 LPs (tests/lp_families.py): slacks enter and leave the basis, so compact
    columns are appended and deleted (the last moves into the hole) between and across flushes."""
    from tests.lp_families import make_lp

    a, b, c = make_lp(seed, kind, 120, 200)
    a = np.asarray(a, dtype=np.float64)
    ns = a.shape[1]
    lp = core.CoreLP.from_inequality_form(a, b, c)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=-1, poll_interval=16,
                     seven_launches=seven) as s:
        _run_stops(s, a, ns, "2 eta file")
        r = s.result()
    entered = sum(1 for _, e, _, _ in r.pivots if e >= ns)
    assert entered > 0 or r.iterations < 64, "no slack entered: the family does not test deletes"


def test_eta_file_across_near_tie_stops(core):
    """A near-tie STOP ends a run before the ambiguous pivot (possibly between BTRAN and the pivot);
    the inverse at the stop, and after resuming, is B^-1 of the basis the result reports."""
    from tests.lp_families import make_lp

    a, b, c = make_lp(7001, 1, 30, 40)
    a = np.asarray(a, dtype=np.float64)
    ns = a.shape[1]
    lp = core.CoreLP.from_inequality_form(a, b, c)
    with core.Solver(lp, numerics=core.FAST, near_tie_action=core.NEAR_TIE_STOP, refactor_interval=-1,
                     poll_interval=16, max_iter=2000) as s:
        stops = 0
        while s.run(0) == "near_tie":
            check(s, a, ns, "2 eta file", seed=stops)
            stops += 1
            assert stops < 2000
        check(s, a, ns, "2 eta file", seed=stops)
    assert stops >= 1


# ------------------------------------------------------------------ 3. sparse basis
def _csc_lp(core, seed, m, per_col):
    ns = 5 * m // 2
    cp, ri, val, b, c = core.gen_sparse_lp(seed, m, ns, per_col)
    return core.CoreLP.from_csc(m, cp, ri, val, b, c), ic.Csc(m, cp, ri, val), ns


@pytest.mark.parametrize("m,per_col", [(60, 3), (150, 4), (256, 5), (1000, 6)])
@pytest.mark.parametrize("poll", [5, 16])
def test_sparse_basis_inverse_at_the_eta_stops(core, m, per_col, poll):
    """X = A[R, S]^-1 minus its etas (k_sparse.hip) and the basic slacks' rows e_r - A[r, S] X, at
    the stops of the dense family."""
    lp, a, ns = _csc_lp(core, 8100 + m, m, per_col)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=-1, poll_interval=poll) as s:
        _run_stops(s, a, ns, "3 sparse basis")


@pytest.mark.parametrize("m,per_col,interval", [(150, 4, 17), (1000, 3, 40)])
def test_sparse_basis_inverse_with_frequent_refactorisations(core, m, per_col, interval):
    lp, a, ns = _csc_lp(core, 8200 + m, m, per_col)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=interval, poll_interval=16) as s:
        _run_stops(s, a, ns, "3 sparse basis", stops=(30, 64, 111, 200, 300))
        assert s.result(log=False).refactors >= 2


def test_sparse_basis_inverse_after_a_warm_start(core):
    """A solver created on a non-slack basis (the state 150 pivots into a solve) factorises it."""
    lp, a, ns = _csc_lp(core, 8300, 256, 4)
    with core.Solver(lp, numerics=core.FAST, poll_interval=16) as s:
        s.run(150)
        mid = s.result(log=False)
    assert mid.dense_columns > 0
    with core.Solver(core.resumed_from(lp, mid), numerics=core.FAST, poll_interval=16) as s:
        r = s.result(log=False)
        assert r.refactors == 1
        check(s, a, ns, "3 sparse basis", recent_count=0)
        _run_stops(s, a, ns, "3 sparse basis", stops=(1, 64, 100))


def test_sparse_basis_inverse_with_dense_rows(core):
    """The dense-rows family of test_sparse_basis_with_dense_rows_reaches_the_highs_optimum: beyond
    1024 structural basics a dense row's slack row combines more rows of X than one LDS chunk."""
    import scipy.sparse as sp

    rng = np.random.default_rng(77)
    m, ns, per_col = 2200, 4000, 5
    rows = np.concatenate([np.sort(rng.choice(np.arange(2, m), per_col, replace=False)) for _ in range(ns)])
    cols = np.repeat(np.arange(ns), per_col)
    vals = rng.uniform(-1, 1, ns * per_col)
    a = sp.csc_matrix((vals, (rows, cols)), shape=(m, ns)).tolil()
    a[0, :] = rng.uniform(0.1, 1.0, ns)
    a[1, :] = rng.uniform(-1.0, 1.0, ns)
    a = sp.csc_matrix(a)
    a.sort_indices()
    x0, y0 = rng.uniform(0, 1, ns), rng.uniform(0, 1, m)
    b = a @ x0 + rng.uniform(0, 1, m)
    c = a.T @ y0 - rng.uniform(0, 1, ns)
    lp = core.CoreLP.from_csc(m, a.indptr, a.indices, a.data, b, c)
    ac = ic.Csc(m, a.indptr, a.indices, a.data)
    with core.Solver(lp, numerics=core.FAST, poll_interval=128) as s:
        for budget in (700, 0):  # 700 pivots in, then the end of the solve
            status = s.run(budget)
            r = s.result(log=False)
            dense_slacks = [int(p) for p in np.flatnonzero((r.basis == ns) | (r.basis == ns + 1))]
            check(s, ac, ns, "3 sparse basis", extra=dense_slacks, seed=budget)
    assert status == "optimal" and r.dense_columns > 1024


# ------------------------------------------------------------------ 4. row-sharded lockstep
@pytest.mark.parametrize("world,m,ns,replicate", [(2, 160, 420, False), (3, 200, 420, True),
                                                  (8, 160, 420, False)])
def test_row_sharded_inverse_is_the_single_gpu_one(core, world, m, ns, replicate):
    """Each rank keeps a slice of Binv0's rows (8 ranks on 160 rows: slices of 32, the last ranks
    own none).  After a flush and after a refactorisation the stitched slices must be the single-GPU
    inverse bit for bit, and B^-1."""
    from dantzig_amd.sharded import make_lockstep, run_lockstep

    a, b, c = core.gen_dense_lp(seed=43 + world, m=m, n_struct=ns)
    a = np.asarray(a)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    opts = dict(poll_interval=16, refactor_interval=100)
    single = core.Solver(lp, numerics=core.FAST, **opts)
    solvers = make_lockstep(lp, world, replicate=replicate, shard_rows=True, **opts)
    try:
        empty = 0
        for budget in (70, 40):  # 70: one flush at 64, 6 etas; 110: refactorised at 100
            assert single.run(budget) == run_lockstep(solvers, budget) == "iter_limit"
            rs = single.result(log=False)
            want, info = single.debug_inverse(0, m)
            assert info["rows"] == (0, m)
            parts = []
            for s in solvers:
                lo, hi = s.row_range()
                blk, inf = s.debug_inverse(lo, hi)
                assert inf["rows"] == (lo, hi) == s.row_range()
                assert (inf["k"], inf["neta"]) == (info["k"], info["neta"])
                empty += hi == lo
                parts.append(blk)
                outside = (hi, hi + 1) if hi < m else (lo - 1, lo)  # a row another rank owns
                with pytest.raises(core.DantzigAmdError):
                    s.debug_inverse(*outside)
            got = np.concatenate(parts)
            assert got.shape == want.shape
            assert np.array_equal(got, want), (budget, np.count_nonzero(got != want))
            assert np.array_equal(solvers[0].result(log=False).basis, rs.basis)
            ratio = ic.residual(want, np.arange(m), a, rs.basis, ns)
            WORST["4 row-sharded"] = max(WORST.get("4 row-sharded", 0.0), float(ratio.max()))
            assert ratio.max() <= ic.C_INVERSE["4 row-sharded"], ratio.max()
        assert single.result(log=False).refactors == 1
        assert world < 8 or empty > 0
    finally:
        single.close()
        for s in solvers:
            s.close()


def test_hook_refuses_strict(core):
    a, b, c = core.gen_dense_lp(seed=5, m=40, n_struct=80)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), numerics=core.STRICT) as s:
        with pytest.raises(core.DantzigAmdError):
            s.debug_inverse(0, 1)
