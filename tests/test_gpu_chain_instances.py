"""The chain kernels' instantiations (k_chain.hip: MAXP register-held FTRAN passes, NARROW = 16 lanes
per row only, NOFOLD = no fold head and no many-candidates path) and the host rule that picks one per
launch (chain_pick, through dzg_debug_chain_instance).  An instantiation only lacks code its launch
cannot reach: no sum, order or barrier changes, so every solve stays, bit for bit, the seven-launch
solve -- whose FTRAN does not go through k_chain.hip -- and the CPU oracle's pivots.

  * config 2's first 4 000 pivots (1024 x 2048, seed 1002, k reaches 367) on grids of 32, 24, 8 and
    100 workgroups: 32 rows per workgroup (the one-pass kernel filled exactly, the benchmark's own
    case), 44 (two passes: one more than it covers), 128 (four passes exactly), 12 (a part-filled
    pass, and workgroups past the last row that own nothing);
  * poll intervals of 7 and 50: the host's bound on k, and with it the pick, changes between batches;
  * DZG_CHAIN_INSTANCES=0, the A/B switch: the generic kernels always;
  * a warm start below k = 512 that crosses it inside the run: the batches hand over from the narrow
    kernels to the generic ones, with the fold head on and with DZG_CHAIN_NO_FOLD=1;
  * the rule itself over a grid of shapes (host code, no GPU).

Nothing a solve is compared against here is produced by the code under test."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def core():
    from dantzig_amd import core as c

    return c


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same_solve(r, w):
    """logs, x, xbar, z, zbar, basis, nonbasis equal exactly"""
    return (r.status == w.status and r.iterations == w.iterations and r.pivots == w.pivots
            and all(np.array_equal(_bits(getattr(r, f)), _bits(getattr(w, f))) for f in ("x", "xbar", "z", "zbar"))
            and np.array_equal(_bits(r.margins), _bits(w.margins))
            and np.array_equal(r.basis, w.basis) and np.array_equal(r.nonbasis, w.nonbasis))


def _rows_per_workgroup(grid, m):
    return ((m + grid - 1) // grid + 3) & ~3  # chain_rows


def _chain_runs_on(grid, m, q):
    """the engine's rule (one row and one column of a workgroup's share per thread, 512 threads)"""
    return _rows_per_workgroup(grid, m) <= 512 and (q + grid - 1) // grid <= 512


@pytest.fixture(scope="module")
def config2(core):
    """config 2's first 4 000 pivots: the oracle's log and the seven-launch solve"""
    n = 4000
    fx = np.load(os.path.join(GOLDEN, "oracle_pivots_1002_1024x2048.npz"))
    seed, m, ns = int(fx["seed"]), int(fx["m"]), int(fx["n_struct"])
    assert (seed, m, ns) == (1002, 1024, 2048) and int(fx["iterations"]) > n
    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    seven = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50, seven_launches=1)
    log = dict(kind=fx["kind"][:n], enter=fx["entering"][:n], leave=fx["leaving"][:n], mu=fx["mu"][:n])
    return lp, n, ns, log, seven


def _is_the_oracles(r, n, log, mu_rtol):
    assert r.status == "iter_limit" and r.iterations == n and len(r.pivots) == n
    assert np.array_equal([p[0] for p in r.pivots], log["kind"])
    assert np.array_equal([p[1] for p in r.pivots], log["enter"])
    assert np.array_equal([p[2] for p in r.pivots], log["leave"])
    got, mu = np.array([p[3] for p in r.pivots]), np.asarray(log["mu"])
    assert np.all(np.abs(got - mu) <= mu_rtol * np.maximum(1.0, np.abs(mu)))


# ---- what dzg_debug_chain_instance returns (include/dantzig_amd.h)
def _pick(m, grid, k_bound, fold, nrz, shard=0, post=1):
    from dantzig_amd import _ffi

    v = _ffi.lib().dzg_debug_chain_instance(m, grid, k_bound, fold, nrz, shard, post)
    return v & 0xFF, bool(v & 0x100), bool(v & 0x200)  # passes, narrow, nofold


GENERIC = (16, False, False)
# the specialised kernels that exist: (passes, narrow, nofold); the no-fold one is k_chain_post's
PRE_KERNELS = [(1, True, False), (4, True, False), (4, False, False)]
POST_KERNELS = [(1, True, True), (4, True, False), (4, False, False)]


def _passes_needed(m, grid, narrow):
    """a pass covers 8 waves x (64 / LPR) rows; 16 lanes per row only while k <= 512 for certain"""
    per = _rows_per_workgroup(grid, m)
    rows = 8 * (4 if narrow else 1)
    return (per + rows - 1) // rows


def test_the_rule_never_picks_a_kernel_that_lacks_what_the_launch_needs():
    """Host code only (the library loads without a device)."""
    seen = set()
    for m in (1, 7, 48, 1000, 1024, 4096, 8192, 8193, 32768, 131072):
        for grid in (1, 8, 24, 32, 100, 255, 256):
            for k_bound in (0, 1, 76, 462, 511, 512, 513, 600, 4096):
                for fold in (0, 1):
                    for nrz in (0, 64, 256, 257, 4096):
                        for post in (0, 1):
                            got = _pick(m, grid, k_bound, fold, nrz, 0, post)
                            passes, narrow, nofold = got
                            seen.add((post,) + got)
                            assert got == GENERIC or got in (POST_KERNELS if post else PRE_KERNELS)
                            if k_bound == 0 or k_bound > 512:
                                assert not narrow
                            if k_bound == 0:
                                assert got == GENERIC
                            if fold == 1 or nrz > 256:
                                assert not nofold
                            known_narrow = 0 < k_bound <= 512
                            covering = [c for c in (POST_KERNELS if post else PRE_KERNELS)
                                        if k_bound > 0 and (not c[1] or known_narrow)
                                        and (not c[2] or (fold == 0 and nrz <= 256))
                                        and c[0] >= _passes_needed(m, grid, known_narrow)]
                            if covering:
                                assert got != GENERIC and passes == min(c[0] for c in covering)
                                assert passes >= _passes_needed(m, grid, known_narrow)
                            else:
                                assert got == GENERIC
                            # a column-sharded rank has no specialised twins
                            assert _pick(m, grid, k_bound, fold, nrz, 1, post) == GENERIC
    # every kernel is reachable
    assert {(0,) + k for k in PRE_KERNELS} | {(1,) + k for k in POST_KERNELS} | {(0,) + GENERIC, (1,) + GENERIC} == seen


def test_the_rule_on_the_shapes_this_project_runs():
    # the benchmark's timed region and config 2's start: 32 rows per workgroup, k < 480, fused pricing
    assert _pick(8192, 256, 76, 0, 64, post=0) == (1, True, False)
    assert _pick(8192, 256, 76, 0, 64, post=1) == (1, True, True)
    assert _pick(1024, 32, 50, 0, 64, post=1) == (1, True, True)
    assert _pick(1024, 24, 50, 0, 64, post=1) == (4, True, False)     # 44 rows: two passes
    assert _pick(1024, 8, 50, 0, 64, post=1) == (4, True, False)      # 128 rows: four passes
    assert _pick(1024, 100, 50, 0, 64, post=1) == (1, True, True)     # 12 rows
    assert _pick(32768, 256, 100, 0, 64, post=1) == (4, True, False)  # config 5: 128 rows per workgroup
    assert _pick(8192, 256, 500, 1, 256, post=1) == (4, True, False)  # fold on: no no-fold kernel
    assert _pick(8192, 256, 513, 1, 256, post=1) == (4, False, False)  # the late regime: 32 rows, 64 lanes each
    assert _pick(8192, 256, 513, 1, 256, post=0) == (4, False, False)
    assert _pick(32768, 256, 600, 1, 256, post=1) == GENERIC          # 128 rows at 64 lanes: 16 passes
    assert _pick(8192, 256, 0, 0, 64, post=1) == GENERIC              # nobody refreshed the bound


# ---- the solves
@pytest.mark.gpu
@pytest.mark.parametrize("grid,rows,passes", [(32, 32, 1), (24, 44, 2), (8, 128, 4), (100, 12, 1)])
def test_config2_on_grids_that_fill_the_instantiations(core, config2, monkeypatch, grid, rows, passes):
    lp, n, _, log, seven = config2
    m, q = lp.m, len(lp.nonbasis)
    assert _chain_runs_on(grid, m, q)
    assert _rows_per_workgroup(grid, m) == rows and _passes_needed(m, grid, True) == passes
    if grid == 100:
        assert (grid - 1) * rows >= m  # the last workgroups own no row
    got = _pick(m, grid, 50, 0, 64, post=0)
    assert got[0] >= passes and (got[0] == 1) == (passes == 1)  # 44 rows: not the one-pass kernel
    monkeypatch.setenv("DZG_CHAIN_GRID", str(grid))
    chain = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50)
    assert chain.chain_fallbacks == 0 and chain.dense_columns == 367
    assert _same_solve(chain, seven), grid
    _is_the_oracles(chain, n, log, 1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("poll", [7, 50])
def test_config2_default_grid_by_poll_interval(core, config2, poll):
    """The bound on k is ncompact + the batch's pivots: another batch size, other batches narrow."""
    lp, n, _, log, seven = config2
    chain = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=poll)
    assert chain.chain_fallbacks == 0
    assert _same_solve(chain, seven), poll
    _is_the_oracles(chain, n, log, 1e-7)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [32, 8])
def test_switch_off_is_the_same_solve(core, config2, monkeypatch, grid):
    """DZG_CHAIN_INSTANCES=0: the generic kernels run every launch."""
    lp, n, _, log, seven = config2
    monkeypatch.setenv("DZG_CHAIN_GRID", str(grid))
    on = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50)
    monkeypatch.setenv("DZG_CHAIN_INSTANCES", "0")
    off = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50)
    assert on.chain_fallbacks == 0 and off.chain_fallbacks == 0
    assert _same_solve(off, seven) and _same_solve(on, seven) and _same_solve(on, off)
    _is_the_oracles(off, n, log, 1e-7)


WARM_K0, WARM_N, WARM_POLL = 500, 250, 7


@pytest.fixture(scope="module")
def warm(core):
    """config 2 from a basis of WARM_K0 structural columns; reference: the seven launches"""
    a, b, c = core.gen_dense_lp(seed=1002, m=1024, n_struct=2048)
    lp = core.warm_started(core.CoreLP.from_inequality_form(a, b, c), WARM_K0)
    seven = core.solve(lp, numerics=core.FAST, max_iter=WARM_N, poll_interval=50, seven_launches=1)
    return lp, seven


@pytest.mark.gpu
@pytest.mark.parametrize("no_fold", ["0", "1"])
def test_warm_start_that_crosses_k_512(core, warm, monkeypatch, no_fold):
    """The first batch is narrow for certain (k0 + the batch's pivots <= 512), the reference ends
    above 512 columns and k moves by at most one per pivot: some batch boundary hands over from the
    narrow kernels to the ones with 64 lanes per row, and every pivot on either side is the seven
    launches' pivot."""
    lp, seven = warm
    assert WARM_K0 + WARM_POLL <= 512
    assert seven.status == "iter_limit" and seven.iterations == WARM_N and seven.dense_columns > 512
    assert _pick(lp.m, 256, WARM_K0 + WARM_POLL, 1, 256)[1] and not _pick(lp.m, 256, seven.dense_columns, 1, 256)[1]
    monkeypatch.setenv("DZG_CHAIN_NO_FOLD", no_fold)
    chain = core.solve(lp, numerics=core.FAST, max_iter=WARM_N, poll_interval=WARM_POLL)
    assert chain.chain_fallbacks == 0
    assert _same_solve(chain, seven)
    long_batches = core.solve(lp, numerics=core.FAST, max_iter=WARM_N, poll_interval=50)
    assert long_batches.chain_fallbacks == 0
    assert _same_solve(long_batches, seven)
