"""beta_t = W_t . a_j of the three-launch iteration, computed as four independent wave sums on four
workgroups (k_chain.hip: chain_beta, chain_beta_fetch; fast_rows.h: fast_beta_wave) instead of by
workgroup t alone.  No sum and no order of a sum changes, so every solve stays, bit for bit, the
seven-launch solve -- whose beta is still fast_beta_dot on one workgroup -- and the CPU oracle's pivots:

  * the two windows whose oracle logs are committed (config 2's first 4 000 pivots, the benchmark
    LP's first 597): chain == seven launches == batches of 7;
  * DZG_CHAIN_GRID = 8, 24, 100: several work items per workgroup, on different waves;
  * DZG_CHAIN_BETA_SPLIT=0, the A/B switch: workgroup t takes the four wave sums of eta t itself;
  * entering slacks while etas are pending: beta_t is then one entry of W_t, published in slot 4 t
    and taken verbatim, never routed through the sum;
  * a warm start at k > 512, where FTRAN's rows run 64 lanes per row behind the new beta.

Nothing a solve is compared against here is produced by the code under test."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PRIMAL, DUAL = 0, 1  # dzg_step_kind as the logs store it
RMAX = 64            # eta-file capacity: the host flushes it every 64 pivots


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


def _chain_runs_on(grid, m, q):
    """the engine's rule (one row and one column of a workgroup's share per thread, 512 threads)"""
    return (((m + grid - 1) // grid + 3) & ~3) <= 512 and (q + grid - 1) // grid <= 512


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


@pytest.fixture(scope="module")
def benchmark_lp(core):
    """the benchmark LP's first 597 pivots: the oracle's log and the seven-launch solve"""
    with open(os.path.join(GOLDEN, "oracle_blocked_pivots_1003_8192x16384.json")) as f:
        fx = json.load(f)
    seed, m, ns = 1003, 8192, 16384
    assert (int(fx["seed"]), int(fx["m"]), int(fx["n_struct"])) == (seed, m, ns)
    n = len(fx["kind"])
    assert n == 597
    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    seven = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50, seven_launches=1)
    log = dict(kind=fx["kind"], enter=fx["entering"], leave=fx["leaving"], mu=fx["mu"])
    return lp, n, ns, log, seven


def _is_the_oracles(r, n, log, mu_rtol):
    assert r.status == "iter_limit" and r.iterations == n and len(r.pivots) == n
    assert np.array_equal([p[0] for p in r.pivots], log["kind"])
    assert np.array_equal([p[1] for p in r.pivots], log["enter"])
    assert np.array_equal([p[2] for p in r.pivots], log["leave"])
    got, mu = np.array([p[3] for p in r.pivots]), np.asarray(log["mu"])
    assert np.all(np.abs(got - mu) <= mu_rtol * np.maximum(1.0, np.abs(mu)))


def test_config2_window_has_slacks_entering_on_pending_etas(config2):
    """From the fixture alone: 1 463 of the 4 000 pivots bring a slack in.  The eta file is flushed
    every 64 pivots, so at most ceil(4000 / 64) = 63 pivots of the window start with an empty file,
    whatever the phase of the flushes: at least 1 400 entering slacks take beta_t = W_t[row] from a
    pending eta -- the verbatim path of the split, in both kernels (both step kinds)."""
    _, n, ns, log, _ = config2
    es = np.asarray(log["enter"]) >= ns
    empty_at_most = (n + RMAX - 1) // RMAX
    assert int(es.sum()) == 1463 and empty_at_most == 63
    assert int(es.sum()) - empty_at_most >= 1400
    kind = np.asarray(log["kind"])
    assert int((es & (kind == PRIMAL)).sum()) - empty_at_most > 0
    assert int((es & (kind == DUAL)).sum()) - empty_at_most > 0


def test_config2_first_4000_pivots(core, config2):
    lp, n, _, log, seven = config2
    chain = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50)
    short = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=7)
    _is_the_oracles(seven, n, log, 1e-7)
    _is_the_oracles(chain, n, log, 1e-7)
    assert chain.dense_columns == 367 and chain.chain_fallbacks == 0
    assert _same_solve(chain, seven)
    assert _same_solve(short, seven)


def test_benchmark_lp_first_597_pivots(core, benchmark_lp):
    lp, n, _, log, seven = benchmark_lp
    chain = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50)
    short = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=7)
    _is_the_oracles(seven, n, log, 1e-9)
    _is_the_oracles(chain, n, log, 1e-9)
    assert chain.near_ties == 0 and chain.dense_columns == 89 and chain.chain_fallbacks == 0
    assert _same_solve(chain, seven)
    assert _same_solve(short, seven)


@pytest.mark.parametrize("grid", [8, 24, 100])
def test_config2_on_small_grids(core, config2, monkeypatch, grid):
    """4 neta work items on 8, 24 or 100 workgroups: up to 32 items per workgroup, handed to its
    waves in turn.  An item's bits depend on the item alone."""
    lp, n, _, log, seven = config2
    assert _chain_runs_on(grid, lp.m, len(lp.nonbasis))
    monkeypatch.setenv("DZG_CHAIN_GRID", str(grid))
    chain = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50)
    short = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=7)
    assert chain.chain_fallbacks == 0
    assert _same_solve(chain, seven), grid
    assert _same_solve(short, seven), grid
    _is_the_oracles(chain, n, log, 1e-7)


def test_benchmark_lp_on_a_grid_of_100(core, benchmark_lp, monkeypatch):
    """(8 and 24 workgroups cannot hold this LP's rows and columns one per thread: the engine would
    run the seven launches, and the test would compare them with themselves)"""
    lp, n, _, log, seven = benchmark_lp
    m, q = lp.m, len(lp.nonbasis)
    assert _chain_runs_on(100, m, q) and not _chain_runs_on(24, m, q) and not _chain_runs_on(8, m, q)
    monkeypatch.setenv("DZG_CHAIN_GRID", "100")
    chain = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50)
    assert chain.chain_fallbacks == 0
    assert _same_solve(chain, seven)
    _is_the_oracles(chain, n, log, 1e-9)


@pytest.mark.parametrize("grid", [None, 24])
def test_switch_off_is_the_same_solve(core, config2, benchmark_lp, monkeypatch, grid):
    """DZG_CHAIN_BETA_SPLIT=0: workgroup t computes the four wave sums of eta t itself and publishes
    the same four slots."""
    monkeypatch.setenv("DZG_CHAIN_BETA_SPLIT", "0")
    if grid is not None:
        monkeypatch.setenv("DZG_CHAIN_GRID", str(grid))
    lp, n, _, log, seven = config2
    chain = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50)
    short = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=7)
    assert _same_solve(chain, seven) and _same_solve(short, seven)
    _is_the_oracles(chain, n, log, 1e-7)
    if grid is None:
        lp, n, _, log, seven = benchmark_lp
        chain = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50)
        assert _same_solve(chain, seven)
        _is_the_oracles(chain, n, log, 1e-9)


@pytest.mark.parametrize("split", ["1", "0"])
def test_warm_start_past_k_512(core, monkeypatch, split):
    """From a basis of 600 structural columns FTRAN's rows take 64 lanes each (k > 512) behind the
    new beta: k moves by at most one per pivot, so it stays above 512 for all of the 85 pivots, which
    fill the eta file once and cross its flush.  Reference: the seven launches."""
    a, b, c = core.gen_dense_lp(seed=1002, m=1024, n_struct=2048)
    k0, n = 600, 85
    assert k0 - n > 512 and n > RMAX
    lp = core.warm_started(core.CoreLP.from_inequality_form(a, b, c), k0)
    seven = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50, seven_launches=1)
    assert seven.status == "iter_limit" and seven.iterations == n and seven.dense_columns > 512
    monkeypatch.setenv("DZG_CHAIN_BETA_SPLIT", split)
    chain = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50)
    short = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=7)
    assert chain.chain_fallbacks == 0
    assert _same_solve(chain, seven)
    assert _same_solve(short, seven)
