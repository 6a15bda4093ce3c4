"""The argmax reductions of the three-launch iteration at small k in their straight-line form
(common.h: dzg_wave_best2_flat; k_chain.hip: chain_spec_reduce, chain_best, chain_best_pair,
chain_reduce_sc1; k_price_rows_small's publish step).  The form is the fold of dzg_better2 bit for bit,
so every solve stays the seven-launch solve -- whose kernels keep the shuffle butterfly -- and the CPU
oracle's pivots:

  * a 256 x 512 LP solved to the end at the default grid (a share of 4 rows and 2 columns per
    workgroup) and at DZG_CHAIN_GRID = 8 (32 rows, 64 columns: one wave reduces both sides together),
    4 (64 rows in one wave, 128 columns through the two-stage block form), 2 and 1 (both sides through
    the block form; up to 512 candidates per workgroup);
  * the first 597 pivots of the benchmark LP against the committed oracle log at the default grid:
    k_price_rows_small and the reduces of 256 workgroup candidates at their real counts.

Nothing a solve is compared against here is produced by the code under test."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
M, NS, SEED = 256, 512, 1002


@pytest.fixture(scope="module")
def core():
    from dantzig_amd import core as c

    return c


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same_solve(r, w):
    """logs, margins, x, xbar, z, zbar, basis, nonbasis equal exactly"""
    return (r.status == w.status and r.iterations == w.iterations and r.pivots == w.pivots
            and all(np.array_equal(_bits(getattr(r, f)), _bits(getattr(w, f))) for f in ("x", "xbar", "z", "zbar"))
            and np.array_equal(_bits(r.margins), _bits(w.margins))
            and np.array_equal(r.basis, w.basis) and np.array_equal(r.nonbasis, w.nonbasis))


def _share(grid, m, q):
    """rows and columns of a workgroup's share (chain_rows, chain_cols of k_chain.hip)"""
    return ((m + grid - 1) // grid + 3) & ~3, (q + grid - 1) // grid


@pytest.fixture(scope="module")
def small_lp(core):
    a, b, c = core.gen_dense_lp(seed=SEED, m=M, n_struct=NS)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    seven = core.solve(lp, numerics=core.FAST, poll_interval=50, seven_launches=1)
    assert seven.status == "optimal" and seven.iterations > 200
    return lp, seven


def test_small_lp_to_the_end_default_grid(core, small_lp):
    lp, seven = small_lp
    chain = core.solve(lp, numerics=core.FAST, poll_interval=50)
    short = core.solve(lp, numerics=core.FAST, poll_interval=7)
    assert chain.chain_fallbacks == 0
    assert _same_solve(chain, seven)
    assert _same_solve(short, seven)


@pytest.mark.parametrize("grid", [8, 4, 2, 1])
def test_small_lp_to_the_end_on_small_grids(core, small_lp, monkeypatch, grid):
    """both paths of chain_best: a share of at most 64 candidates is reduced by wave 0 alone, a larger
    one by the workgroup in two stages"""
    lp, seven = small_lp
    rows, cols = _share(grid, lp.m, len(lp.nonbasis))
    assert rows <= 512 and cols <= 512  # (the engine runs the chain)
    assert {8: (True, True), 4: (True, False), 2: (False, False), 1: (False, False)}[grid] == (rows <= 64, cols <= 64)
    monkeypatch.setenv("DZG_CHAIN_GRID", str(grid))
    chain = core.solve(lp, numerics=core.FAST, poll_interval=50)
    assert chain.chain_fallbacks == 0
    assert _same_solve(chain, seven), grid


def test_benchmark_lp_first_597_pivots_are_the_oracles(core):
    with open(os.path.join(GOLDEN, "oracle_blocked_pivots_1003_8192x16384.json")) as f:
        fx = json.load(f)
    seed, m, ns = 1003, 8192, 16384
    assert (int(fx["seed"]), int(fx["m"]), int(fx["n_struct"])) == (seed, m, ns)
    n = len(fx["kind"])
    assert n == 597
    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    r = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50)
    assert r.status == "iter_limit" and r.iterations == n and len(r.pivots) == n
    assert r.near_ties == 0 and r.dense_columns == 89 and r.chain_fallbacks == 0
    assert np.array_equal([p[0] for p in r.pivots], fx["kind"])
    assert np.array_equal([p[1] for p in r.pivots], fx["entering"])
    assert np.array_equal([p[2] for p in r.pivots], fx["leaving"])
    got, mu = np.array([p[3] for p in r.pivots]), np.asarray(fx["mu"])
    assert np.all(np.abs(got - mu) <= 1e-9 * np.maximum(1.0, np.abs(mu)))
