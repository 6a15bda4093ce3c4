"""k_price_rows_small after its rows stage was rebuilt (the row list fetched beside the control block,
a lane's offsets read from LDS in one batch, all row loads of a trip back to back, 16 bytes a lane with
a half-wave per row group): the sums and their order are unchanged, so a chain solve is bit for bit
the seven-launch solve, which prices the same pivots with k_price_rows<2> + k_price_rows_finish --
the same sums by other code.  Every case compares pivots, margins, x, xbar, z, zbar, basis and
nonbasis exactly, at poll intervals 50 and 7.

The windows are the smallest that reach each edge of the kernel: the group counts G = ceil((k + 1) /
16) at which the work is laid out differently (1 -> 2, 8 -> 9, 16 -> 17: the first half-wave with two
groups), the host's switches between the instantiations (k_hint = k + batch passing 127 and 255), the
cap of 480 where the pass is handed to k_price_rows and the fold, and the column edges (a last tile
that is not full, fewer than 64 columns, more tiles than CUs, more than two workgroups per CU can
hold: the 8-byte instantiation).  A window deep in the solve starts from the state the seven launches
reach there (core.resumed_from), which keeps both step kinds in it; a warm start would pivot primal
steps only.  What a window contains is read from the seven-launch log, not from the code under test.

The engine's row-major copy has a row stride that is a multiple of 4 and a base from hipMalloc, so
rows that are not 16-byte aligned cannot be produced through the API (dzg_price_small would hand
them to k_price_rows and its finish, the reference of these tests).  The kernel's guard (k beyond the
rule or the cap while the solve runs: DZG_PANIC) cannot be reached without a launch whose host bound
is wrong, and is not provoked here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PRIMAL, DUAL = 0, 1


@pytest.fixture(scope="module")
def core():
    from dantzig_amd import core as c

    return c


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same_solve(r, w):
    """logs, margins, x, xbar, z, zbar, basis, nonbasis equal exactly (tests/test_gpu_small_k_trips.py)"""
    return (r.status == w.status and r.iterations == w.iterations and r.pivots == w.pivots
            and all(np.array_equal(_bits(getattr(r, f)), _bits(getattr(w, f))) for f in ("x", "xbar", "z", "zbar"))
            and np.array_equal(_bits(r.margins), _bits(w.margins))
            and np.array_equal(r.basis, w.basis) and np.array_equal(r.nonbasis, w.nonbasis))


def _window(seven, k0, ns):
    """From the seven-launch log: the compact width k each pivot was priced at (a leaving slack
    appends a column of the compact inverse, an entering slack deletes one), and the counts of
    primal steps, dual steps, entering slacks and leaving slacks."""
    kind = np.array([p[0] for p in seven.pivots])
    es = np.array([p[1] for p in seven.pivots]) >= ns
    ls = np.array([p[2] for p in seven.pivots]) >= ns
    k_after = k0 + np.cumsum(ls.astype(np.int64) - es.astype(np.int64))
    k_at = np.concatenate([[k0], k_after[:-1]])
    assert int(k_after[-1]) == seven.dense_columns
    return k_at, (int((kind == PRIMAL).sum()), int((kind == DUAL).sum()), int(es.sum()), int(ls.sum()))


_reference = {}


def _case(core, m, ns, seed, prefix, n):
    """The LP after `prefix` pivots of the seven launches (0: the slack basis), the width k it has
    there and the seven-launch solve of the next n pivots; computed once per window, left unchanged."""
    key = (m, ns, seed, prefix, n)
    if key not in _reference:
        a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
        lp = core.CoreLP.from_inequality_form(a, b, c)
        k0 = 0
        if prefix > 0:
            pre = core.solve(lp, numerics=core.FAST, max_iter=prefix, poll_interval=50, seven_launches=1, log=False)
            assert pre.status == "iter_limit" and pre.iterations == prefix
            lp, k0 = core.resumed_from(lp, pre), pre.dense_columns
        seven = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50, seven_launches=1)
        assert seven.status == "iter_limit" and seven.iterations == n and len(seven.pivots) == n
        _reference[key] = (lp, k0, seven)
    return _reference[key]


def _chain_is_seven(core, lp, seven, n):
    chain = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=50)
    short = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=7)
    assert _same_solve(chain, seven)
    assert _same_solve(short, seven)


# 1024 x 2048, seed 1002 (config 2): rows_T = 0.93 m n_s / (m + n_s) = 634 > every k below.  Its
# oracle log (tests/golden/oracle_pivots_1002_1024x2048.npz) has k = 16 after pivot 29, 128 after 792,
# 205 / 248 / 256 after 1 718 / 2 280 / 2 412 and 480 after 6 030: the windows start a little before.
M, NS, SEED = 1024, 2048, 1002
# (pivots before the window, pivots of the window, values of k + 1 it must price at,
#  the bound of the host's switch that k + 50 and k + 7 must pass inside it)
WINDOWS = {
    "G 1 -> 2, 8 -> 9, k_hint passes 127": (0, 850, (16, 17, 128, 129), 127),
    "G 16 -> 17, k_hint passes 255": (1600, 900, (256, 257), 255),
    "the cap of 480": (5850, 300, (480, 481), None),
}


@pytest.mark.parametrize("name", list(WINDOWS))
def test_group_count_edges(core, name):
    prefix, n, widths, switch = WINDOWS[name]
    lp, k0, seven = _case(core, M, NS, SEED, prefix, n)
    k_at, counts = _window(seven, k0, NS)
    print(f"{name}: k {int(k_at.min())}..{int(k_at.max())}, primal/dual/entering slacks/leaving slacks {counts}")
    for w in widths:
        assert np.any(k_at + 1 == w), f"no pivot priced at k + 1 = {w}"
    # both step kinds, the extra row of a leaving slack, the reordered list after an entering slack
    assert min(counts) > 0
    if switch is not None:  # batches of 50 and of 7 on both sides of the host's bound
        assert np.any(k_at + 50 < switch) and np.any(k_at + 7 >= switch)
    _chain_is_seven(core, lp, seven, n)


# (m, n_s, seed, pivots): a last tile of 44 columns (ldt = 1004); one tile that is not full; 300 tiles
# on 256 CUs; 520 tiles, more than two workgroups per CU hold (the four-per-CU instantiation)
COLUMN_EDGES = {
    "ldt = 1004": (1024, 1001, 1002, 400),
    "50 columns": (1024, 50, 1002, 150),
    "300 tiles": (64, 64 * 300, 1002, 150),
    "520 tiles": (64, 64 * 520, 1002, 150),
}


@pytest.mark.parametrize("name", list(COLUMN_EDGES))
def test_column_edges(core, name):
    m, ns, seed, n = COLUMN_EDGES[name]
    rows_t = int(0.93 * m * ns / (m + ns))
    lp, _, seven = _case(core, m, ns, seed, 0, n)
    k_at, counts = _window(seven, 0, ns)
    print(f"{name}: rows_T {rows_t}, k {int(k_at.min())}..{int(k_at.max())}, "
          f"primal/dual/entering slacks/leaving slacks {counts}")
    assert int(k_at.max()) >= 16 and counts[3] > 0  # more than one row group; leaving slacks
    assert np.any(k_at < rows_t)                    # the row-wise pass priced pivots of the window
    _chain_is_seven(core, lp, seven, n)
