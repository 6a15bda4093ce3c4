"""The small-k pricing pass in k_chain_pre's tail (csrc/k_chain.hip, PRICE): every workgroup forms all
of BTRAN's compact row itself -- the eta rows from the kept compact copy d.wk -- and prices its column
tile behind it, two launches a pivot.  The arithmetic is the owner's and k_price_rows_small's, so a
solve is bit for bit the three-launch solve (DZG_CHAIN_PRICE_FUSED=0) and the seven-launch solve: every
case compares the pivot log (kind, entering, leaving, mu), the margins, x, xbar, z, zbar, basis and
nonbasis exactly, and reads the counters of dzg_debug_chain_price_counts to see which form ran.

What a window holds (the widths k it prices at, the four kinds of pivot: appending, deleting, both,
neither) is read from the seven-launch log, never from the code under test.  The deep windows start
from the state the seven launches reach there (core.resumed_from), as in
tests/test_gpu_price_small_one_trip.py, whose windows these are.

256 x 512 reaches k = 128 only after some 800 pivots (seed 1: pivot 814 by the CPU oracle), so the
first window is 900 pivots long; rows_T = 158 there, so batches of 50 leave the fused pass at k = 108
(k + 50 >= rows_T) and G = 8 -> 9 is priced in the tail at poll intervals 1 and 7."""
import numpy as np
import pytest

from dantzig_amd import _ffi

gpu = pytest.mark.gpu
PRIMAL, DUAL = 0, 1
CAP = 480  # dzg_price_small: k_hint < 480


@pytest.fixture(scope="module")
def core():
    from dantzig_amd import core as c

    return c


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same_solve(r, w):
    return (r.status == w.status and r.iterations == w.iterations and r.pivots == w.pivots
            and all(np.array_equal(_bits(getattr(r, f)), _bits(getattr(w, f))) for f in ("x", "xbar", "z", "zbar"))
            and np.array_equal(_bits(r.margins), _bits(w.margins))
            and np.array_equal(r.basis, w.basis) and np.array_equal(r.nonbasis, w.nonbasis))


def _window(seven, k0, ns):
    """From the seven-launch log: the width k each pivot was priced at, and how many pivots append a
    compact column only (a slack leaves), delete one only (a slack enters), do both, do neither."""
    es = np.array([p[1] for p in seven.pivots]) >= ns
    ls = np.array([p[2] for p in seven.pivots]) >= ns
    k_after = k0 + np.cumsum(ls.astype(np.int64) - es.astype(np.int64))
    k_at = np.concatenate([[k0], k_after[:-1]])
    assert int(k_after[-1]) == seven.dense_columns
    kinds = (int((ls & ~es).sum()), int((~ls & es).sum()), int((ls & es).sum()), int((~ls & ~es).sum()))
    return k_at, kinds


_reference = {}


def _case(core, m, ns, seed, prefix, n):
    """The LP after `prefix` seven-launch pivots (0: the slack basis), its width there and the
    seven-launch solve of the next n pivots; computed once per window, left unchanged."""
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


def _unfused(core, monkeypatch, lp, n, poll, **opts):
    """The three launches: DZG_CHAIN_PRICE_FUSED is read once, when the solver is created."""
    monkeypatch.setenv("DZG_CHAIN_PRICE_FUSED", "0")
    with core.Solver(lp, numerics=core.FAST, max_iter=n, poll_interval=poll, **opts) as s:
        monkeypatch.delenv("DZG_CHAIN_PRICE_FUSED")
        s.run(0)
        assert s.debug_chain_price_counts()[0] == 0
        return s.result()


def _fused(core, lp, n, poll, chunk=0, after_run=None, **opts):
    """The default form, run in chunks of `chunk` pivots (0: one run() call); after_run(solver) after
    each call.  Returns the result and the (fused, unfused) counters."""
    with core.Solver(lp, numerics=core.FAST, max_iter=n, poll_interval=poll, **opts) as s:
        done = 0
        while True:
            status = s.run(chunk)
            done += chunk
            if after_run is not None:
                after_run(s)
            if chunk == 0 or done >= n or status != "iter_limit":
                break
        return s.result(), s.debug_chain_price_counts()


def _wk_is_current(s):
    bad, valid = s.debug_wk_mismatch()
    assert valid and bad == 0, f"{bad} entries of the kept compact eta rows differ from W"


# ---- 256 x 512 from the slack basis: G 1 -> 2 and 8 -> 9, k_hint passes 127, several flushes
M0, NS0, SEED0, N0 = 256, 512, 1, 900


@gpu
@pytest.mark.parametrize("poll", [1, 7, 50])
def test_from_the_slack_basis(core, monkeypatch, poll):
    lp, _, seven = _case(core, M0, NS0, SEED0, 0, N0)
    k_at, kinds = _window(seven, 0, NS0)
    rows_t = int(0.93 * M0 * NS0 / (M0 + NS0))
    print(f"poll {poll}: k {int(k_at.min())}..{int(k_at.max())}, rows_T {rows_t}, "
          f"appending / deleting / both / neither {kinds}")
    assert min(kinds) > 0                                     # each of the four kinds of pivot occurs
    for w in (16, 17, 128, 129):                              # G = ceil((k + 1) / 16): 1 -> 2, 8 -> 9
        assert np.any(k_at + 1 == w), f"no pivot priced at k + 1 = {w}"
    assert np.any(k_at + poll < 127) and (poll == 50 or np.any(k_at + poll >= 127))
    assert N0 > 3 * 64                                        # several flushes of the eta file
    check = _wk_is_current if poll in (1, 7) else None
    got, (nf, nu) = _fused(core, lp, N0, poll, chunk=poll if check else 0, after_run=check)
    print(f"poll {poll}: fused {nf}, unfused {nu}")
    assert nf > 0 and nf + nu == N0
    if poll in (1, 7):
        assert nu == 0                                        # k + poll < rows_T for the whole window
    assert _same_solve(got, seven)
    assert _same_solve(_unfused(core, monkeypatch, lp, N0, poll), seven)


# ---- 1024 x 2048, seed 1002: the windows of tests/test_gpu_price_small_one_trip.py
M1, NS1, SEED1 = 1024, 2048, 1002


@gpu
def test_two_groups_a_half_wave(core, monkeypatch):
    """k 192 -> 264: G passes 16 -> 17 and the host switches to the tail with <2, 2, 16>."""
    prefix, n = 1600, 900
    lp, k0, seven = _case(core, M1, NS1, SEED1, prefix, n)
    k_at, kinds = _window(seven, k0, NS1)
    print(f"k {int(k_at.min())}..{int(k_at.max())}, appending / deleting / both / neither {kinds}")
    assert np.any(k_at + 1 == 256) and np.any(k_at + 1 == 257)
    for poll in (50, 7):
        assert np.any(k_at + poll < 255) and np.any(k_at + poll >= 255)
        got, (nf, nu) = _fused(core, lp, n, poll)
        assert (nf, nu) == (n, 0)
        assert _same_solve(got, seven)
    assert _same_solve(_unfused(core, monkeypatch, lp, n, 50), seven)


@gpu
def test_past_the_cap(core, monkeypatch):
    """k 461 -> 480 and beyond: a batch whose bound k + poll reaches the cap prices in a launch of its
    own (and from k + poll >= 512 on in k_price_rows): the fused counter grows by whole batches
    exactly while the bound is below the cap."""
    prefix, n, poll = 5850, 300, 7
    lp, k0, seven = _case(core, M1, NS1, SEED1, prefix, n)
    k_at, _ = _window(seven, k0, NS1)
    print(f"k {int(k_at.min())}..{int(k_at.max())}")
    assert np.any(k_at + poll < CAP) and np.any(k_at + poll >= CAP) and int(k_at[-1]) + poll >= CAP
    seen = []

    def note(s):
        seen.append(s.debug_chain_price_counts())

    got, (nf, nu) = _fused(core, lp, n, poll, chunk=poll, after_run=note)
    assert _same_solve(got, seven)
    before = (0, 0)
    for b, now in enumerate(seen):                            # batch b starts at pivot b * poll
        size = min(poll, n - b * poll)
        fused_batch = int(k_at[b * poll]) + size < CAP
        assert (now[0] - before[0], now[1] - before[1]) == ((size, 0) if fused_batch else (0, size)), b
        before = now
    assert nf > 0 and nu > 0 and seen[-1][0] == seen[-2][0]   # the counter has stopped growing
    assert _same_solve(_unfused(core, monkeypatch, lp, n, poll), seven)


# ---- column edges: a ragged last tile (ldt = 1004), one partial tile (50 columns)
@gpu
@pytest.mark.parametrize("name,m,ns,n", [("ldt = 1004", 1024, 1001, 400), ("50 columns", 1024, 50, 150)])
def test_column_edges(core, monkeypatch, name, m, ns, n):
    lp, _, seven = _case(core, m, ns, 1002, 0, n)
    k_at, kinds = _window(seven, 0, ns)
    rows_t = int(0.93 * m * ns / (m + ns))
    print(f"{name}: rows_T {rows_t}, k {int(k_at.min())}..{int(k_at.max())}, kinds {kinds}")
    assert int(k_at.max()) >= 16 and kinds[0] + kinds[2] > 0
    got, (nf, nu) = _fused(core, lp, n, 7)
    print(f"{name}: fused {nf}, unfused {nu}")
    assert nf > 0 and nf + nu == n
    # (a batch is fused while its bound k + batch stays below rows_T, where the row-wise pass ends)
    assert nf == sum(min(7, n - b) for b in range(0, n, 7) if int(k_at[b]) + min(7, n - b) < min(rows_t, CAP))
    assert _same_solve(got, seven)
    assert _same_solve(_unfused(core, monkeypatch, lp, n, 7), seven)


@gpu
def test_more_tiles_than_workgroups_stays_unfused(core, monkeypatch):
    """300 tiles on a chain grid of at most 256 workgroups: a workgroup looping over tiles would
    serialise their row trips, so the pass keeps its own launch."""
    m, ns, n = 64, 64 * 300, 150
    lp, _, seven = _case(core, m, ns, 1002, 0, n)
    got, (nf, nu) = _fused(core, lp, n, 50)
    assert (nf, nu) == (0, n)
    assert _same_solve(got, seven)
    assert _same_solve(_unfused(core, monkeypatch, lp, n, 50), seven)


# ---- timing: a slot whose pricing pass is timed runs the three launches
@gpu
def test_timed_slots_keep_their_launch(core, monkeypatch):
    lp, _, seven = _case(core, M0, NS0, SEED0, 0, N0)
    n, poll = 400, 40                                         # ten whole batches, k + 40 < rows_T throughout
    k_at, _ = _window(seven, 0, NS0)
    assert int(k_at[:n].max()) + poll < int(0.93 * M0 * NS0 / (M0 + NS0))
    ref = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=poll, seven_launches=1)
    got, (nf, nu) = _fused(core, lp, n, poll, profile=(1 << _ffi.K_PRICE) | (8 << 16))
    assert (nf, nu) == (7 * n // 8, n // 8)                   # every 8th slot of a batch is timed
    assert got.kernel_launches["price"] == nu
    assert _same_solve(got, ref)
    allc, (nf, nu) = _fused(core, lp, n, poll, profile=-1)    # every class, every slot
    assert (nf, nu) == (0, n)
    assert _same_solve(allc, ref)
    assert _same_solve(_unfused(core, monkeypatch, lp, n, poll), ref)
    assert _same_solve(_unfused(core, monkeypatch, lp, n, poll, profile=(1 << _ffi.K_PRICE) | (8 << 16)), ref)


# ---- the validity flag: cleared between two run() calls, the next batch gathers again
@gpu
def test_regather_after_the_flag_is_cleared(core, monkeypatch):
    lp, _, seven = _case(core, M0, NS0, SEED0, 0, N0)
    n, poll = 300, 7
    ref = core.solve(lp, numerics=core.FAST, max_iter=n, poll_interval=poll, seven_launches=1)
    with core.Solver(lp, numerics=core.FAST, max_iter=n, poll_interval=poll) as s:
        assert s.run(100) == "iter_limit"                     # (100 = 64 + 36: pending etas in W)
        bad, valid = s.debug_wk_mismatch(clear_valid=True)
        assert valid and bad == 0
        assert s.debug_wk_mismatch() == (0, False)
        s.run(0)
        bad, valid = s.debug_wk_mismatch()
        assert valid and bad == 0                             # gathered again, and kept current since
        assert s.debug_chain_price_counts() == (n, 0)
        assert _same_solve(s.result(), ref)
    assert _same_solve(_unfused(core, monkeypatch, lp, n, poll), ref)


# ---- the host's rule, without a device
def test_host_rule():
    rule = _ffi.lib().dzg_debug_chain_price_rule
    m, q = 8192, 16384
    for grid in (1, 8, 200, 256):
        per = ((m + grid - 1) // grid + 3) & ~3               # chain_rows: the one-pass narrow kernel holds 32
        for tiles in (0, 1, grid - 1, grid, grid + 1, 300, 1024):
            for k_hint in (0, 1, 126, 127, 254, 255, 479, 480, 512, 513, 5000):
                for timed in (0, 1):
                    for small in (0, 1):
                        want = int(bool(small and not timed and 1 <= tiles <= grid and tiles * 512 >= q
                                        and 0 < k_hint < CAP and per <= 32))
                        assert rule(m, grid, k_hint, tiles, q, small, timed) == want, (grid, tiles, k_hint, timed, small)
    # every nonbasic position needs a pricing workgroup; four passes of rows do not leave the threads
    assert rule(8192, 256, 100, 256, 256 * 512, 1, 0) == 1 and rule(8192, 256, 100, 256, 256 * 512 + 1, 1, 0) == 0
    assert rule(8192, 256, 100, 32, 2048, 1, 0) == 1 and rule(8196, 256, 100, 32, 2048, 1, 0) == 0
