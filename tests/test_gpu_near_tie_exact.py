"""FAST's near-tie flags and margins against exact arithmetic (near-tie arbitration).

AUTO rests on: a decision FAST takes differently from the reference is flagged.  Here the flagged set F
and the pivot log come from FAST; everything they are compared with comes from tests/exact_shadow.py,
which follows FAST's own log in `fractions.Fraction` (integer LPs: a tie is an equality of fractions).
For every pivot j the shadow reached:

  A  delicate (exact tie, primal = dual, a zero ybar that can matter, a zero ratio-test denominator)
     => j in F; a first tie between bit-identical twins has margins[j] == 0.0
  B  j not in F => FAST's (kind, entering, leaving) is the unique exact decision
  C  j in F => delicate, or exact margin <= 1e-6, or the optimality test is at its threshold
  D  j not in F => |margins[j] - M_j| <= 1e-9, and margins[j] == inf <=> M_j == inf
  E  the run's end: an unflagged verdict is the exact one, a delicate one is booked, and
     min_margin == min(margins) with the terminal margin included

One deviation from "every zero ybar is delicate": an entry with ybar = 0 exactly, y > 0 and a real
candidate on its side cannot change what the reference does (it is no candidate there, or one with a
hugely negative ratio); dzg_first_pivot_entry lets it stand aside and fast_status flags it only when
it is its side's best.  Such pivots are checked as unflagged ones (B, D) and counted in the tally.

The groups of LPs and what they hold are asserted on the CPU in tests/test_exact_shadow_host.py.
Run with -s for the per-path tallies.
"""
import numpy as np
import pytest

from tests import exact_shadow as es
from tests.lp_families import log3

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def core():
    from dantzig_amd import core as c

    return c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def solve_stop_resume(core, lp, cap, **opts):
    """The LP in NEAR_TIE_STOP, every stop resumed: (result, F)."""
    flagged = set()
    with core.Solver(lp, numerics=core.FAST, near_tie_action=core.NEAR_TIE_STOP, max_iter=cap, **opts) as s:
        status = s.run(0)
        while status == "near_tie":
            it = s.result(log=False).iterations
            assert it not in flagged and len(flagged) <= cap, "a resumed stop did not move on"
            flagged.add(it)
            status = s.run(0)
        return s.result(), flagged


def check_end(tally, tag, run, r, flagged):
    """Claim E on a run that ended by itself (not at the iteration budget)."""
    fail = tally.failures.append
    n = len(r.pivots)
    floor = float(r.margins.min()) if n else np.inf
    if r.status == "iter_limit" or run.terminal is None:
        if run.terminal is not None and not r.min_margin == floor:
            fail(f"{tag}: E min_margin {r.min_margin!r} is not min(margins) {floor!r}")
        return
    t = run.terminal
    tally.terminals += 1
    if n not in flagged:
        if t.must_flag:
            fail(f"{tag}: E delicate verdict {t.verdict} {sorted(t.reasons)} after pivot {n} not booked")
        elif r.status != t.verdict:
            fail(f"{tag}: E unflagged status {r.status} against exact {t.verdict}")
        elif t.margin == es.INF or t.verdict == "optimal":
            # (an optimal verdict's margin is the optimality test's alone: inf outside its threshold)
            if not r.min_margin == floor:
                fail(f"{tag}: E min_margin {r.min_margin!r} is not min(margins) {floor!r}")
        elif abs(r.min_margin - min(floor, float(t.margin))) > es.MARGIN_AGREES_TO:
            fail(f"{tag}: E min_margin {r.min_margin!r} against min(margins, terminal) "
                 f"{min(floor, float(t.margin))!r}")
    elif not (t.delicate or t.margin <= es.NO_SPURIOUS_ABOVE or t.opt_edge):
        fail(f"{tag}: E/C verdict {r.status} flagged, exact margin {float(t.margin):.3e}, not delicate")
    if not r.min_margin <= floor:
        fail(f"{tag}: E min_margin {r.min_margin!r} above min(margins) {floor!r}")


def check_count_run(tally, tag, run, r, flagged, k):
    """The same LP counting instead of stopping (k) against STOP + resume (r, F): the same status, log
    and margins bit for bit, near_ties == |F| and first_near_tie == min F.  Two things the code defines:

    * a run that ends singular or in a panic at a flagged iteration chose that pivot and never
      executed it, and took no verdict: nothing books it, so near_ties is |F| - 1 there (AUTO hands
      such an end to STRICT whatever the counters say);
    * once FAST has pivoted on an element that is exactly zero (the shadow stopped), its state is
      rounding noise, the health monitor sees a pivot error near 1, and WHEN it refactorises depends on
      the poll boundaries, which every resumed run() shifts.  From there on the two runs may part;
      up to and including that pivot they may not.  Returns 1 for an LP where they did."""
    fail = tally.failures.append
    lr, lk = log3(r.pivots), log3(k.pivots)
    mr = _bits(r.margins if r.iterations else [])
    mk = _bits(k.margins if k.iterations else [])
    same = (k.status, lk) == (r.status, lr) and np.array_equal(mr, mk)
    if k.first_near_tie != min(flagged, default=-1):
        fail(f"{tag}: COUNT first_near_tie {k.first_near_tie}, F = {sorted(flagged)}")
    if same:
        unbooked = int(r.status in ("singular", "panic") and len(lr) in flagged)
        # (a panic taken by status() itself -- no candidate on either side -- is a verdict and is booked)
        if len(flagged) - k.near_ties not in ((0, 1) if unbooked and r.status == "panic" else (unbooked,)):
            fail(f"{tag}: COUNT near_ties {k.near_ties}, status {k.status}, F = {sorted(flagged)}")
        return 0
    n = min(len(lr), len(lk))
    d = next((i for i in range(n) if lr[i] != lk[i] or mr[i] != mk[i]), n)
    if run.stopped_at is None or d <= run.stopped_at:
        fail(f"{tag}: COUNT ({k.status}, {len(lk)} pivots) and STOP + resume ({r.status}, {len(lr)} pivots) "
             f"part at pivot {d}; first exactly zero pivot element at {run.stopped_at}")
    return 1


def solver_path(core, name, make_lp, **opts):
    """Claims A-E for one way of running core.Solver over the "solver" group."""
    tally, cap, parted = es.Tally(), es.GROUPS["solver"]["cap"], 0
    for tag, a, b, c in es.group_lps("solver"):
        lp = make_lp(core, a, b, c)
        r, flagged = solve_stop_resume(core, lp, cap, **opts)
        run = es.check_log(tally, tag, a, b, c, log3(r.pivots), r.margins if r.margins is not None else [],
                           flagged)
        if run.stopped_at is None:
            check_end(tally, tag, run, r, flagged)
        # the same LP, counting instead of stopping: the same log, and the counters are F's
        k = core.solve(lp, numerics=core.FAST, near_tie_action=core.NEAR_TIE_COUNT, max_iter=cap, **opts)
        parted += check_count_run(tally, tag, run, r, flagged, k)
    print("\n" + tally.line(name) + f"; LPs where COUNT and STOP + resume part after a zero pivot element {parted}")
    assert not tally.failures, f"{len(tally.failures)} failures:\n" + "\n".join(tally.failures[:40])
    assert tally.delicate >= 40 and tally.unflagged >= 150
    assert tally.twin_zero >= 4


def dense(core, a, b, c):
    return core.CoreLP.from_inequality_form(a, b, c)


def csc(core, a, b, c):
    import scipy.sparse as sp

    m = sp.csc_matrix(a)
    m.eliminate_zeros()
    m.sort_indices()
    return core.CoreLP.from_csc(a.shape[0], m.indptr, m.indices, m.data, b, c)


# ---------------------------------------------------------------------------- 1-3: dense, one LP
@pytest.mark.parametrize("poll", [1, 16])
def test_chain_kernels_against_exact_arithmetic(core, poll):
    """The default chain kernels (small-k forms at these sizes, pricing in k_chain_pre's tail)."""
    solver_path(core, f"chain, poll_interval {poll}", dense, poll_interval=poll)


@pytest.mark.parametrize("poll", [1, 16])
def test_seven_launches_against_exact_arithmetic(core, poll):
    solver_path(core, f"seven launches, poll_interval {poll}", dense, poll_interval=poll, seven_launches=1)


@pytest.mark.parametrize("grid", [8, 24])
def test_small_chain_grid_against_exact_arithmetic(core, monkeypatch, grid):
    """Row and column shares of a few entries per workgroup: twins 1 and 2 places apart fall on the two
    sides of a share's end, twins ns/2 apart into different workgroups."""
    monkeypatch.setenv("DZG_CHAIN_GRID", str(grid))
    solver_path(core, f"chain on {grid} workgroups", dense, poll_interval=16)


# ---------------------------------------------------------------------------- 4: sparse-basis path
@pytest.mark.parametrize("fused", ["1", "0"])
def test_sparse_basis_path_against_exact_arithmetic(core, monkeypatch, fused):
    monkeypatch.setenv("DZG_SP_FUSED", fused)
    solver_path(core, f"CSC, DZG_SP_FUSED={fused}", csc, poll_interval=16)


# ---------------------------------------------------------------------------- 5: the batch solver
@pytest.mark.parametrize("name", ["batch16", "batch32", "batch64", "batch72"])
def test_batch_fast_against_exact_arithmetic(core, name):
    """One call per row bucket, STOP and COUNT.  The batch's stop is not resumed: STOP gives each LP's
    first flagged pivot i; pivots [0, i) are checked as unflagged, pivot i as flagged; COUNT must put
    its first near tie at i with the same log and margins, bit for bit, before it.  refactor_every = 2:
    a rebuild of the in-LDS inverse falls inside the longer prefixes."""
    tally, cap = es.Tally(), es.GROUPS[name]["cap"]
    group = es.group_lps(name)
    lps = [dense(core, a, b, c) for _, a, b, c in group]
    opts = dict(numerics=core.FAST, max_iter=cap, refactor_every=2, log_cap=cap)
    stop = core.solve_batch_fast(lps, near_tie_action=core.NEAR_TIE_STOP, **opts)
    count = core.solve_batch_fast(lps, near_tie_action=core.NEAR_TIE_COUNT, **opts)
    prefixes = []
    for (tag, a, b, c), r, k in zip(group, stop, count):
        n = len(r.pivots)
        pending = r.status == "near_tie"
        run = es.check_log(tally, tag, a, b, c, log3(r.pivots), r.margins, set(), pending=pending)
        prefixes.append(n if pending else -1)
        if pending:
            if k.first_near_tie != n:
                tally.failures.append(f"{tag}: STOP stopped before pivot {n}, COUNT's first near tie is {k.first_near_tie}")
            if log3(k.pivots)[:n] != log3(r.pivots) or not np.array_equal(_bits(k.margins[:n]), _bits(r.margins)):
                tally.failures.append(f"{tag}: COUNT's log or margins differ from STOP's before pivot {n}")
        else:
            if (k.status, k.near_ties, log3(k.pivots)) != (r.status, 0, log3(r.pivots)):
                tally.failures.append(f"{tag}: an unflagged LP differs between STOP and COUNT")
            if run.stopped_at is None:
                check_end(tally, tag, run, r, set())
    print("\n" + tally.line(f"solve_batch_fast, {name}") + f"; prefix lengths {sorted(set(prefixes))}")
    assert not tally.failures, f"{len(tally.failures)} failures:\n" + "\n".join(tally.failures[:40])
    assert len(lps) >= 64 and len({p for p in prefixes if p >= 0}) >= 3 and max(prefixes) >= 3
    assert tally.unflagged >= 100 and tally.flagged >= 30


# ---------------------------------------------------------------------------- the deep regimes
# The large-k kernel forms cannot be shadowed whole, but a small exact problem can be embedded in a
# large one.  R is a continuous 1024 x 2048 block started from the basis "first k structurals" in a
# state chosen so that R never competes: x = x*, z = z* with entries in (1e6, 2e6) (b and c are
# DERIVED from them in long double: b = B x*, c = N^T y* - z* with y* = z* on the rows whose slack
# is nonbasic and 0 elsewhere), so every first-pivot ratio of R is below -1e6, and R's dx and dz are
# exactly 0 while only the gadget pivots (block-diagonal data), so R never enters a ratio test.  The
# gadget G (5 x 10 integers, costs and right-hand sides times 1e3, slack basis) sits block-diagonally
# and the shadow of G alone predicts every pivot; claims A-D apply, F from STOP + resume.  Where G's
# twins sit among the nonbasic and basic positions is the point: both sides of what the kernels cut
# the columns and rows into.
MR, NSR, MG, NSG = 1024, 2048, 5, 10
DEEP_PIVOTS = 12
GADGET_SEED = 7054  # its controls stay clear of a verdict and of mu < 10 for six pivots, in every placement
_deep_base = {}


def deep_base(core, k):
    """R's matrix and the b, c that make (x*, z*) the state of the basis "first k structurals"."""
    if k not in _deep_base:
        LD = np.longdouble
        a, _, _ = core.gen_dense_lp(seed=1002, m=MR, n_struct=NSR)
        a = np.ascontiguousarray(a, dtype=np.float64)
        rng = np.random.default_rng(4000 + k)
        xs, zs = 1e6 * rng.uniform(1.0, 2.0, MR), 1e6 * rng.uniform(1.0, 2.0, NSR)  # z*: structurals k.., then slacks
        ald = a.astype(LD)
        b = ald[:, :k] @ xs[:k].astype(LD)
        b[k:] += xs[k:].astype(LD)
        y = np.zeros(MR, LD)
        y[:k] = zs[NSR - k:]                     # nonbasic slack of row r < k: z = y_r
        c = ald.T @ y                            # basic structurals: c_j = a_j . y (reduced cost 0)
        c[k:] -= zs[:NSR - k].astype(LD)         # nonbasic structurals: z_j = a_j . y - c_j = z*_j
        _deep_base.clear()                       # (one regime's 17 MB at a time)
        _deep_base[k] = (a, b.astype(np.float64), c.astype(np.float64), xs, zs)
    return _deep_base[k]


def gadget(seed, col_pair, row_pair, control):
    """5 x 10 integers, distinct costs and right-hand sides (times 1e3).  col_pair: the best column
    gets an identical twin at these two G indices (it enters at pivot 0: a tie between twins for the
    entering index).  row_pair: the row that wins pivot 0's ratio test gets an identical twin at these
    two G rows.  control: the second twin's cost (right-hand side) is moved instead, by a relative 1e-7 of the ratio,
    to the side that makes the SECOND one the winner -- no tie, nothing to flag."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-3, 4, (MG, NSG)).astype(np.float64)
    b = 1e3 * rng.permutation(np.arange(1, MG + 1)).astype(np.float64)
    c = 1e3 * rng.permutation(np.arange(NSG) - 3).astype(np.float64)
    best = int(np.argmax(c))
    if col_pair is not None:
        j0, j1 = col_pair
        for arr in (a.T, c):  # the best column to j0, its twin to j1
            arr[[best, j0]] = arr[[j0, best]]
        a[:, j1], c[j1] = a[:, j0], c[j0]
        if control:
            c[j1] *= 1.0 + 1e-7
        best = j1 if control else j0
    if row_pair is not None:
        i0, i1 = row_pair
        a[i0, best] = 3.0
        ratio = a[:, best] / (b + c[best])   # dx / (x + mu xbar) at pivot 0
        win = int(np.argmax(ratio))
        for arr in (a, b):
            arr[[win, i0]] = arr[[i0, win]]
        a[i1], b[i1] = a[i0], b[i0]
        if control:
            # dx / (x + mu xbar) with mu = c[best] at pivot 0: the second twin's ratio is the larger by
            # 1e-7.  (Moving the row's matrix entry instead leaves two rows 1e-7 apart: a basis of
            # condition 1e7 a few pivots on, where rounding, not the runner-up, decides -- DESIGN section 4.)
            b[i1] = (b[i0] + c[best]) / (1.0 + 1e-7) - c[best]
    return a, b, c


def embedded_lp(core, k, g, col_pos, row_pos):
    """R and G block-diagonally; G's columns at the nonbasic positions col_pos and G's slacks at the
    basic positions row_pos (both increasing, so 'the lower position' means the same in G alone)."""
    a_r, b_r, c_r, xs, zs = deep_base(core, k)
    ga, gb, gc = g
    m, ns = MR + MG, NSR + NSG
    a = np.zeros((m, ns))
    a[:MR, :NSR], a[MR:, NSR:] = a_r, ga
    c = np.concatenate([c_r, gc, np.zeros(m)])
    # warm_started's layout for R, G's slack basis behind it; then G's members swapped into place
    basis = np.concatenate([np.arange(k), ns + np.arange(k, MR), ns + MR + np.arange(MG)]).astype(np.int64)
    nonbasis = np.concatenate([np.arange(k, NSR), ns + np.arange(k), NSR + np.arange(NSG)]).astype(np.int64)
    x, z = np.concatenate([xs, gb]), np.concatenate([zs, -gc])
    for arr_pos, codes, vals, first in ((row_pos, basis, x, MR), (col_pos, nonbasis, z, NSR)):
        assert list(arr_pos) == sorted(set(arr_pos))
        order = np.arange(len(codes))
        free = [p for p in range(len(codes) - 1, -1, -1) if p not in set(arr_pos)]
        # G's members to arr_pos in order; whoever sat there moves to the freed places
        src = list(range(first, len(codes)))
        moved_out = [p for p in arr_pos if p < first]
        targets = [p for p in src if p not in set(arr_pos)]
        order[list(arr_pos)] = src
        order[targets] = moved_out
        codes[:], vals[:] = codes[order], vals[order]
    assert k <= min(row_pos)
    return core.CoreLP(a=a, c=c, basis=basis, nonbasis=nonbasis, x=x, z=z)


def deep_case(core, tally, tag, k, g, col_pos, row_pos, expect_tie, **opts):
    ga, gb, gc = g
    lp = embedded_lp(core, k, g, col_pos, row_pos)
    r, flagged = solve_stop_resume(core, lp, DEEP_PIVOTS, poll_interval=4, **opts)
    ns = NSR + NSG
    glog, fail = [], tally.failures.append
    for kind, enter, leave in log3(r.pivots):  # back to G's own codes
        ge = enter - NSR if NSR <= enter < ns else (enter - ns - MR + NSG if enter >= ns + MR else None)
        gl = leave - NSR if NSR <= leave < ns else (leave - ns - MR + NSG if leave >= ns + MR else None)
        if ge is None or gl is None:
            break
        glog.append((kind, ge, gl))
    # follow while G dominates: mu at least 10 and both first-pivot sides led by two candidates of G
    sh, n = es.Shadow(ga.tolist(), gb.tolist(), gc.tolist()), 0
    twins, moved = es.twin_classes(ga.tolist(), gb.tolist(), gc.tolist()), set()
    for j, p in enumerate(glog):
        step = sh.decide()
        sides = [sum(yb > 0 for yb in sh.zbar), sum(xb > 0 for xb in sh.xbar)]
        if step.mu is None or step.mu < 10 or min(sides) < 2 or step.verdict is not None:
            break
        es.check_pivot(tally, tag, j, step, p, float(r.margins[j]), j in flagged, twins, moved)
        if j == 0:
            if expect_tie and not (0 in flagged and r.margins[0] == 0.0 and step.reasons == {"tie"}
                                   and p[1] == min(step.entering_set) and p[2] == min(step.leaving_set)):
                fail(f"{tag}: pivot 0 is a tie between twins: flagged {0 in flagged}, margin {r.margins[0]!r}, "
                     f"{p} of entering {sorted(step.entering_set)} leaving {sorted(step.leaving_set)}")
            if not expect_tie and (0 in flagged or step.delicate or not 0.9e-7 < step.margin < 1.1e-7):
                fail(f"{tag}: control's pivot 0: flagged {0 in flagged}, exact margin {float(step.margin):.3e}")
        moved |= {p[1], p[2]}
        n += 1
        if not sh.pivot(p[1], p[2]):
            break
    if n < (1 if expect_tie else 5):
        fail(f"{tag}: only {n} pivots of the gadget checked; log {log3(r.pivots)[:4]}, status {r.status}")
    if r.chain_fallbacks:
        fail(f"{tag}: {r.chain_fallbacks} chain fallbacks")
    return r


# twin columns: both sides of a lane, a wave, a 256- and a 512-column boundary, the two last positions
# and the two ends; q = 2058 nonbasic positions.  G's ten columns sit at ten increasing positions of
# which two hold the twins (G indices j0 < j1).
Q = NSR + NSG
COL_CASES = {
    "0,1": ((0, 1), [0, 1, 5, 70, 300, 700, 1000, 1300, 1700, 2000]),
    "63,64": ((1, 2), [3, 63, 64, 200, 300, 700, 1000, 1300, 1700, 2000]),
    "255,256": ((2, 3), [3, 100, 255, 256, 300, 700, 1000, 1300, 1700, 2000]),
    "511,512": ((3, 4), [3, 100, 200, 511, 512, 700, 1000, 1300, 1700, 2000]),
    "q-2,q-1": ((8, 9), [3, 100, 200, 400, 600, 700, 1000, 1300, Q - 2, Q - 1]),
    "0,q-1": ((0, 9), [0, 100, 200, 400, 600, 700, 1000, 1300, 1700, Q - 1]),
}


def row_cases(k):
    """Twin rows at the first and last row of one workgroup's share of 8 rows (1029 rows on 256
    workgroups: ((1029 + 255) / 256 + 3) & ~3), and on the two sides of a share's end."""
    s = (k + 15) // 8 * 8  # the first share that starts at or above k + 8
    return {"one share": ((0, 1), [s, s + 7, s + 40, s + 81, s + 122]),
            "two shares": ((1, 2), [s + 2, s + 7, s + 8, s + 81, s + 122])}


# (k, environment, price_pass_used: 1 the row-wise pass, 2 the column pass; rows_T is 638 at this shape)
DEEP_REGIMES = {"k=100": (100, {}, 1), "k=200": (200, {}, 1), "k=400": (400, {}, 1), "k=520": (520, {}, 1),
                "k=700": (700, {}, 2), "k=520 rows only": (520, {"DZG_PRICE_ROWS_T": "1000000"}, 1),
                "k=520 columns only": (520, {"DZG_PRICE_ROWS": "0"}, 2)}


@pytest.mark.parametrize("seven", [0, 1])
@pytest.mark.parametrize("regime", sorted(DEEP_REGIMES))
def test_twins_at_the_kernels_edges_in_the_deep_regimes(core, monkeypatch, regime, seven):
    """Below 127, 127-254, 255-479, 480 up to rows_T (638 at this shape) and above it, chain form and
    seven launches: a tie between bit-identical twins is flagged with margin exactly 0.0 and goes to
    the lower position; with one twin moved by a relative 1e-7 nothing is flagged, the larger wins and
    the margin is the exact one to 1e-9."""
    k, env, price_pass = DEEP_REGIMES[regime]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    tally, used = es.Tally(), set()
    default_rows = list(range(MR, MR + MG))
    default_cols = COL_CASES["0,1"][1]
    for where, (pair, pos) in COL_CASES.items():
        for control in (False, True):
            g = gadget(GADGET_SEED, pair, None, control)
            r = deep_case(core, tally, f"{regime} columns {where}{' control' if control else ''}", k, g, pos,
                          default_rows, not control, seven_launches=seven)
            used.add(r.price_pass_used)
    for where, (pair, pos) in row_cases(k).items():
        for control in (False, True):
            g = gadget(GADGET_SEED, None, pair, control)
            deep_case(core, tally, f"{regime} rows {where}{' control' if control else ''}", k, g, default_cols,
                      pos, not control, seven_launches=seven)
    print("\n" + tally.line(f"{regime}, {'seven launches' if seven else 'chain'}") + f"; price_pass_used {sorted(used)}")
    assert not tally.failures, f"{len(tally.failures)} failures:\n" + "\n".join(tally.failures[:40])
    assert tally.twin_zero >= 8 and tally.unflagged >= 40 and used == {price_pass}
