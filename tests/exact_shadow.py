"""The reference's pivot rule in exact rational arithmetic, following a given pivot log.

    max c.x  st  A x <= b, x >= 0,  data taken as the exact rationals its doubles are, slack basis (codes: structurals 0 .. ns-1, slacks
    ns .. ns+m-1, as CoreLP.from_inequality_form and oracle.stdform_from_dense number them).

State, all `fractions.Fraction`: x, xbar, z, zbar updated by the reference's own formulas
(oracle/dzg_oracle.c, do_pivot / pivot_vec) and the tableau T = B^-1 [A I], from which dx is a column
and dz a negated row.  Before each logged pivot the shadow takes every decision of the reference's
status() and ratio test (ora_find_first_pivot, ora_find_second_pivot, ora_simplex_solve) on the exact
state -- the argmax SETS, so a tie is an equality of fractions -- and the margin FAST would report if
it computed in exact arithmetic (dzg_margin, combined as fast_status and ratio_margin combine them).
Then it applies the LOGGED pivot, whatever the exact rule would have done: a pivot FAST (or the float
reference) resolves differently from exact arithmetic does not derail it.

Nothing here reads a float the solver under test produced, except the log it is told to follow.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from fractions import Fraction

INF = float("inf")
PRIMAL, DUAL = 0, 1
EPSILON = Fraction(1, 10 ** 12)   # the reference's optimality threshold (src/simplex.rs:9)
OPT_EDGE = Fraction(1, 10 ** 6)   # |top - EPSILON| within this: the optimality test is at rounding level


def rel_margin(winner, runner_up):
    """dzg_margin on exact values: (winner - runner-up) / max(|winner|, |runner-up|); 0 on a tie
    (and when both are 0); +inf with no runner-up (None)."""
    if runner_up is None:
        return INF
    den = max(abs(winner), abs(runner_up))
    if den == 0:
        return Fraction(0)
    return (winner - runner_up) / den


def argmax_set(cands, skip=None):
    """cands: [(ratio, position)].  Returns (argmax set of positions, top ratio, margin); margin is
    None without a candidate.  `skip` (mutation hook of the host test, never set otherwise): the
    runner-up does not look at that position -- what a reduction that drops one lane would do."""
    if not cands:
        return frozenset(), None, None
    top = max(r for r, _ in cands)
    win = sorted(k for r, k in cands if r == top)
    lowest = win[0]
    others = [r for r, k in cands if k != lowest and k != skip]
    runner = max(others) if others else None
    if skip is not None:
        win = [k for k in win if k == lowest or k != skip]
    return frozenset(win), top, rel_margin(top, runner)


@dataclass
class Step:
    """What exact arithmetic says about one iteration (or about the state after the last logged one)."""
    first_z: frozenset = frozenset()   # argmax set of find_first_pivot(z, zbar), nonbasic positions
    first_x: frozenset = frozenset()   # ... of find_first_pivot(x, xbar), basic positions
    kind: int | None = None            # the step status() takes (DUAL on primal == dual, as `primal < dual` says)
    mu: Fraction | None = None
    ratio_set: frozenset = frozenset() # argmax set of the ratio test over ratios > 0, positions
    verdict: str | None = None         # "optimal" / "unbounded" / "infeasible" / "panic": no pivot follows
    margin: object = INF               # M_j: Fraction, or INF
    reasons: frozenset = frozenset()   # why the iteration is delicate (empty: it is not)
    shadowed_pseudo: bool = False      # see below
    opt_edge: bool = False             # both sides have candidates and |top - EPSILON| <= OPT_EDGE
    decision: tuple | None = None      # (kind, entering code, leaving code) when every set is a singleton
    tie_codes: frozenset = frozenset() # variable codes tied in the decisions whose index is used
    entering_set: frozenset = frozenset()  # codes exact arithmetic allows as entering / leaving
    leaving_set: frozenset = frozenset()

    @property
    def delicate(self) -> bool:
        return bool(self.reasons)

    @property
    def must_flag(self) -> bool:
        """Delicate for a reason that can change what the reference does (see shadowed_pseudo)."""
        return bool(self.reasons) and not self.shadowed_pseudo


# Reasons.  "tie": an argmax whose index is used has more than one winner, or both ratios are 0;
# "primal=dual"; "zero_ybar": an entry of a first-pivot side with ybar = 0 exactly (0/0 when y = 0 too;
# otherwise the sign of a rounding error decides whether the reference has a candidate there);
# "zero_den": a ratio-test denominator y + mu ybar = 0 exactly; "nonpositive_winner" cannot arise from
# exact ratios > 0 and is kept for completeness of the list.
# shadowed_pseudo: the iteration's ONLY reason is zero_ybar, every such entry has y > 0, and its side
# has a real candidate (ybar > 0) as well.  In the reference that entry is no candidate or one with a
# hugely negative ratio: it cannot win and cannot be the runner-up that matters; dzg_first_pivot_entry
# lets it stand aside (ratio -inf) and fast_status flags it only when it is its side's best.


@dataclass
class ShadowRun:
    steps: list = field(default_factory=list)   # one Step per logged pivot reached
    terminal: Step | None = None                # the state after the last logged pivot (None: stopped)
    stopped_at: int | None = None               # index of a logged pivot whose element is exactly 0
    x: list = field(default_factory=list)
    z: list = field(default_factory=list)
    basis: list = field(default_factory=list)
    nonbasis: list = field(default_factory=list)


def _first_side(y, ybar, skip):
    cands = [(-y[k] / ybar[k], k) for k in range(len(y)) if ybar[k] > 0]
    zero = [k for k in range(len(y)) if ybar[k] == 0]
    win, top, mg = argmax_set(cands, skip)
    # every zero-ybar entry harmless in the reference?  (y > 0 there and a real candidate beside it)
    harmless = bool(cands) and all(y[k] > 0 for k in zero)
    return win, top, mg, bool(zero), harmless


def _ratio_test(mu, y, ybar, dy, skip):
    cands, zero_den = [], False
    for k in range(len(y)):
        den = y[k] + mu * ybar[k]
        if den == 0:
            zero_den = True
            continue
        r = dy[k] / den
        if r > 0:
            cands.append((r, k))
    win, top, mg = argmax_set(cands, skip)
    return win, top, mg, zero_den


class Shadow:
    def __init__(self, a, b, c, skip_runner_up=None):
        m, ns = len(a), len(a[0]) if len(a) else 0
        F = Fraction  # (of a float: that double exactly -- integers in the families, any double in a control)
        self.m, self.ns = m, ns
        self.T = [[F(v) for v in a[i]] + [F(int(i == r)) for r in range(m)] for i in range(m)]
        self.basis = list(range(ns, ns + m))
        self.nonbasis = list(range(ns))
        self.x = [F(v) for v in b]
        self.xbar = [F(1)] * m
        self.z = [-F(v) for v in c]
        self.zbar = [F(1)] * ns
        self.skip = skip_runner_up

    def dx(self, code):
        return [self.T[i][code] for i in range(self.m)]

    def dz(self, b_i):
        row = self.T[b_i]
        return [-row[j] for j in self.nonbasis]

    def decide(self) -> Step:
        s = Step()
        wj, dual, mj, zero_z, harmless_z = _first_side(self.z, self.zbar, self.skip)
        wi, primal, mi, zero_x, harmless_x = _first_side(self.x, self.xbar, self.skip)
        s.first_z, s.first_x = wj, wi
        reasons = set()
        if zero_z or zero_x:
            reasons.add("zero_ybar")
        margins = []
        if wj and wi:
            top = max(primal, dual)
            s.opt_edge = abs(top - EPSILON) <= OPT_EDGE
            if primal <= EPSILON and dual <= EPSILON:
                s.verdict = "optimal"
            else:
                if primal == dual:
                    reasons.add("primal=dual")
                margins.append(rel_margin(max(primal, dual), min(primal, dual)))
                s.kind, s.mu = (PRIMAL, dual) if primal < dual else (DUAL, primal)
        elif wj:
            s.kind, s.mu = PRIMAL, dual
        elif wi:
            s.kind, s.mu = DUAL, primal
        else:
            s.verdict = "panic"
        tie_codes = set()
        if s.kind == PRIMAL:
            margins.append(mj)
            s.entering_set = frozenset(self.nonbasis[k] for k in wj)
            if len(wj) > 1:
                tie_codes |= s.entering_set
            n_j = min(wj)
            w2, top2, m2, zero_den = _ratio_test(s.mu, self.x, self.xbar, self.dx(self.nonbasis[n_j]), self.skip)
            s.leaving_set = frozenset(self.basis[k] for k in w2)
            if not w2:
                s.verdict = "unbounded"
        elif s.kind == DUAL:
            margins.append(mi)
            s.leaving_set = frozenset(self.basis[k] for k in wi)
            if len(wi) > 1:
                tie_codes |= s.leaving_set
            b_i = min(wi)
            w2, top2, m2, zero_den = _ratio_test(s.mu, self.z, self.zbar, self.dz(b_i), self.skip)
            s.entering_set = frozenset(self.nonbasis[k] for k in w2)
            if not w2:
                s.verdict = "infeasible"
        if s.kind is not None:
            s.ratio_set = w2
            if zero_den:
                reasons.add("zero_den")
            if w2:
                margins.append(m2)
                if not top2 > 0:
                    reasons.add("nonpositive_winner")
                if len(w2) > 1:
                    tie_codes |= s.leaving_set if s.kind == PRIMAL else s.entering_set
        s.margin = min(margins, default=INF)
        if s.margin == 0:
            reasons.add("tie")
        s.tie_codes = frozenset(tie_codes)
        s.reasons = frozenset(reasons)
        s.shadowed_pseudo = (reasons == {"zero_ybar"} and (not zero_z or harmless_z)
                             and (not zero_x or harmless_x))
        if s.verdict is None and len(s.entering_set) == 1 and len(s.leaving_set) == 1:
            s.decision = (s.kind, next(iter(s.entering_set)), next(iter(s.leaving_set)))
        return s

    def pivot(self, entering, leaving) -> bool:
        """Applies a logged pivot exactly (do_pivot); False when its element is exactly zero."""
        n_j, b_i = self.nonbasis.index(entering), self.basis.index(leaving)
        dx, dz = self.dx(entering), self.dz(b_i)
        if dx[b_i] == 0:
            return False
        assert dz[n_j] == -dx[b_i]

        def upd(v, d, p, num):
            t = num / d[p]
            for k in range(len(v)):
                v[k] = v[k] - t * d[k] if d[k] != 0 else v[k]
            v[p] = t

        upd(self.x, dx, b_i, self.x[b_i])
        upd(self.xbar, dx, b_i, self.xbar[b_i])
        upd(self.z, dz, n_j, self.z[n_j])
        upd(self.zbar, dz, n_j, self.zbar[n_j])
        T = self.T
        piv = T[b_i][entering]
        prow = [v / piv if v != 0 else v for v in T[b_i]]
        nz = [j for j, v in enumerate(prow) if v != 0]
        for i in range(self.m):
            f = T[i][entering]
            if i == b_i or f == 0:
                continue
            row = T[i]
            for j in nz:
                row[j] -= f * prow[j]
        T[b_i] = prow
        self.basis[b_i], self.nonbasis[n_j] = entering, leaving
        return True


def follow(a, b, c, log, skip_runner_up=None, with_terminal=True) -> ShadowRun:
    """The shadow along `log` = [(kind, entering, leaving), ...] (further fields ignored)."""
    sh = Shadow(a, b, c, skip_runner_up)
    run = ShadowRun()
    for j, p in enumerate(log):
        run.steps.append(sh.decide())
        if not sh.pivot(int(p[1]), int(p[2])):
            run.stopped_at = j
            break
    if run.stopped_at is None and with_terminal:
        run.terminal = sh.decide()
    run.x, run.z, run.basis, run.nonbasis = sh.x, sh.z, sh.basis, sh.nonbasis
    return run


# ------------------------------------------------------------------------------------------------
# The LP groups both test files use.  (family, rows from, rows below, how many): seeds count up from
# the group's base, and an LP with more than 100 structurals is passed over.  `cap` is the number of
# pivots followed per LP.  tests/test_exact_shadow_host.py asserts, from the oracle's logs alone, that
# every group has enough delicate and enough clean pivots and no exact margin in (0, 1e-6).
# ------------------------------------------------------------------------------------------------
GROUPS = {
    # one LP at a time (Solver): families 1, 2 and 3 at 8-40 rows, a few of 41-72 rows
    "solver": dict(base=9100, cap=80, parts=[(1, 8, 41, 8), (1, 41, 73, 2), (2, 8, 41, 4), (3, 8, 41, 8),
                                             (3, 41, 73, 1), (4, 8, 41, 4), (5, 8, 41, 8)]),
    # one batch call per row bucket of batch_host.h.  The batch solver's STOP is not resumed: what is
    # checked is the run of pivots before an LP's first flag, and families 1-3 are flagged at pivot 0 or
    # 1 at these widths -- families 4 and 5 supply the longer runs
    "batch16": dict(base=9300, cap=12, parts=[(4, 8, 17, 32), (5, 8, 17, 12), (1, 8, 17, 8), (2, 8, 17, 4), (3, 8, 17, 8)]),
    "batch32": dict(base=9400, cap=8, parts=[(4, 17, 33, 32), (5, 17, 33, 12), (1, 17, 33, 8), (2, 17, 33, 4), (3, 17, 33, 8)]),
    "batch64": dict(base=9500, cap=6, parts=[(4, 33, 65, 32), (5, 33, 65, 12), (1, 33, 65, 8), (2, 33, 65, 4), (3, 33, 65, 8)]),
    "batch72": dict(base=9600, cap=6, parts=[(4, 65, 73, 32), (5, 65, 73, 12), (1, 65, 73, 8), (2, 65, 73, 4), (3, 65, 73, 8)]),
}
_group_cache, _follow_cache = {}, {}


def group_lps(name):
    """[(tag, a, b, c)] of a group, a / b / c as float64 arrays of integers."""
    if name not in _group_cache:
        from tests.lp_families import make_lp

        g, out = GROUPS[name], []
        seed = g["base"]
        for kind, lo, hi, count in g["parts"]:
            got = 0
            while got < count:
                a, b, c = make_lp(seed, kind, lo, hi)
                seed += 1
                if a.shape[1] > 100:
                    continue
                out.append((f"{name}/family{kind}/seed{seed - 1}", a, b, c))
                got += 1
        _group_cache[name] = out
    return _group_cache[name]


def follow_cached(tag, a, b, c, log):
    """follow() on an LP of a group, remembered per (LP, log): most paths of FAST produce the same log."""
    key = (tag, tuple(tuple(int(v) for v in p[:3]) for p in log))
    if key not in _follow_cache:
        _follow_cache[key] = follow(a.tolist(), b.tolist(), c.tolist(), key[1])
    return _follow_cache[key]


# ------------------------------------------------------------------------------------------------
# FAST against the shadow: claims A-E of tests/test_gpu_near_tie_exact.py.  The flagged set and the
# log come from FAST; everything they are compared with comes from the Fractions above.
# ------------------------------------------------------------------------------------------------
NO_SPURIOUS_ABOVE = 1e-6   # C: a flag needs a delicate pivot or an exact margin at most this
MARGIN_AGREES_TO = 1e-9    # D


def twin_classes(a, b, c):
    """code -> class id, for variables with an identical twin in the data: structural columns with
    the same column and cost, slacks of rows with the same row and right-hand side."""
    m, ns = len(a), len(a[0])
    out, seen = {}, {}
    for j in range(ns):
        key = ("c", tuple(a[i][j] for i in range(m)), c[j])
        seen.setdefault(key, []).append(j)
    for i in range(m):
        key = ("r", tuple(a[i]), b[i])
        seen.setdefault(key, []).append(ns + i)
    for n, codes in enumerate(v for v in seen.values() if len(v) > 1):
        for code in codes:
            out[code] = n
    return out


@dataclass
class Tally:
    """What one path checked (printed by the tests; DESIGN section 4 quotes it)."""
    delicate: int = 0          # delicate pivots reached (A)
    unflagged: int = 0         # unflagged pivots checked (B, D)
    unchecked: int = 0         # logged pivots behind a pivot element that is exactly zero
    flagged: int = 0
    spurious: int = 0          # flagged, not delicate (C lets them pass only at an exact margin <= 1e-6 or at
                               # the optimality test's edge)
    shadowed_pseudo_unflagged: int = 0
    twin_zero: int = 0         # first ties between bit-identical twins: margins[j] == 0.0 asserted
    worst_margin_gap: float = 0.0
    terminals: int = 0
    after_twin_event: int = 0  # flagged pivots whose reasons include the 0/0 a twin pivot leaves behind
    failures: list = field(default_factory=list)

    def line(self, name):
        return (f"{name}: delicate {self.delicate}, unflagged checked {self.unflagged}, unchecked {self.unchecked}, "
                f"flagged {self.flagged} (spurious {self.spurious}), twin ties at exactly 0.0 {self.twin_zero}, "
                f"worst |margins - M| {self.worst_margin_gap:.3e}, shadowed pseudo-candidates left unflagged "
                f"{self.shadowed_pseudo_unflagged}, flagged with a zero ybar in the state {self.after_twin_event}, "
                f"terminal verdicts {self.terminals}")


def check_pivot(tally, tag, j, step, logged, margin, is_flagged, twins, moved):
    """Claims A-D for pivot j.  `logged` = FAST's (kind, entering, leaving), None when FAST stopped
    before executing it (the batch solver's STOP); margin likewise."""
    fail = tally.failures.append
    if step.must_flag:
        tally.delicate += 1
    if is_flagged:
        tally.flagged += 1
        if "zero_ybar" in step.reasons:
            tally.after_twin_event += 1
        if not step.delicate:
            tally.spurious += 1
            if not (step.margin <= NO_SPURIOUS_ABOVE or step.opt_edge):                       # C
                fail(f"{tag} pivot {j}: C flagged, not delicate, exact margin {float(step.margin):.3e}")
        if (step.reasons == {"tie"} and margin is not None and step.tie_codes
                and len({twins.get(v, -1 - v) for v in step.tie_codes}) == 1
                and not (step.tie_codes & moved)):
            tally.twin_zero += 1
            if margin != 0.0:                                                                 # A, twins
                fail(f"{tag} pivot {j}: A tie between bit-identical twins {sorted(step.tie_codes)}, "
                     f"margin {margin!r} is not 0.0")
        return
    if step.must_flag:                                                                        # A
        fail(f"{tag} pivot {j}: A delicate {sorted(step.reasons)} (exact margin {float(step.margin):.3e}) "
             f"not flagged, FAST margin {margin!r}")
        return
    tally.shadowed_pseudo_unflagged += step.shadowed_pseudo
    tally.unflagged += 1
    if logged is not None and tuple(logged) != step.decision:                                 # B
        fail(f"{tag} pivot {j}: B unflagged {tuple(logged)} is not the exact decision {step.decision} "
             f"(entering {sorted(step.entering_set)}, leaving {sorted(step.leaving_set)})")
    if margin is not None:                                                                    # D
        if step.margin == INF or margin == INF:
            if not (step.margin == INF and margin == INF):
                fail(f"{tag} pivot {j}: D margin {margin!r} against exact {float(step.margin)!r}")
        else:
            gap = abs(Fraction(margin) - step.margin)
            tally.worst_margin_gap = max(tally.worst_margin_gap, float(gap))
            if gap > MARGIN_AGREES_TO:
                fail(f"{tag} pivot {j}: D margin {margin!r} against exact {float(step.margin)!r}")


def check_log(tally, tag, a, b, c, log, margins, flagged, pending=False, cap=None):
    """Follows FAST's `log` and applies A-D to every pivot the shadow reaches.  pending: FAST stopped
    before pivot len(log) (flagged, not executed): C is applied to that iteration as well.  Returns
    the ShadowRun (its terminal Step is the state after the log, for E)."""
    log = [tuple(int(v) for v in p[:3]) for p in log]
    if cap is not None:
        log = log[:cap]
    run = follow_cached(tag, a, b, c, log)
    twins = twin_classes(a.tolist(), b.tolist(), c.tolist())
    moved = set()
    for j, step in enumerate(run.steps):
        check_pivot(tally, tag, j, step, log[j], float(margins[j]), j in flagged, twins, moved)
        moved |= {log[j][1], log[j][2]}
    tally.unchecked += len(log) - len(run.steps)
    if pending and run.terminal is not None:
        check_pivot(tally, tag, len(log), run.terminal, None, None, True, twins, moved)
    return run
