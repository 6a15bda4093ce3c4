"""LPs whose final basis is built to order, and a checker of sensitivity ranges that looks at the
winning variable as well as at the endpoint (pure numpy; tests/test_planted_host.py holds both to
the CPU oracle, tests/test_gpu_planted_postsolve.py uses them on the FAST post-solve kernels).

    max c.x  st  a x <= b,  x >= 0        variables 0..ns-1 structural, ns + r the slack of row r

planted_optimal: a support S of k structurals and a set T of k tight rows are drawn; x*_S, the slacks
of the rows outside T, y*_T and the reduced costs t of the structurals outside S are multiples of 1/4
in [1/4, 2]; b = a x* + slack and c = a^T y* - t.  The basis is S plus the slacks of the rows outside
T, optimal by construction, and the state handed over is the planted one: x by basis position, z by
nonbasic position.  The structurals sit at a random permutation of T's positions and the basic
slacks at a derangement of the other positions, so no slack sits at the position of its own row and
S is not in order; the nonbasic set is shuffled.  degenerate = g sets g of x*_S and g basic slacks to
exactly 0.0: with the planted x carried as it is, every ratio at such a position is -0.0 or +0.0 in
any arithmetic, and the right-hand-side ranges have exact ties.

planted_unbounded / planted_infeasible: the same data with one column (one row) of the matrix rebuilt
so that the planted state is where the solve stops, before its first pivot, with the entering
(leaving) position known.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tests import ranging_reference as rref
from tests import state_check as sc
from tests.duals_helpers import long_double_y

LD = np.longdouble
C_DUALS = 32.0           # tests/test_gpu_duals.py
FLOOR = 1e-13            # the floor of the tolerance there
SKIP_CAP = 0.02          # directions with a |delta| within a factor 2 of pivot_tol: at most 2 %
CLOSE = 1e-6             # positions kept per direction: within this of the best (>> any tolerance)


# ---------------------------------------------------------------- generators
@dataclass
class Planted:
    """One planted LP in its final state.  pos / var: the nonbasic position and variable that enter
    (an unbounded plant) or the basis position and variable that leave (an infeasible one), -1
    otherwise."""
    a: np.ndarray
    b: np.ndarray
    c: np.ndarray
    basis: np.ndarray
    nonbasis: np.ndarray
    x: np.ndarray
    z: np.ndarray
    pos: int = -1
    var: int = -1
    zeros: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))  # positions with x = 0.0

    def __iter__(self):  # (a, b, c, basis, nonbasis, x, z) = planted_optimal(...)
        return iter((self.a, self.b, self.c, self.basis, self.nonbasis, self.x, self.z))

    @property
    def cc(self):
        """c over all n variables (0 for the slacks)."""
        return np.concatenate([self.c, np.zeros(self.a.shape[0])])


def _quarters(rng, size):
    return rng.integers(1, 9, size).astype(np.float64) / 4.0


def _skeleton(seed, m, ns, k):
    """a, S, T and the positions: struct_pos[i] the position of S[i], slack_pos[i] of off[i]'s slack."""
    if not 0 <= k <= min(m, ns):
        raise ValueError("planted: 0 <= k <= min(m, ns)")
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, (m, ns))
    s_cols = rng.choice(ns, k, replace=False)
    t_rows = np.sort(rng.choice(m, k, replace=False))
    off = np.setdiff1d(np.arange(m), t_rows)
    struct_pos = rng.permutation(t_rows)
    slack_pos = np.roll(off, int(rng.integers(1, len(off)))) if len(off) > 1 else off.copy()
    if len(off) == 1 and k > 0:  # the one basic slack trades places with a structural
        struct_pos[0], slack_pos[0] = slack_pos[0], struct_pos[0]
    return rng, a, s_cols, t_rows, off, struct_pos, slack_pos


def _finish(rng, m, ns, a, b, c, s_cols, t_rows, off, struct_pos, slack_pos, xs, slack, y_t, t_red):
    basis = np.empty(m, dtype=np.int64)
    x = np.empty(m)
    basis[struct_pos], x[struct_pos] = s_cols, xs
    basis[slack_pos], x[slack_pos] = ns + off, slack
    nb_struct = np.setdiff1d(np.arange(ns), s_cols)
    nonbasis = np.concatenate([nb_struct, ns + t_rows]).astype(np.int64)
    z = np.concatenate([t_red[nb_struct], y_t])
    order = rng.permutation(len(nonbasis))
    return Planted(a=a, b=b, c=c, basis=basis, nonbasis=nonbasis[order], x=x, z=z[order],
                   zeros=np.flatnonzero(x == 0.0))


def _values(rng, m, ns, k):
    xs, slack = _quarters(rng, k), _quarters(rng, m - k)
    y_t, t_red = _quarters(rng, k), _quarters(rng, ns)
    return xs, slack, y_t, t_red


def _data(a, s_cols, t_rows, off, xs, slack, y_t, t_red):
    m, ns = a.shape
    xfull, yfull, sfull = np.zeros(ns), np.zeros(m), np.zeros(m)
    xfull[s_cols], yfull[t_rows], sfull[off] = xs, y_t, slack
    t_red = t_red.copy()
    t_red[s_cols] = 0.0
    return a @ xfull + sfull, a.T @ yfull - t_red, t_red


def planted_optimal(seed, m, ns, k, degenerate=0, zero_positions=None) -> Planted:
    """The planted optimum.  degenerate = g: g structural and g slack positions (drawn, or the
    positions listed in zero_positions) carry x = 0.0 exactly."""
    rng, a, s_cols, t_rows, off, struct_pos, slack_pos = _skeleton(seed, m, ns, k)
    xs, slack, y_t, t_red = _values(rng, m, ns, k)
    if zero_positions is not None:
        zero_positions = np.asarray(zero_positions, dtype=np.int64)
        xs[np.isin(struct_pos, zero_positions)] = 0.0
        slack[np.isin(slack_pos, zero_positions)] = 0.0
    elif degenerate:
        if degenerate > min(k, m - k):
            raise ValueError("planted: degenerate <= min(k, m - k)")
        xs[rng.choice(k, degenerate, replace=False)] = 0.0
        slack[rng.choice(m - k, degenerate, replace=False)] = 0.0
    b, c, t_red = _data(a, s_cols, t_rows, off, xs, slack, y_t, t_red)
    return _finish(rng, m, ns, a, b, c, s_cols, t_rows, off, struct_pos, slack_pos, xs, slack, y_t, t_red)


def _basis_matrix(a, m, ns, s_cols, off, struct_pos, slack_pos):
    bm = np.zeros((m, m))
    bm[:, struct_pos] = a[:, s_cols]
    bm[off, slack_pos] = 1.0
    return bm


def planted_unbounded(seed, m, ns, k, slack=False) -> Planted:
    """The planted state with an entering variable nothing blocks: B^-1 (its column) = -u, u > 0 a
    vector of quarters, and its reduced cost -1.  slack=False: a nonbasic structural whose column is
    rebuilt as -B u.  slack=True: the slack of a tight row r; one basic structural column is rebuilt
    so that B (-u) = e_r, and y_r = -1."""
    rng, a, s_cols, t_rows, off, struct_pos, slack_pos = _skeleton(seed, m, ns, k)
    if k < 1 or (not slack and k >= ns):
        raise ValueError("planted_unbounded: 1 <= k, and k < ns for a structural entering")
    xs, sl, y_t, t_red = _values(rng, m, ns, k)
    u = _quarters(rng, m)  # by position
    if slack:
        i = int(rng.integers(0, k))
        r = int(t_rows[i])
        y_t[i] = -1.0
        enter = ns + r
        s = int(rng.integers(0, k))  # the basic structural whose column is rebuilt
        bm = _basis_matrix(a, m, ns, s_cols, off, struct_pos, slack_pos)
        rest = bm @ u - bm[:, struct_pos[s]] * u[struct_pos[s]]
        unit = np.zeros(m)
        unit[r] = 1.0
        a[:, s_cols[s]] = (-unit - rest) / u[struct_pos[s]]
    else:
        enter = int(rng.choice(np.setdiff1d(np.arange(ns), s_cols)))
        a[:, enter] = -(_basis_matrix(a, m, ns, s_cols, off, struct_pos, slack_pos) @ u)
        t_red[enter] = -1.0
    b, c, t_red = _data(a, s_cols, t_rows, off, xs, sl, y_t, t_red)
    out = _finish(rng, m, ns, a, b, c, s_cols, t_rows, off, struct_pos, slack_pos, xs, sl, y_t, t_red)
    out.var, out.pos = enter, int(np.flatnonzero(out.nonbasis == enter)[0])
    return out


def planted_infeasible(seed, m, ns, k, slack=False) -> Planted:
    """The planted state with one basic position at x = -1 whose row of B^-1 N is positive, so that no
    nonbasic variable can raise it: the multipliers y (quarters on the tight rows, 0 elsewhere, 1 at
    the leaving slack's own row) have y.a_j = 1 at the leaving structural, 0 at the other basic
    structurals and a quarter at every nonbasic one; one tight row of a is rebuilt to make it so.
    slack=False: a basic structural leaves; slack=True: a basic slack (k < m)."""
    rng, a, s_cols, t_rows, off, struct_pos, slack_pos = _skeleton(seed, m, ns, k)
    if k < 1 or (slack and k >= m):
        raise ValueError("planted_infeasible: 1 <= k, and k < m for a slack leaving")
    xs, sl, y_t, t_red = _values(rng, m, ns, k)
    yf = np.zeros(m)
    yf[t_rows] = _quarters(rng, k)
    target = _quarters(rng, ns)  # y.a_j: positive at the nonbasic structurals
    target[s_cols] = 0.0
    if slack:
        i = int(rng.integers(0, m - k))
        yf[off[i]] = 1.0
        pos, var = int(slack_pos[i]), ns + int(off[i])
        sl[i] = -1.0
    else:
        i = int(rng.integers(0, k))
        target[s_cols[i]] = 1.0
        pos, var = int(struct_pos[i]), int(s_cols[i])
        xs[i] = -1.0
    row = int(rng.choice(t_rows))  # the rebuilt row
    a[row] = (target - (yf @ a - yf[row] * a[row])) / yf[row]
    b, c, t_red = _data(a, s_cols, t_rows, off, xs, sl, y_t, t_red)
    out = _finish(rng, m, ns, a, b, c, s_cols, t_rows, off, struct_pos, slack_pos, xs, sl, y_t, t_red)
    assert out.basis[pos] == var
    out.var, out.pos = var, pos
    return out


def stdform(p: Planted):
    """The oracle's standard form in the planted state."""
    from oracle import oracle as ora

    m, ns = p.a.shape
    col_ptr, row_idx, val = ora.csc_from_dense(np.concatenate([p.a, np.eye(m)], axis=1))
    return ora.StdForm(m=m, n=m + ns, col_ptr=col_ptr, row_idx=row_idx, val=val, c=p.cc, constant=0.0,
                       basis=p.basis.copy(), nonbasis=p.nonbasis.copy(), x=p.x.copy(), z=p.z.copy())


def core_lp(core, p: Planted):
    """The CoreLP that starts in the planted state."""
    return core.CoreLP(a=p.a, c=p.cc, basis=p.basis, nonbasis=p.nonbasis, x=p.x, z=p.z)


# ---------------------------------------------------------------- long-double references of a basis
def basis_columns(a, basis, nonbasis):
    """(B, N, unit_rows) dense: unit_rows[k] = r where nonbasic position k holds the slack of row r."""
    m, ns = a.shape
    codes = sc.var_codes(m + ns, ns)
    nb = codes[np.asarray(nonbasis)]
    return sc.columns(a, m, codes[np.asarray(basis)]), sc.columns(a, m, nb), np.where(nb < 0, -1 - nb, -1)


def exact_duals(a, cc, basis, nonbasis):
    """(y, d_N) in long double: B^T y = c_B refined with long-double residuals, d_N = N^T y - c_N."""
    bm, nm, _ = basis_columns(a, basis, nonbasis)
    cc = np.asarray(cc, dtype=np.float64)
    y = long_double_y(bm, cc[np.asarray(basis)])
    return y, nm.astype(LD).T @ y - cc[np.asarray(nonbasis)].astype(LD)


def numpy_duals(a, cc, basis, nonbasis):
    """The same by numpy's plain double solve: the yardstick."""
    bm, nm, _ = basis_columns(a, basis, nonbasis)
    cc = np.asarray(cc, dtype=np.float64)
    y = np.linalg.solve(bm.T, cc[np.asarray(basis)])
    return y, nm.T @ y - cc[np.asarray(nonbasis)]


@dataclass
class Side:
    """The ranges of one kind of direction in one arithmetic.  near[i]: some |delta| of direction i
    lies in [tol / 2, 2 tol].  close_lo[i] / close_hi[i]: (positions, r, clamped == 0) of the
    candidates of that end whose r lies within CLOSE of the best, positions ascending."""
    ranges: list
    near: list
    close_lo: list
    close_hi: list


def side_from_deltas(deltas, clamped, variables, tol) -> Side:
    """rref.ratio_rule per delta vector (the division taken at the candidates only: a unit direction of
    a nonbasic variable has one), plus the near-winners of each end."""
    out = Side([], [], [], [])
    clamped = np.asarray(clamped)
    for delta in deltas:
        size = np.abs(delta)
        out.near.append(bool(np.any((size >= tol / 2) & (size <= 2 * tol))))
        cand = np.flatnonzero(size > tol)
        dl = delta[cand]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = -(clamped[cand] / dl)
        up = dl > 0
        ends = []
        for store, sel, first_best, none in ((out.close_lo, up, np.argmax, -np.inf),
                                             (out.close_hi, ~up, np.argmin, np.inf)):
            picks, rs = cand[sel], r[sel]
            if not len(picks):
                ends += [none, -1]
                store.append((picks, rs, np.zeros(0, dtype=bool)))
                continue
            j = first_best(rs)  # the first position wins a tie
            ends += [float(rs[j]), int(variables[picks[j]])]
            keep = np.abs(rs - rs[j]) <= CLOSE * max(1.0, abs(float(rs[j])))
            store.append((picks[keep], rs[keep], clamped[picks[keep]] == 0))
        out.ranges.append(rref.RefRange(ends[0], ends[2], ends[1], ends[3]))
    return out


def cost_deltas(inv, nmat, unit_rows, basis, nonbasis, dirs):
    """delta of every cost direction in the arithmetic of inv (as rref.ranges_from_inverse forms it)."""
    ft = inv.dtype
    m, n = inv.shape[0], len(basis) + len(nonbasis)
    unit_rows = np.asarray(unit_rows, dtype=np.int64)
    t = np.zeros((m, len(nonbasis)), dtype=ft)  # B^-1 N
    dense = np.flatnonzero(unit_rows < 0)
    t[:, dense] = inv @ nmat[:, dense].astype(ft)
    slack = np.flatnonzero(unit_rows >= 0)
    t[:, slack] = inv[:, unit_rows[slack]]
    where = np.full(n, -1, dtype=np.int64)
    where[np.asarray(basis)] = np.arange(m)
    for direction in dirs:
        g = np.zeros(n, dtype=ft)
        delta = np.zeros(len(nonbasis), dtype=ft)
        for j, v in direction.items():
            g[int(j)] = v
            if where[int(j)] >= 0:
                delta = delta + ft.type(v) * t[where[int(j)]]
        yield delta - g[np.asarray(nonbasis)]


def rhs_deltas(inv, dirs):
    ft = inv.dtype
    for direction in dirs:
        delta = np.zeros(inv.shape[0], dtype=ft)
        for i, v in direction.items():
            delta = delta + ft.type(v) * inv[:, int(i)]
        yield delta


def reference_sides(a, basis, nonbasis, x, d_n, cost_dirs, rhs_dirs, tol=rref.DEFAULT_TOL, exact=True):
    """(cost Side, rhs Side) of the basis: exact=True from the long-double inverse, with x and d_n as
    given (the carried x; the long-double d_N); exact=False from numpy's double inverse."""
    bm, nm, unit_rows = basis_columns(a, basis, nonbasis)
    m = len(basis)
    inv = rref.refined_inverse(bm) if exact else np.linalg.solve(bm, np.eye(m))
    ft = inv.dtype
    xc = np.maximum(np.asarray(x, dtype=ft), 0)
    dc = np.maximum(np.asarray(d_n, dtype=ft), 0)
    cost = side_from_deltas(cost_deltas(inv, nm, unit_rows, basis, nonbasis, cost_dirs), dc, nonbasis, tol)
    rhs = side_from_deltas(rhs_deltas(inv, rhs_dirs), xc, basis, tol)
    return cost, rhs


# ---------------------------------------------------------------- the checker
def endpoint_error(got_lo, got_hi, want, skip, what):
    """max |t - t^| / max(1, |t^|) over the finite endpoints of the directions not skipped; infinite
    and finite must agree exactly (tests/test_gpu_ranging.py's metric)."""
    worst = 0.0
    for i, w in enumerate(want):
        if skip[i]:
            continue
        for g, t in ((got_lo[i], w.lo), (got_hi[i], w.hi)):
            assert np.isfinite(g) == np.isfinite(t), (what, i, g, t)
            if np.isfinite(t):
                worst = max(worst, abs(g - t) / max(1.0, abs(t)))
            else:
                assert g == t, (what, i, g, t)
    return worst


def _check_winner(got_var, end, close, variables, tol, what):
    """Returns 1 if the end was an exact tie of two or more positions."""
    pos, r, zero = close
    if not np.isfinite(end):
        assert got_var == -1, (what, "a winner at an infinite end", got_var)
        return 0
    assert got_var != -1, (what, "no winner at a finite end")
    inside = np.abs(r - end) <= tol * max(1.0, abs(end))
    w, wz = pos[inside], zero[inside]
    assert len(w), what
    allowed = [int(variables[p]) for p in w]
    assert int(got_var) in allowed, (what, "the winner is none of the positions at the end", int(got_var), allowed)
    if wz.all():  # every ratio is a zero: the tie is exact in any arithmetic, the lowest position wins
        assert int(got_var) == int(variables[w.min()]), (what, "exact tie: not the lowest position",
                                                         int(got_var), allowed)
        return int(len(w) >= 2)
    return 0


def check_ranges(got_lo, got_hi, got_lo_var, got_hi_var, want: Side, yardstick: Side, variables, what=""):
    """Holds one kind of ranges (cost: variables = nonbasis; rhs: variables = basis) to the long-double
    Side `want`, with numpy's double-precision Side of the same basis as the yardstick:

      endpoints  error <= max(C_DUALS * numpy's error, 1e-13), same metric; directions with a |delta|
                 within a factor 2 of pivot_tol are skipped, at most 2 % of them
      winners    W = the positions whose long-double r lies within that tolerance of the long-double
                 end: the variable returned is the variable of a member of W; where every member of W
                 has clamped value exactly 0 it is the variable at the lowest position of W; -1 goes
                 with an infinite end, and only with one

    Returns dict(err, yard, tol, ratio, skipped, directions, exact_ties)."""
    nd = len(want.ranges)
    assert len(got_lo) == len(got_hi) == len(got_lo_var) == len(got_hi_var) == nd == len(yardstick.ranges), what
    skipped = int(np.sum(want.near))
    assert skipped <= SKIP_CAP * nd, (what, skipped, nd)
    err = endpoint_error(got_lo, got_hi, want.ranges, want.near, what)
    yard = endpoint_error([w.lo for w in yardstick.ranges], [w.hi for w in yardstick.ranges], want.ranges,
                          want.near, what + " numpy")
    tol = max(C_DUALS * yard, FLOOR)
    assert tol <= CLOSE / 4, (what, tol)
    assert err <= tol, (what, err, tol)
    ties = 0
    for i, w in enumerate(want.ranges):
        if want.near[i]:
            continue
        ties += _check_winner(got_lo_var[i], w.lo, want.close_lo[i], variables, tol, f"{what} lo_var[{i}]")
        ties += _check_winner(got_hi_var[i], w.hi, want.close_hi[i], variables, tol, f"{what} hi_var[{i}]")
    return dict(err=err, yard=yard, tol=tol, ratio=err / max(yard, FLOOR / C_DUALS), skipped=skipped,
                directions=nd, exact_ties=ties)


def unit_and_pair_directions(seed, m, n, pairs=16, dense=True):
    """Every unit cost and rhs direction, `pairs` two-entry differences of each kind and one dense
    direction of each kind (coefficients multiples of 1/4 in [-2, 2] without 0)."""
    rng = np.random.default_rng(seed)
    cost = [{j: 1.0} for j in range(n)]
    rhs = [{r: 1.0} for r in range(m)]
    for _ in range(pairs):
        if n >= 2:
            i, j = rng.choice(n, 2, replace=False)
            cost.append({int(i): 1.0, int(j): -1.0})
        if m >= 2:
            i, j = rng.choice(m, 2, replace=False)
            rhs.append({int(i): 1.0, int(j): -1.0})
    if dense:
        def coef(size):
            return (rng.integers(1, 9, size) / 4.0 * rng.choice([-1.0, 1.0], size)).tolist()
        cost.append(dict(zip(rng.permutation(n).tolist(), coef(n))))
        rhs.append(dict(zip(rng.permutation(m).tolist(), coef(m))))
    return cost, rhs


# ---------------------------------------------------------------- the cases both test files use
SHAPES = [(64, 64, 20), (128, 192, 50), (33, 15, 9), (8, 4200, 6), (300, 520, 120)]
K_EDGES = [(70, 140, k) for k in (1, 63, 64, 65, 70)]
TIES = [(97, 161, 40, 6), (300, 520, 120, 8)]
OPTIMAL_CASES = [s + (0,) for s in SHAPES + K_EDGES] + TIES
RAY_SHAPES = [(64, 64, 20), (33, 15, 9), (300, 520, 120)]
RAY_KINDS = ["unbounded", "unbounded-slack", "infeasible", "infeasible-slack"]


def _seed(m, ns, k, g=0):
    return 7 + 1000 * m + 10 * k + g


def optimal_case(m, ns, k, g=0) -> Planted:
    """The planted optimum of a case.  A degenerate case of more than 256 rows has its zeros on both
    sides of position 256, half of each kind, so that a right-hand-side tie is decided across two
    row tiles of 256 positions."""
    seed = _seed(m, ns, k, g)
    if not g or m <= 256:
        return planted_optimal(seed, m, ns, k, degenerate=g)
    plain = planted_optimal(seed, m, ns, k)
    zeros = []
    for kind in (plain.basis < ns, plain.basis >= ns):
        low = np.flatnonzero(kind & (np.arange(m) < 256))
        high = np.flatnonzero(kind & (np.arange(m) >= 256))
        for part, count in ((low, g // 2), (high, g - g // 2)):  # spread over the tile
            zeros += part[np.linspace(0, len(part) - 1, count).astype(np.int64)].tolist()
    return planted_optimal(seed, m, ns, k, zero_positions=zeros)


def ray_case(kind, m, ns, k) -> Planted:
    make = planted_unbounded if kind.startswith("unbounded") else planted_infeasible
    return make(_seed(m, ns, k), m, ns, k, slack=kind.endswith("-slack"))
