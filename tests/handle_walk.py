"""A host mirror of a live core.Solver and the random walks it is driven through
(tests/test_handle_walk_host.py, tests/test_gpu_handle_walk.py).

`Mirror` holds what a handle on a dense LP holds: the LP in its slack start (a, c by variable, x = b by
row, z = -c[nonbasis], var_col, constant) and the state of the basis it stands at (basis, nonbasis, x,
xbar, z, zbar, status, iterations, objective, the accumulated pivot log).  Its four operations carry
the signatures of core.Solver's and are built from pieces the other tests already rely on:

    run(k)                    ora.simplex_solve from the carried state (k = 0: to the end)
    reoptimize(b, c, const)   new data, then the restart state
    extend(rows, rhs, ...)    core.extended_lp; new slacks after the basis, new variables after the
                              nonbasis; then the restart state
    remove(rows, cols)        core.reduced_lp on the slack-start LP; the lists renumbered through
                              var_map, survivors in order; then the restart state

The restart state is the STRICT one, bit for bit: x = ora.lu_solve(B, b), z = core_duals(...).d on the
nonbasics, xbar = zbar = 1, status running, counters and log kept.

`recipe(seed, m, ns, steps)` draws a list of operations against a mirror -- what is removable and which
status is current decide what can be drawn.  The base LP is reopt_check's feasible-and-bounded
construction in numpy: a uniform in [-1, 1], b = a x0 + rb, c = a^T y0 - rc.  The recipe keeps x0 and
y0 through the walk (new columns enter x0 at 0, new rows y0 at 0), so that b + d, c - e, rows with
rhs >= rows . x0 and columns with cost <= cols . y0 leave the LP solvable, and so that an LP that has
become infeasible or unbounded -- planted, or by a removal -- has a repair: b raised to a x0 + r where
it is below, c lowered to a^T y0 - r where it is above, or the planted rows / column removed once free.
"""
from __future__ import annotations

import dataclasses
from types import SimpleNamespace

import numpy as np

from dantzig_amd import core
from oracle import oracle as ora
from tests import duals_reference as dref
from tests import extend_check as ec
from tests import remove_check as rmc
from tests import state_check as sc

RESTARTS = ("reoptimize", "extend", "remove")
STATUSES = ("running", "iter_limit", "optimal", "unbounded", "infeasible")
ORACLE_MAX = 1_000_000


def ceil16(m: int) -> int:
    return (int(m) + 15) // 16 * 16


@dataclasses.dataclass
class Op:
    call: str            # run | reoptimize | extend | remove
    kind: str            # what the recipe drew, for the coverage counts
    kw: dict             # the keyword arguments of the call (run: {"max_new_iters": k})


def snapshot(st) -> SimpleNamespace:
    """basis, nonbasis, x, xbar, z, zbar of a Mirror or a CoreResult, copied."""
    return SimpleNamespace(**{k: np.array(getattr(st, k)) for k in ("basis", "nonbasis", "x", "xbar", "z", "zbar")})


class Mirror:
    def __init__(self, a, b, c, constant: float = 0.0, max_iter: int = 0):
        self.lp = core.CoreLP.from_inequality_form(np.array(a, dtype=np.float64), b, c, constant)
        self.max_iter = int(max_iter)
        self.basis, self.nonbasis = self.lp.basis.copy(), self.lp.nonbasis.copy()
        self.x, self.z = self.lp.x.copy(), self.lp.z.copy()
        self.xbar, self.zbar = np.ones(self.lp.m), np.ones(self.lp.n - self.lp.m)
        self.status, self.iterations, self.pivots = "running", 0, []
        self.runs = 0
        self.start = snapshot(self)        # the state the carried one descends from
        self.objective = self._objective()

    # ------------------------------------------------------------------ pieces
    def dims(self):
        return self.lp.m, self.lp.n, self.lp.n_struct

    def stdform(self):
        sf = sc.stdform(self.lp.a, self.lp.n_struct, self.lp.c, self, self.lp.var_col)
        sf.constant = float(self.lp.constant)
        return sf

    def at_basis(self) -> core.CoreLP:
        """The LP with the lists of the current basis (x and z stay the slack start's)."""
        return dataclasses.replace(self.lp, basis=self.basis.copy(), nonbasis=self.nonbasis.copy())

    def removable(self):
        return rmc.free_masks(self.at_basis())

    def _objective(self) -> float:
        return ora.simplex_solve(self.stdform(), max_iter=0, xbar=self.xbar, zbar=self.zbar).objective

    def _restart(self):
        st = host_restart(self, self.basis, self.nonbasis)
        self.x, self.z, self.xbar, self.zbar = st.x, st.z, st.xbar, st.zbar
        self.status = "running"
        self.start = snapshot(self)
        self.objective = self._objective()

    # ------------------------------------------------------------------ the four operations
    def run(self, max_new_iters: int = 0) -> str:
        if self.status not in ("running", "iter_limit"):
            return self.status
        self.runs += 1
        budget = int(max_new_iters) if max_new_iters > 0 else ORACLE_MAX
        if self.max_iter > 0:
            budget = max(0, min(budget, self.max_iter - self.iterations))
        res = ora.simplex_solve(self.stdform(), max_iter=budget, xbar=self.xbar, zbar=self.zbar)
        self.basis, self.nonbasis = res.basis, res.nonbasis
        self.x, self.xbar, self.z, self.zbar = res.x, res.xbar, res.z, res.zbar
        self.pivots += [(int(k), int(e), int(l), float(mu)) for k, e, l, mu in res.pivots]
        self.iterations += int(res.iterations)
        self.status, self.objective = res.status, res.objective
        return self.status

    def reoptimize(self, b=None, c=None, constant=None) -> None:
        lp = self.lp
        b = lp.x if b is None else np.array(b, dtype=np.float64)
        c = lp.c if c is None else np.array(c, dtype=np.float64)
        assert b.shape == (lp.m,) and c.shape == (lp.n,)
        self.lp = dataclasses.replace(lp, x=b, c=c, z=-c[lp.nonbasis],
                                      constant=lp.constant if constant is None else float(constant))
        self._restart()

    def extend(self, rows=None, rhs=None, cols=None, c_cols=None) -> None:
        n = self.lp.n
        self.lp = core.extended_lp(self.lp, rows, rhs, cols, c_cols)
        p, r = self.lp.m - len(self.basis), self.lp.n_struct - len(self.nonbasis)
        self.basis = np.concatenate([self.basis, n + r + np.arange(p)]).astype(np.int64)
        self.nonbasis = np.concatenate([self.nonbasis, n + np.arange(r)]).astype(np.int64)
        self._restart()

    def remove(self, rows=None, cols=None):
        core.reduced_lp(self.at_basis(), rows, cols)           # ValueError for what is not free
        self.lp, var_map, row_map = core.reduced_lp(self.lp, rows, cols)
        self.basis = var_map[self.basis[var_map[self.basis] >= 0]]
        self.nonbasis = var_map[self.nonbasis[var_map[self.nonbasis] >= 0]]
        self._restart()
        return var_map, row_map


def host_restart(mir: Mirror, basis, nonbasis) -> SimpleNamespace:
    """The STRICT restart state of a basis on the mirror's LP: x = lu_solve(B, b), z = core_duals(...).d on the
    nonbasics, as tests/test_gpu_extend.py forms them; xbar = zbar = 1."""
    lp = mir.lp
    basis, nonbasis = np.asarray(basis, dtype=np.int64), np.asarray(nonbasis, dtype=np.int64)
    st = SimpleNamespace(basis=basis, nonbasis=nonbasis, z=np.zeros(len(nonbasis)), xbar=np.ones(lp.m),
                         zbar=np.ones(lp.n - lp.m))
    st.x = ora.lu_solve(sc.columns(lp.a, lp.m, ec.codes_of(lp)[basis]), lp.x)
    sf = sc.stdform(lp.a, lp.n_struct, lp.c, st, lp.var_col)
    sf.constant = float(lp.constant)
    st.z = dref.core_duals(sf, st).d[nonbasis]
    return st


def apply(target, op: Op):
    """One operation on a Mirror or a core.Solver."""
    if op.call == "run":
        return target.run(op.kw["max_new_iters"])
    return getattr(target, op.call)(**op.kw)


# ---------------------------------------------------------------------- the recipe
def base_lp(rng, m: int, ns: int):
    """(a, b, c, x0, y0): feasible at x0, dual feasible at y0."""
    a = rng.uniform(-1.0, 1.0, (m, ns))
    x0, y0, rb, rc = rng.random(ns), rng.random(m), rng.random(m), rng.random(ns)
    return a, a @ x0 + rb, a.T @ y0 - rc, x0, y0


KINDS = ["run", "stop", "move_b", "move_c", "add_rows", "add_cols", "add_both", "drop_rows", "drop_cols",
         "drop_both", "plant_infeasible", "plant_unbounded"]
WEIGHTS = [0.20, 0.12, 0.09, 0.09, 0.10, 0.07, 0.05, 0.07, 0.07, 0.05, 0.045, 0.045]


def _c_by_column(lp, c_cols):
    """c by variable from costs by structural column (slacks cost 0)."""
    codes = ec.codes_of(lp)
    return np.where(codes >= 0, np.asarray(c_cols)[np.maximum(codes, 0)], 0.0)


def recipe(seed: int, m: int, ns: int, steps: int, m_range=(4, 40), ns_range=(4, 48)):
    """(a, b, c, ops): the base LP and `steps` operations, the last one a run to the end."""
    rng = np.random.default_rng(seed)
    a, b, c, x0, y0 = base_lp(rng, m, ns)
    mir = Mirror(a, b, c)
    pair, ray_col = None, None        # the planted rows / column, in today's numbering
    ops = []

    def columns_cost():
        c_col = np.zeros(mir.lp.n_struct)
        codes = ec.codes_of(mir.lp)
        s = np.flatnonzero(codes >= 0)
        c_col[codes[s]] = mir.lp.c[s]
        return c_col

    def relax_b():
        return Op("reoptimize", "repair_b", dict(b=np.maximum(mir.lp.x, mir.lp.a @ x0 + rng.random(mir.lp.m))))

    def lower_c():
        c_col = np.minimum(columns_cost(), mir.lp.a.T @ y0 - rng.random(mir.lp.n_struct))
        return Op("reoptimize", "repair_c", dict(c=_c_by_column(mir.lp, c_col)))

    def draw(kind):
        nonlocal pair, ray_col
        lp = mir.lp
        m, ns = lp.m, lp.n_struct
        if kind == "run":
            return Op("run", kind, dict(max_new_iters=0))
        if kind == "stop":
            return Op("run", kind, dict(max_new_iters=int(rng.integers(1, 8))))
        if kind == "move_b":
            return Op("reoptimize", kind, dict(b=lp.x + rng.random(m)))
        if kind == "move_c":
            kw = dict(c=_c_by_column(lp, columns_cost() - rng.random(ns)))
            if rng.random() < 0.5:
                kw["constant"] = float(rng.integers(-4, 5)) / 4
            return Op("reoptimize", kind, kw)
        if kind in ("add_rows", "add_cols", "add_both"):
            p = int(rng.integers(1, 4)) if kind != "add_cols" else 0
            r = int(rng.integers(1, 4)) if kind != "add_rows" else 0
            if m + p > m_range[1] or ns + r > ns_range[1]:
                return None
            kw = {}
            if p:
                rows = rng.uniform(-1.0, 1.0, (p, ns))
                rows[p // 2, ns // 2] = -0.0
                kw.update(rows=rows, rhs=rows @ x0 + 0.5 * rng.random(p))
            if r:
                cols = rng.uniform(-1.0, 1.0, (m + p, r))
                cols[(m + p) // 2, r // 2] = -0.0
                kw.update(cols=cols, c_cols=cols[:m].T @ y0 - 0.5 * rng.random(r))
            return Op("extend", kind, kw)
        if kind.startswith("drop"):
            free_rows, free_cols = (np.flatnonzero(v) for v in mir.removable())
            rows, cols = [], []
            if kind != "drop_cols" and len(free_rows):
                k = int(rng.integers(1, min(len(free_rows), 5) + 1))
                rows = sorted(rng.choice(free_rows, k, replace=False).tolist())
            if kind != "drop_rows" and len(free_cols):
                k = int(rng.integers(1, min(len(free_cols), 5) + 1))
                cols = sorted(rng.choice(free_cols, k, replace=False).tolist())
            if (kind == "drop_both" and not (rows and cols)) or not (rows or cols):
                return None
            if m - len(rows) < m_range[0] or ns - len(cols) < ns_range[0]:
                return None
            return Op("remove", kind, dict(rows=rows or None, cols=cols or None))
        if kind == "plant_infeasible":
            if pair is not None or m + 2 > m_range[1]:
                return None
            pair = [m, m + 1]
            return Op("extend", kind, dict(rows=np.array([np.ones(ns), -np.ones(ns)]), rhs=np.array([1.0, -2.0])))
        if kind == "plant_unbounded":
            if ray_col is not None or ns + 1 > ns_range[1]:
                return None
            ray_col = ns
            return Op("extend", kind, dict(cols=-np.ones((m, 1)), c_cols=np.array([1.0])))
        raise ValueError(kind)

    def repair():
        nonlocal pair, ray_col
        free_rows, free_cols = mir.removable()
        if mir.status == "infeasible":
            if pair is not None and free_rows[pair].all() and rng.random() < 0.6:
                return Op("remove", "repair_remove_rows", dict(rows=list(pair), cols=None))
            return relax_b()
        if ray_col is not None and free_cols[ray_col] and rng.random() < 0.6:
            return Op("remove", "repair_remove_col", dict(rows=None, cols=[ray_col]))
        return lower_c()

    def follow(op):
        """x0, y0 and the planted indices through the operation just drawn."""
        nonlocal x0, y0, pair, ray_col
        if op.call == "extend":
            y0 = np.concatenate([y0, np.zeros(len(op.kw.get("rhs", ())))])
            x0 = np.concatenate([x0, np.zeros(len(op.kw.get("c_cols", ())))])
        elif op.call == "remove":
            rows, cols = op.kw["rows"] or [], op.kw["cols"] or []
            keep_r, keep_c = np.ones(len(y0), bool), np.ones(len(x0), bool)
            keep_r[rows], keep_c[cols] = False, False
            row_map, col_map = np.cumsum(keep_r) - 1, np.cumsum(keep_c) - 1
            if pair is not None:
                pair = None if not keep_r[pair].all() else [int(row_map[i]) for i in pair]
            if ray_col is not None:
                ray_col = None if not keep_c[ray_col] else int(col_map[ray_col])
            x0, y0 = x0[keep_c], y0[keep_r]
        elif op.kind == "repair_b":
            pair = None                # relaxed: ordinary rows from now on
        elif op.kind == "repair_c":
            ray_col = None

    for step in range(steps):
        op = None
        if step == steps - 1:
            op = draw("run")
        elif step == steps - 2:        # the change the last run answers
            if mir.status in ("infeasible", "unbounded") or pair is not None or ray_col is not None:
                op = relax_b() if (mir.status == "infeasible" or pair is not None) else lower_c()
            else:
                op = draw(("move_b", "move_c")[int(rng.integers(0, 2))])
        elif mir.status in ("infeasible", "unbounded") and rng.random() < 0.5:
            op = repair()
        while op is None:
            op = draw(KINDS[int(rng.choice(len(KINDS), p=WEIGHTS))])
        follow(op)
        apply(mir, op)
        ops.append(op)
    return a, b, c, ops


# ---------------------------------------------------------------------- the walks
@dataclasses.dataclass(frozen=True)
class Walk:
    name: str
    seed: int
    m: int
    ns: int
    steps: int
    m_range: tuple = (4, 40)
    ns_range: tuple = (4, 48)

    def recipe(self):
        return recipe(self.seed, self.m, self.ns, self.steps, self.m_range, self.ns_range)


SMALL = [Walk(f"14x20 seed {s}", s, 14, 20, 40) for s in (1, 2, 55, 119)]
LARGE = Walk("60x70 seed 59", 59, 60, 70, 25, (4, 72), (4, 80))
WALKS = SMALL + [LARGE]
CAPPED = SMALL[0]          # the walk of the max_iter test

def exact_restart(mir: Mirror, basis=None, nonbasis=None):
    """The long-double state of a basis (default: the mirror's) on the mirror's LP: what a restart is held to."""
    lp = mir.lp
    return sc.exact_state(lp.a, lp.n_struct, lp, mir.basis if basis is None else basis,
                          mir.nonbasis if nonbasis is None else nonbasis, lp.var_col)


def exact_carried(mir: Mirror, basis=None, nonbasis=None):
    """The long-double state of a basis reached by pivots from the mirror's last restart state."""
    lp = mir.lp
    return sc.exact_state(lp.a, lp.n_struct, mir.start, mir.basis if basis is None else basis,
                          mir.nonbasis if nonbasis is None else nonbasis, lp.var_col)


def capped(walk: "Walk"):
    """(a, b, c, ops, total): the walk's first 20 steps, then a new right-hand side and a run to the end,
    for a handle created with max_iter = total, the pivot count after step 20.  That handle does what an
    unbounded one does for 20 steps and must then stop at once: opts.max_iter bounds the total."""
    a, b, c, ops = recipe_of(walk)
    mir = Mirror(a, b, c)
    for op in ops[:20]:
        apply(mir, op)
    rng = np.random.default_rng(walk.seed + 1000)
    tail = [Op("reoptimize", "move_b", dict(b=mir.lp.x + rng.random(mir.lp.m))), Op("run", "run", dict(max_new_iters=0))]
    return a, b, c, ops[:20] + tail, mir.iterations


_recipes = {}


def recipe_of(walk: Walk):
    """The walk's (a, b, c, ops), drawn once and shared; nothing in it is written to afterwards."""
    if walk not in _recipes:
        _recipes[walk] = walk.recipe()
    return _recipes[walk]
