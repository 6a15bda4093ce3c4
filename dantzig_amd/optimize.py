"""Minimize / Maximize / Solution (python-source/dantzig/optimize.py:8-154).

The core always maximises: Minimize negates the objective on the way in and the optimal value
on the way out (optimize.py:114-117, :21-27).  A model with an integer variable is solved by
branch and bound (rust.solve_mip); Solution.mip then reports the search in the user's sense.
solve(duals=True) adds dual values, reduced costs and an optimality certificate, in the user's sense
too: Solution.dual(constraint), Solution.reduced_cost(variable), Solution.certificate.
solve(ranging=True) adds how far those slopes hold: Solution.rhs_range(constraint) and
Solution.objective_range(variable)."""
from __future__ import annotations

import abc
import ctypes as C
from dataclasses import dataclass
from typing import Union

import numpy as np

from . import _ffi, core
from . import rust as rs
from .exceptions import InfeasibleError, SolveError, UnboundedError
from .model import AffExpr, Constraint, LinExpr, Variable

_SENSES = ("minimize", "maximize")


@dataclass(frozen=True)
class Certificate:
    """The optimality certificate of one solve(duals=True), objectives in the user's sense.  source:
    "fresh" (duals recomputed on the GPU from the final basis) or "carried" (read off the carried
    reduced costs); gap = primal_objective - dual_objective; z_diff: how far the carried reduced
    costs are from the recomputed ones, relative."""
    source: str
    primal_objective: float
    dual_objective: float
    gap: float
    primal_infeasibility: float
    dual_infeasibility: float
    z_diff: float


@dataclass(frozen=True)
class Range:
    """The closed interval [lo, hi] of a constraint's b or of a variable's objective coefficient over
    which the optimal basis holds (-inf / +inf where nothing blocks); the current value is inside."""
    lo: float
    hi: float


class _Ray:
    """Common to PrimalRay and FarkasRay: the model's constraints (kept alive, found by identity) and
    the first row of each, as Solution keeps them."""

    def __init__(self, *, ray: "rs.PyRay", sense: str, constraints) -> None:
        self._ray = ray
        self._sense = sense
        self._rows: dict = {}
        row = 0
        for constraint in constraints:
            self._rows.setdefault(id(constraint), (constraint, row))
            row += len(constraint.rust_inequalities())

    def _first_row(self, constraint: Constraint) -> int:
        entry = self._rows.get(id(constraint))
        if entry is None:
            raise KeyError("the constraint is not part of the solved model")
        return entry[1]

    @property
    def violation(self) -> float:
        """How far the ray's sign conditions are missed (0.0: not at all; NaN: the ray holds a NaN)."""
        return self._ray.violation

    @property
    def proven(self) -> bool:
        """True when the ray, as computed, proves the verdict: no violation and the right sign of
        objective_rate / rhs_value.  False: the solver said so, the ray does not show it."""
        return self._ray.proven


class PrimalRay(_Ray):
    """UnboundedError.ray of a solve(rays=True): a direction along which every feasible point can move
    for ever while the objective improves."""

    def direction(self, variable: Variable) -> float:
        return self._ray.var.get(variable.to_rust_variable().id, 0.0)

    def slack_rate(self, constraint: Constraint) -> list:
        """How fast the slack of each row of `constraint` (linexpr <= b as lowered) grows along the
        ray; negative: the row would be left."""
        first = self._first_row(constraint)
        return [self._ray.con[first + k] for k in range(len(constraint._signs))]

    @property
    def objective_rate(self) -> float:
        """The change of the objective per unit of the ray, in the user's sense: positive under
        Maximize, negative under Minimize for a proven ray."""
        return -self._ray.value if self._sense == "minimize" else self._ray.value

    def __repr__(self) -> str:
        return f"PrimalRay(proven={self.proven}, objective_rate={self.objective_rate!r}, violation={self.violation!r})"


class FarkasRay(_Ray):
    """InfeasibleError.ray of a solve(rays=True): multipliers >= 0 on the rows `linexpr <= b` whose
    combination has coefficient zero on every variable and a negative right-hand side."""

    def multiplier(self, constraint: Constraint) -> float:
        """The multiplier of `constraint` in its normal form linexpr <=, >= or == b: >= 0 for <=, <= 0
        for >=, either sign for ==."""
        first = self._first_row(constraint)
        value = 0.0
        for k, sign in enumerate(constraint._signs):
            value += sign * self._ray.con[first + k]
        return value

    def bound_multipliers(self, variable: Variable) -> tuple:
        """(lb, ub): the multipliers of the rows -x <= -lb and x <= ub of `variable`, 0.0 where the
        bound is absent."""
        vid = variable.to_rust_variable().id
        return self._ray.lb.get(vid, 0.0), self._ray.ub.get(vid, 0.0)

    def aggregated(self, variable: Variable) -> float:
        """The coefficient of `variable` in the combined row (zero up to rounding for a proof)."""
        return self._ray.var.get(variable.to_rust_variable().id, 0.0)

    @property
    def rhs_value(self) -> float:
        """The right-hand side of the combined row; negative for a proven ray."""
        return self._ray.value

    def __repr__(self) -> str:
        return f"FarkasRay(proven={self.proven}, rhs_value={self.rhs_value!r}, violation={self.violation!r})"


class Solution:
    def __init__(self, *, solution: rs.PySolution, sense: str, constraints=None, objective=None) -> None:
        if sense not in _SENSES:
            raise ValueError(f"sense is {sense!r}; a Solution is built for {_SENSES[0]!r} or {_SENSES[1]!r}")
        self._solution = solution
        self._sense = sense
        # duals: the model's constraints (kept alive, found by identity) and the first row of each
        self._rows: dict = {}
        row = 0
        for constraint in constraints or []:
            self._rows.setdefault(id(constraint), (constraint, row))
            row += len(constraint.rust_inequalities())
        # ranging: the model's objective (the coefficients the ranges are about), user's sense
        self._objective = objective

    def _duals(self) -> "rs.PyDuals":
        duals = getattr(self._solution, "duals", None)
        if duals is None:
            raise RuntimeError("this Solution carries no dual values: ask for them with solve(duals=True)")
        return duals

    def dual(self, constraint: Constraint) -> float:
        """d objective_value / d b of `constraint` in its normal form linexpr <=, >= or == b."""
        duals = self._duals()
        entry = self._rows.get(id(constraint))
        if entry is None:
            raise KeyError("the constraint is not part of the solved model")
        first = entry[1]
        value = 0.0
        for k, sign in enumerate(constraint._signs):
            value += sign * duals.con_dual[first + k]
        return -value if self._sense == "minimize" else value

    def reduced_cost(self, variable: Variable) -> float:
        """The objective coefficient of `variable` less its constraints' duals times its coefficients
        (bound rows left out), in the user's sense."""
        value = self._duals().var_rc[variable.to_rust_variable().id]
        return -value if self._sense == "minimize" else value

    def _ranging(self) -> "rs.PyRanging":
        ranging = getattr(self._solution, "ranging", None)
        if ranging is None:
            raise RuntimeError("this Solution carries no ranges: ask for them with solve(ranging=True)")
        return ranging

    def rhs_range(self, constraint: Constraint) -> Range:
        """The values of the constraint's own b, in its written form linexpr <=, >= or == b, over which
        the optimal basis holds: inside it the objective moves by dual(constraint) per unit of b."""
        ranging = self._ranging()
        entry = self._rows.get(id(constraint))
        if entry is None:
            raise KeyError("the constraint is not part of the solved model")
        group = list(self._rows).index(id(constraint))
        # the user's b from the first row: b as written if its sign is +1, the negated row's -b otherwise
        b = constraint._signs[0] * constraint.rust_inequalities()[0]._b
        return Range(b + ranging.group_lo[group], b + ranging.group_hi[group])

    def objective_range(self, variable: Variable) -> Range:
        """The values of the objective coefficient of `variable` over which the optimal basis holds:
        inside it the solution stays and the objective moves by solution[variable] per unit."""
        ranging = self._ranging()
        key = variable.to_rust_variable().id
        if key not in ranging.var_lo:
            raise KeyError("the variable is not part of the solved model")
        coef = self._objective.linexpr.map_ids_to_coefs().get(key, 0.0)
        lo, hi = ranging.var_lo[key], ranging.var_hi[key]
        if self._sense == "minimize":  # the core's coefficient is -coef: its step t is -(the user's)
            lo, hi = -hi, -lo
        return Range(coef + lo, coef + hi)

    @property
    def certificate(self) -> Certificate:
        duals = self._duals()
        flip = -1.0 if self._sense == "minimize" else 1.0
        primal, dual = flip * duals.primal_objective, flip * duals.dual_objective
        return Certificate(source=duals.source, primal_objective=primal, dual_objective=dual,
                           gap=primal - dual, primal_infeasibility=duals.primal_infeasibility,
                           dual_infeasibility=duals.dual_infeasibility, z_diff=duals.z_diff)

    @property
    def objective_value(self) -> float:
        value = self._solution.objective_value
        return -value if self._sense == "minimize" else value

    def __getitem__(self, variable: Variable) -> float:
        return self._solution[variable.to_rust_variable()]

    @property
    def mip(self):
        """None for an LP.  For a model with integer variables: the search's MipInfo (status,
        nodes, rounds, lp_iterations, best_bound, gap), best_bound in the user's sense."""
        info = self._solution.mip
        if info is None or self._sense == "maximize":
            return info
        flipped = rs.MipInfo(**{k: getattr(info, k) for k in rs.MipInfo.__slots__})
        flipped.best_bound = -info.best_bound
        flipped.objective = None if info.objective is None else -info.objective
        return flipped


class Optimize(abc.ABC):
    """Common part of Minimize and Maximize: objective, constraint list, chaining."""

    def __init__(self, objective: Union[Variable, LinExpr, AffExpr]) -> None:
        self.objective = objective.to_affexpr()
        self.constraints: list = []

    @property
    @abc.abstractmethod
    def sense(self) -> str:
        raise NotImplementedError

    def subject_to(self, constraints):
        """Add one constraint or a list of constraints; returns self for chaining."""
        batch = [constraints] if isinstance(constraints, Constraint) else constraints
        if not isinstance(batch, list):  # like the reference, list items are not inspected here
            raise TypeError("subject_to takes a Constraint or a list of Constraints, got "
                            f"{type(constraints).__name__}")
        self.constraints += batch
        return self

    st = subject_to

    def yield_rust_inequalities(self):
        for constraint in self.constraints:
            yield from constraint.rust_inequalities()

    def _core_objective(self) -> AffExpr:
        return -self.objective if self.sense == "minimize" else self.objective

    def _rust_problem(self):
        return self._core_objective().to_rust_affexpr(), list(self.yield_rust_inequalities())

    def _row_groups(self) -> list:
        """One group of rows per constraint: its rows with Constraint._signs as coefficients, so that
        the group's step is the change of the constraint's own b."""
        groups, seen, row = [], set(), 0
        for constraint in self.constraints:
            n = len(constraint.rust_inequalities())
            if id(constraint) not in seen:  # (a constraint added twice: Solution keeps its first rows)
                seen.add(id(constraint))
                groups.append([(row + k, sign) for k, sign in enumerate(constraint._signs)])
            row += n
        return groups

    def _wrap_ray(self, exc: Exception) -> Exception:
        """The exception of a solve(rays=True) with its core ray in this model's terms."""
        ray = getattr(exc, "ray", None)
        if isinstance(ray, rs.PyRay):
            cls = PrimalRay if ray.kind == "primal" else FarkasRay
            exc.ray = cls(ray=ray, sense=self.sense, constraints=list(self.constraints))
        return exc

    def solve(self, *, duals: bool = False, ranging: bool = False, rays: bool = False) -> Solution:
        """Solve on the GPU.  Raises exceptions.UnboundedError / InfeasibleError.  duals=True: the
        Solution also answers dual(), reduced_cost() and certificate (LPs only: ValueError for a
        model with an integer variable).  ranging=True (implies duals): also rhs_range() and
        objective_range(); NotImplementedError where the solve's route has no ranging.  rays=True
        (composes with duals; ValueError with ranging or an integer variable): the UnboundedError
        carries `.ray`, a PrimalRay, the InfeasibleError a FarkasRay; `.ray.proven` says whether the
        verdict checks out.  `.ray` stays None where the solve's route has no rays."""
        objective, constraints = self._rust_problem()
        if rays and ranging:
            raise ValueError("rays=True and ranging=True: the ranging call carries no ray; ask in two calls")
        if rays:
            if rs._has_integer(objective, constraints):
                raise ValueError("rays=True: rays are not defined for a model with integer variables")
            try:
                return Solution(solution=rs.solve(objective, constraints, duals=duals, rays=True),
                                sense=self.sense, constraints=list(self.constraints) if duals else None)
            except SolveError as exc:
                raise self._wrap_ray(exc)
        if rs._has_integer(objective, constraints):
            if ranging:
                raise ValueError("ranging=True: ranges are not defined for a model with integer variables")
            if duals:
                raise ValueError("duals=True: dual values are not defined for a model with integer variables")
            return Solution(solution=rs.solve_mip(objective, constraints), sense=self.sense)
        if ranging:
            return Solution(solution=rs.solve(objective, constraints, ranging=self._row_groups()),
                            sense=self.sense, constraints=list(self.constraints), objective=self.objective)
        if duals:
            return Solution(solution=rs.solve(objective, constraints, duals=True), sense=self.sense,
                            constraints=list(self.constraints))
        return Solution(solution=rs.solve(objective, constraints), sense=self.sense)

    def session(self, **core_opts) -> "Session":
        """A Session on this model: its solve() keeps the model on the GPU, and later
        solve(objective=..., rhs=...) calls re-optimise from the last basis instead of starting over.
        core_opts: fields of dzg_opts (numerics, max_iter, ...) over rust.set_options()'s.  ValueError
        for a model with an integer variable."""
        return Session(self, **core_opts)


def _model_rows(constraints, rhs: dict) -> list:
    """The rows of `constraints` with the right-hand sides of `rhs` ({id(constraint): the new b of its
    normal form}): row k of a changed constraint is its linear part as lowered with
    b = Constraint._signs[k] * (the new b)."""
    rows = []
    for constraint in constraints:
        b = rhs.get(id(constraint))
        for ineq, sign in zip(constraint.rust_inequalities(), constraint._signs):
            rows.append(ineq if b is None else rs.PyInequality(linexpr=ineq._linexpr, b=sign * b))
    return rows


def _lower_model(sense: str, objective, rows: list):
    """(the core problem, lower()'s arrays, the variables in lowering order) of a model in `sense`:
    the lowering Session and SessionBatch share."""
    objective = -objective if sense == "minimize" else objective
    problem = (objective.to_rust_affexpr(), rows)
    arrays, order = rs.lower(*problem)
    return problem, arrays, order


def _normal_b(b) -> float:
    """As a comparison forms it, b = -(constant of lhs - rhs): a written 0 arrives as -0.0."""
    return -(0.0 - float(b))


def _user_values(res, form, order) -> dict:
    """{variable id: x+ - x-} of a core result on the standard form `form` (src/simplex.rs:354-371)."""
    by_var = dict(zip(res.basis.tolist(), res.x.tolist()))
    return {v.id: by_var.get(int(form.pos_var[i]), 0.0) - by_var.get(int(form.neg_var[i]), 0.0)
            for i, v in enumerate(order)}


# what dzg_solver_reoptimize / _extend / _remove say when the handle's basis is the obstacle
_NO_CARRY_ON = ("did not refactorise", "cannot be carried on from")


class Session:
    """A model kept on the GPU between solves (Optimize.session): the first solve() lowers the model,
    uploads it and solves it from the slack basis; every later solve(objective=..., rhs=...) changes
    the objective and / or right-hand sides and re-optimises from the basis the last solve ended on
    (core.Solver.reoptimize), without a new upload.  Changes accumulate.  add_constraints() appends
    constraints over the model's variables: the next solve() extends the live solver by their rows
    (core.Solver.extend: the resident matrix grows on the GPU) and carries on from the same basis.
    remove_constraints() takes constraints away again: one that add_constraints put on the live solver
    and that is slack at the current basis leaves it on the GPU (core.Solver.remove) and the solve
    carries on from the same basis; any other removal -- a constraint of the original model, a
    binding one -- makes the next solve() a cold rebuild from the slack basis (counted in `rebuilds`).
    A solve() whose live solver cannot restart from its last basis (a singular or panic end; a FAST
    end on a basis that does not refactorise) starts over from the slack basis too (`restarts`).
    Besides that only b and the objective may change: variable bounds, the coefficients of an existing
    row, new variables and integer variables are out of scope.

    Numerics is the handle's: AUTO runs STRICT up to auto_strict_rows rows, else FAST with near
    ties counted.  A re-optimised path is not the reference's path from the slack basis, so the
    promise is the optimum (or the verdict), not the pivots, and at a degenerate optimum possibly
    another vertex.  `pivots` lists the pivots of each solve."""

    def __init__(self, problem: "Optimize", **core_opts) -> None:
        self._problem = problem
        self._constraints = list(problem.constraints)
        self._objective = problem.objective
        self._rhs: dict = {}   # id(constraint) -> the new b of its normal form
        self._added: list = []  # constraints added to a live solver, in the order of their rows
        self._extended = 0      # ... of which the solver holds this many already
        self._removed: list = []  # constraints to take off the live solver at the next solve
        self.rebuilds = 0         # cold rebuilds remove_constraints has caused
        self.restarts = 0         # cold starts because the last basis could not be carried on from
        self._opts = {**rs._options, **core_opts}
        self._opts.setdefault("refactor_interval", -1)  # (FAST: reserves what reoptimize needs)
        self._solver = None
        self._form = None
        self._order = None
        self._iterations = 0
        self.pivots: list = []
        self._check_lp(self._lowered()[0])

    @staticmethod
    def _check_lp(problem) -> None:
        if rs._has_integer(*problem):
            raise ValueError("session: re-optimisation is not defined for a model with integer variables")

    def _inequalities(self) -> list:
        """The model's rows with the right-hand sides of the session: row k of a changed constraint is
        its linear part as lowered with b = Constraint._signs[k] * (the new b of the normal form)."""
        return _model_rows(self._constraints, self._rhs)

    def _lowered(self):
        return _lower_model(self._problem.sense, self._objective, self._inequalities())

    def add_constraints(self, constraints) -> "Session":
        """Add one constraint or a list of constraints over variables the model already has.  Before
        the first solve() they simply join the model.  After it, the next solve() appends their rows
        below the rows the solver holds (the model's, then the bound rows, then earlier additions),
        and re-optimises from the last basis; solve(rhs={constraint: b}) works on them as on any
        other.  ValueError for a variable the model has not seen, for an integer variable and for a
        constraint that is already part of the session; nothing is added then.  A constraint that
        remove_constraints has taken away since the last solve() is simply kept."""
        batch = [constraints] if isinstance(constraints, Constraint) else constraints
        if not isinstance(batch, list) or not all(isinstance(c, Constraint) for c in batch):
            raise TypeError("add_constraints takes a Constraint or a list of Constraints")
        leaving = {id(c) for c in self._removed}
        known = {id(c) for c in self._constraints + self._added} - leaving
        order = self._order if self._solver is not None else self._lowered()[2]
        seen = {v.id for v in order}
        for k, constraint in enumerate(batch):
            if id(constraint) in known or any(constraint is c for c in batch[:k]):
                raise ValueError("add_constraints: the constraint is already part of the session")
            for ineq in constraint.rust_inequalities():
                if any(v.is_integer for v in ineq._linexpr.vars):
                    raise ValueError("add_constraints: integer variables are not defined for a session")
                if any(v.id not in seen for v in ineq._linexpr.vars):
                    raise ValueError("add_constraints: the constraint uses a variable the model has not seen "
                                     "(adding variables is a core-level feature: core.Solver.extend)")
        if self._solver is None:
            self._constraints += batch
        else:
            back = {id(c) for c in batch} & leaving    # (still on the solver: the removal is called off)
            self._removed = [c for c in self._removed if id(c) not in back]
            self._added += [c for c in batch if id(c) not in back]
        return self

    def remove_constraints(self, constraints) -> "Session":
        """Remove one constraint or a list of constraints the session holds.  Before the first solve()
        they simply leave the model.  After it, the next solve() drops them from the live solver on
        the GPU (core.Solver.remove) and re-optimises from the same basis when every one of them was
        added by add_constraints and every one of their rows has a basic slack at the current basis
        (the constraint is not binding there); those rows sit below the model's, so no other index
        moves.  In every other case -- a constraint of the original model, a binding one -- the
        session closes its solver, lowers the model without the constraints and the next solve()
        starts from the slack basis: the result is the same, the basis is lost; `rebuilds` counts
        these and `pivots` shows what they cost.  A removed constraint may be added again later.
        KeyError for a constraint the session does not hold (or one listed twice); nothing is removed
        then."""
        batch = [constraints] if isinstance(constraints, Constraint) else constraints
        if not isinstance(batch, list) or not all(isinstance(c, Constraint) for c in batch):
            raise TypeError("remove_constraints takes a Constraint or a list of Constraints")
        held = {id(c) for c in self._constraints + self._added} - {id(c) for c in self._removed}
        for k, constraint in enumerate(batch):
            if id(constraint) not in held or any(constraint is c for c in batch[:k]):
                raise KeyError("the constraint is not part of the session's model")
        gone = {id(c) for c in batch}
        if self._solver is None:
            self._constraints = [c for c in self._constraints if id(c) not in gone]
            for key in gone:
                self._rhs.pop(key, None)
        else:
            self._removed += batch
        return self

    def _apply_removals(self) -> None:
        """What remove_constraints left for the next solve: off the live solver if that is free,
        else the solver goes and the model is lowered again without them."""
        if not self._removed:
            return
        gone = {id(c) for c in self._removed}
        self._removed = []
        rows, at = [], self._form.m
        for constraint in self._added[:self._extended]:   # the rows the solver holds below the form's
            k = len(constraint.rust_inequalities())
            if id(constraint) in gone:
                rows += range(at, at + k)
            at += k
        original = any(id(c) in gone for c in self._constraints)
        live = not original and (not rows or bool(self._solver.removable()[0][rows].all()))
        stuck = False
        if live and rows:
            try:
                self._solver.remove(rows=rows)
            except _ffi.DantzigAmdError as exc:      # (see solve(): a basis that cannot be carried on from)
                if not any(s in str(exc) for s in _NO_CARRY_ON):
                    raise
                live, stuck = False, True
        if live:
            self._extended -= sum(id(c) in gone for c in self._added[:self._extended])
            self._added = [c for c in self._added if id(c) not in gone]
        else:
            self.close()
            self._constraints = [c for c in self._constraints if id(c) not in gone]
            if stuck:       # (not a rebuild the removal itself asked for)
                self.restarts += 1
            else:
                self.rebuilds += 1
        for key in gone:
            self._rhs.pop(key, None)

    def _rows_of(self, constraint, form, order) -> list:
        """The rows of `constraint` over the structural columns of `form` (the standard form of this
        session's model, variables in `order`): [(coefficients by column, b)], one per inequality
        sum coef_u u <= b it lowers to, +coef on the column of u's x+ and -coef on that of its x-; a
        repeated variable keeps its last coefficient, as the builder's rows do."""
        slot = {v.id: i for i, v in enumerate(order)}
        new_b = self._rhs.get(id(constraint))
        out = []
        for ineq, sign in zip(constraint.rust_inequalities(), constraint._signs):
            row = np.zeros(form.n_struct)
            for coef, v in zip(ineq._linexpr.coefs, ineq._linexpr.vars):
                u = slot[v.id]
                row[form.var_col[form.pos_var[u]]] = coef
                row[form.var_col[form.neg_var[u]]] = -coef
            out.append((row, ineq._b if new_b is None else sign * new_b))
        return out

    def _change(self, objective, rhs) -> None:
        if objective is not None:
            self._objective = objective.to_affexpr()
        known = {id(c) for c in self._constraints + self._added}
        for constraint, b in (rhs or {}).items():
            if id(constraint) not in known:
                raise KeyError("the constraint is not part of the session's model")
            if not isinstance(b, (int, float)):
                raise TypeError("rhs maps a constraint to the number its normal form compares with")
            self._rhs[id(constraint)] = _normal_b(b)

    def solve(self, *, objective=None, rhs=None) -> Solution:
        """Solve the model with `objective` (a new expression in the problem's sense) and `rhs`
        ({constraint: new b}, b of the constraint's normal form linexpr <=, >= or == b: the number
        Solution.rhs_range speaks about) replacing what the session holds.  Raises
        exceptions.UnboundedError / InfeasibleError like Optimize.solve; the session stays usable.
        ValueError if the change alters more of the standard form than b, c and the constant (an
        objective over a variable the model had not seen)."""
        self._apply_removals()
        before = (self._objective, dict(self._rhs))
        self._change(objective, rhs)
        try:
            problem, arrays, order = self._lowered()
            self._check_lp(problem)
            form = rs.standard_form(arrays)
            if self._solver is not None and not (form.same_shape_as(self._form)
                                                 and [v.id for v in order] == [v.id for v in self._order]):
                raise ValueError("session: the new objective or right-hand side changes the standard form "
                                 "(only b and the objective's coefficients may change)")
            # the rows added to the live solver, below the form's: their b follows the form's
            added = [r for c in self._added for r in self._rows_of(c, form, order)]
            pending = [r for c in self._added[self._extended:] for r in self._rows_of(c, form, order)]
            b_all = np.concatenate([form.x, [b for _, b in added]])
            c_all = np.concatenate([form.c, np.zeros(len(added))])
        except Exception:
            self._objective, self._rhs = before
            raise
        if self._solver is None:
            lp = core.CoreLP(a=form.a, c=form.c, basis=form.basis, nonbasis=form.nonbasis, x=form.x,
                             z=form.z, var_col=form.var_col, constant=form.constant)
            self._solver = core.Solver(lp, **self._opts)
        else:
            try:
                if pending:
                    self._solver.extend(rows=np.array([row for row, _ in pending]), rhs=[b for _, b in pending])
                    self._extended = len(self._added)
                self._solver.reoptimize(b=b_all, c=c_all, constant=form.constant)
            except _ffi.DantzigAmdError as exc:
                # The basis the last solve ended on cannot be carried on from: a singular / panic end, or a
                # FAST run that counted near ties and ended on a basis that does not refactorise (two
                # parallel columns, such as the halves of a free variable, both basic).  The model is whole
                # on the host, so the session starts over from the slack basis instead of failing.
                if not any(s in str(exc) for s in _NO_CARRY_ON):
                    raise
                self.close()
                self.restarts += 1
                return self.solve()
        self._form, self._order = form, order
        self._solver.run(0)
        res = self._solver.result(log=False)
        self.pivots.append(res.iterations - self._iterations)
        self._iterations = res.iterations
        if res.status_code == _ffi.UNBOUNDED:
            raise UnboundedError("The objective is unbounded")
        if res.status_code == _ffi.INFEASIBLE:
            raise InfeasibleError("The model is infeasible")
        if res.status_code != _ffi.OPTIMAL:
            raise RuntimeError(f"simplex terminated with status {res.status!r} after {res.iterations} iterations")
        values = _user_values(res, form, order)
        return Solution(solution=rs.PySolution(res.objective, values, self.pivots[-1], res.numerics,
                                               (form.m + len(added), form.n + len(added))),
                        sense=self._problem.sense)

    def close(self) -> None:
        if self._solver is not None:
            self._solver.close()
            self._solver = None
            self._iterations = 0  # (a later solve() starts a new solver from the slack basis)
            self._constraints += self._added  # (... of the whole model)
            self._added, self._extended = [], 0
            gone = {id(c) for c in self._removed}
            self._constraints = [c for c in self._constraints if id(c) not in gone]
            for key in gone:   # (removals that were waiting for the next solve)
                self._rhs.pop(key, None)
            self._removed = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Minimize(Optimize):
    """min objective  s.t. constraints.

    >>> x = Variable(lb=1.0, ub=None); y = Variable(lb=None, ub=2.0)
    >>> result = Minimize(x - 5 * y).solve()      # result[x] == 1.0, result[y] == 2.0
    """

    sense = property(lambda self: "minimize")


class Maximize(Optimize):
    """max objective  s.t. constraints."""

    sense = property(lambda self: "maximize")


def solve_many(problems, *, duals: bool = False, ranging: bool = False, rays: bool = False,
               return_exceptions: bool = False, fast: bool = False) -> list:
    """[p.solve() for p in problems] in one batched call (rust.solve_many): the small models share
    one launch on the GPU, one workgroup per model, bit for bit what p.solve() returns.  A model
    that is unbounded or infeasible raises the exception p.solve() raises, with the model's index
    in the message, after the whole batch is done; with return_exceptions=True the exception
    instance stands in that model's place.  duals=True: every Solution is p.solve(duals=True)'s;
    ranging=True: p.solve(ranging=True)'s; rays=True: every exception is p.solve(rays=True)'s, `.ray`
    included.  fast=True: the shared batch runs FAST numerics and falls back to STRICT, model by
    model, where a decision of the pivot rule comes within rounding of a tie (rust.solve_many); not
    together with duals, ranging or rays (ValueError): sessions(problems, fast=True).solve(duals=True,
    ranging=True, rays=True) has them behind the FAST batch."""
    problems = list(problems)
    for i, p in enumerate(problems):
        if not isinstance(p, Optimize):
            raise TypeError(f"problems[{i}] is a {type(p).__name__}, not a Minimize / Maximize")
    if fast and (duals or ranging or rays):
        raise ValueError("fast=True does not combine with duals, ranging or rays yet")
    if rays and ranging:
        raise ValueError("rays=True and ranging=True: the ranging call carries no ray; ask in two calls")
    duals = duals or ranging
    raw = rs.solve_many([p._rust_problem() for p in problems], duals=duals,
                        ranging=[p._row_groups() for p in problems] if ranging else False,
                        rays=rays, return_exceptions=return_exceptions or rays, **({"fast": True} if fast else {}))
    if rays:  # (the core rays become the models' before anything is raised)
        raw = [p._wrap_ray(r) if isinstance(r, Exception) else r for p, r in zip(problems, raw)]
        if not return_exceptions:
            for r in raw:
                if isinstance(r, Exception):
                    raise r
    return [r if isinstance(r, Exception)
            else Solution(solution=r, sense=p.sense, constraints=list(p.constraints) if duals else None,
                          objective=p.objective if ranging else None)
            for p, r in zip(problems, raw)]


class _BatchModel:
    """One model of a SessionBatch: what it holds now and where its last solve ended."""
    __slots__ = ("problem", "objective", "rhs", "form", "order", "last", "arrays")


def sessions(problems, fast: bool = False, resident: bool = False, **core_opts) -> "SessionBatch":
    """A SessionBatch over `problems` (Minimize / Maximize models): the batched sibling of
    Optimize.session().  fast=True: the batch runs FAST numerics; resident=True: the batch stays on
    the GPU between calls (SessionBatch)."""
    return SessionBatch(problems, fast=fast, resident=resident, **core_opts)


class SessionBatch:
    """Many small models re-optimised together (dantzig_amd.sessions): the first solve() runs every
    model from its slack basis in one STRICT batch, one workgroup per model; every later
    solve(objectives=..., rhs=...) hands each model's last basis to the batch as its start
    (core.solve_batch(start=...)), so that a model whose data moved a little takes the few pivots
    from its last basis instead of all of them.  Changes accumulate, as in a Session.

    A model is started cold again when its last solve ended singular or panicked, or when its change
    alters more of the standard form than b, c and the constant.  The batch is stateless on the
    device: nothing stays there between calls, the matrices are uploaded again on every call; what
    is kept, on the host, is each model's last basis.  A re-optimised path is not the reference's
    path from the slack basis: the promise is the optimum (or the verdict), not the pivots, and at a
    degenerate optimum possibly another vertex.

    `pivots` holds one list per call with one count per model, `cold` the number of models each call
    started cold.  core_opts: fields of dzg_opts over rust.set_options()'s; numerics is STRICT (AUTO
    means STRICT here).  ValueError for a model that does not go through the STRICT batch: more than
    128 rows in standard form, or an integer variable.

    fast=True: every call is core.solve_batch_fast, the later ones with start=...: one workgroup per
    model keeps the explicit basis inverse in LDS.  numerics is then FAST or AUTO (the default: a
    model whose FAST solve comes within rounding of a tie, or ends singular, is solved by the STRICT
    batch in the same call, from the same start); `strict_fallbacks` holds, per call, the number of
    models whose result is STRICT's (a warm model often is one of them: the split pair x+ - x- of
    the lowering leaves a reduced cost at zero up to rounding).

    resident=True: the batch is a core.BatchSolver.  The first solve() puts
    every model's matrix on the GPU; a later call sends the right-hand sides, costs and constants
    that changed and nothing else, and returns what the stateless batch returns, bit for bit.  When a
    change alters a model's standard form beyond b, c and the constant the handle is built again
    from the new forms (`rebuilds` counts that) and the other models carry on from their last
    bases.  close(), or leaving the `with` block, frees the GPU memory; a later solve() starts over."""

    def __init__(self, problems, fast: bool = False, resident: bool = False, **core_opts) -> None:
        problems = list(problems)
        if not isinstance(resident, (bool, np.bool_)):
            raise TypeError(f"sessions: resident is True or False, not {resident!r}")
        for i, p in enumerate(problems):
            if not isinstance(p, Optimize):
                raise TypeError(f"problems[{i}] is a {type(p).__name__}, not a Minimize / Maximize")
        self._opts = {**rs._options, **core_opts}
        self._fast = bool(fast)
        if self._fast:
            if self._opts.get("numerics", core.AUTO) not in (core.FAST, core.AUTO):
                raise ValueError("sessions(fast=True): numerics is FAST or AUTO")
        elif self._opts.get("numerics", core.AUTO) not in (core.STRICT, core.AUTO):
            raise ValueError("sessions: the batch runs STRICT numerics only (numerics=STRICT or AUTO)")
        self._models = []
        for i, p in enumerate(problems):
            st = _BatchModel()
            st.problem, st.objective, st.rhs, st.last = p, p.objective, {}, None
            st.form, st.order, st.arrays = self._lower_full(i, p, st.objective, st.rhs)
            self._models.append(st)
        self.pivots: list = []
        self.cold: list = []
        self.strict_fallbacks: list = []
        self._resident = bool(resident)
        self._handle = None
        self.rebuilds = 0

    @staticmethod
    def _lower(i: int, p: "Optimize", objective, rhs: dict):
        return SessionBatch._lower_full(i, p, objective, rhs)[:2]

    @staticmethod
    def _lower_full(i: int, p: "Optimize", objective, rhs: dict):
        """(form, order, the lowered arrays dzg_model_map_duals / _ray read)."""
        problem, arrays, order = _lower_model(p.sense, objective, _model_rows(p.constraints, rhs))
        if rs._has_integer(*problem):
            raise ValueError(f"problems[{i}]: re-optimisation is not defined for a model with integer variables")
        form = rs.standard_form(arrays)
        if form.m > _ffi.BATCH_MAX_ROWS:
            raise ValueError(f"problems[{i}]: {form.m} rows in standard form; the batch takes at most "
                             f"{_ffi.BATCH_MAX_ROWS}")
        return form, order, arrays

    def __len__(self) -> int:
        return len(self._models)

    def _per_model(self, what, name: str) -> list:
        if what is None:
            return [None] * len(self._models)
        what = list(what)
        if len(what) != len(self._models):
            raise ValueError(f"{name}: {len(what)} entries for {len(self._models)} models (None = unchanged)")
        return what

    @staticmethod
    def _core_request(problem, form, order):
        """Model i's ranging request in terms of its standard form: one cost direction per user
        variable (+1 on x+, -1 on x-), one right-hand-side direction per constraint (_row_groups)."""
        cost = []
        for u in range(len(order)):
            d = {}
            if form.pos_var[u] >= 0:
                d[int(form.pos_var[u])] = 1.0
            if form.neg_var[u] >= 0:
                d[int(form.neg_var[u])] = -1.0
            cost.append(d)
        return cost, [{int(r): float(k) for r, k in g} for g in problem._row_groups()]

    @staticmethod
    def _model_duals(res, arrays, form, order):
        """rs.PyDuals / rs.PyRanging of a core result, as solve_many maps them (dzg_model_map_duals)."""
        du = res.duals
        if du is None:
            return None, None
        md, buf, cm = _ffi.ModelDuals(), rs._DualBuffers(arrays), rs._c_model(arrays)
        buf.fill(md)
        y = _ffi.f64(du.y)
        _ffi.check(_ffi.lib().dzg_model_map_duals(C.byref(cm), _ffi.ptr(y), C.c_int64(form.m), C.byref(md)),
                   "dzg_model_map_duals")
        md.core.source, md.core.primal_obj, md.core.dual_obj = du.source_code, du.primal_obj, du.dual_obj
        md.core.primal_infeas, md.core.dual_infeas, md.core.z_diff = du.primal_infeas, du.dual_infeas, du.z_diff
        rg = res.ranging
        if rg is None:
            return buf.pyduals(md, order), None
        by_id = lambda a, cast: {v.id: cast(a[i]) for i, v in enumerate(order)}  # noqa: E731
        return buf.pyduals(md, order), rs.PyRanging(
            var_lo=by_id(rg.cost_lo, float), var_hi=by_id(rg.cost_hi, float), var_lo_var=by_id(rg.cost_lo_var, int),
            var_hi_var=by_id(rg.cost_hi_var, int), group_lo=[float(v) for v in rg.rhs_lo],
            group_hi=[float(v) for v in rg.rhs_hi], group_lo_var=[int(v) for v in rg.rhs_lo_var],
            group_hi_var=[int(v) for v in rg.rhs_hi_var])

    @staticmethod
    def _model_ray(res, arrays, form, order):
        """rs.PyRay of a core result's ray (dzg_model_map_ray), None without one."""
        ray = res.ray
        if ray is None:
            return None
        mr, buf, cm = _ffi.ModelRay(), rs._RayBuffers(arrays), rs._c_model(arrays)
        buf.fill(mr)
        d, y = _ffi.f64(ray.d), _ffi.f64(ray.y)
        _ffi.check(_ffi.lib().dzg_model_map_ray(C.byref(cm), C.c_int32(ray.kind_code), _ffi.ptr(d), _ffi.ptr(y),
                                                C.c_int64(form.m), C.c_int64(form.n), C.byref(mr)),
                   "dzg_model_map_ray")
        mr.core.kind, mr.core.proven, mr.core.value = ray.kind_code, int(ray.proven), ray.value
        mr.core.violation, mr.core.mu = ray.violation, ray.mu
        return buf.pyray(mr, order)

    def solve(self, objectives=None, rhs=None, return_exceptions: bool = False, duals: bool = False,
              ranging: bool = False, rays: bool = False) -> list:
        """duals=True: every Solution answers dual(), reduced_cost() and certificate; ranging=True (implies
        duals): also rhs_range() and objective_range(); rays=True: the UnboundedError / InfeasibleError of
        a model carries `.ray` -- each as solve_many maps them, computed behind the batch from the state
        the model ended in (core.solve_batch_fast / core.BatchSolver.solve with the same keywords; a
        STRICT session goes through solve_batch_fast(numerics=STRICT, start=...)).  All three compose,
        with each other and with a warm start.

        Solve every model with objectives[i] (a new expression in model i's sense) and rhs[i]
        ({constraint: new b}, as Session.solve takes it) replacing what the batch holds for it; None,
        for one model or for the whole argument, means unchanged.  Returns one Solution per model,
        values mapped as Session.solve maps them.  A model that ends unbounded or infeasible raises
        UnboundedError / InfeasibleError with its index in the message once the whole batch is done;
        with return_exceptions=True the exception stands in that model's place.  Either way the batch
        stays usable.  KeyError / TypeError / ValueError for a bad change: nothing is changed then."""
        objectives, rhs = self._per_model(objectives, "objectives"), self._per_model(rhs, "rhs")
        staged = []
        for i, st in enumerate(self._models):
            objective = st.objective if objectives[i] is None else objectives[i].to_affexpr()
            new_rhs = dict(st.rhs)
            known = {id(c) for c in st.problem.constraints}
            for constraint, b in (rhs[i] or {}).items():
                if id(constraint) not in known:
                    raise KeyError(f"rhs[{i}]: the constraint is not part of the model")
                if not isinstance(b, (int, float)):
                    raise TypeError("rhs maps a constraint to the number its normal form compares with")
                new_rhs[id(constraint)] = _normal_b(b)
            form, order, arrays = self._lower_full(i, st.problem, objective, new_rhs)
            warm = (st.last is not None and st.last.status not in ("singular", "panic")
                    and form.same_shape_as(st.form) and [v.id for v in order] == [v.id for v in st.order])
            staged.append((objective, new_rhs, form, order, warm, arrays))
        lps = [core.CoreLP(a=f.a, c=f.c, basis=f.basis, nonbasis=f.nonbasis, x=f.x, z=f.z, var_col=f.var_col,
                           constant=f.constant) for _, _, f, _, _, _ in staged]
        start = [st.last if warm else None for st, (_, _, _, _, warm, _) in zip(self._models, staged)]
        duals = bool(duals or ranging)
        post = {}
        if duals or rays:
            post = dict(duals=duals, rays=bool(rays))
            if ranging:
                post["ranging"] = [self._core_request(st.problem, f, o)
                                   for st, (_, _, f, o, _, _) in zip(self._models, staged)]
        if self._resident:
            results = self._solve_resident(lps, [f for _, _, f, _, _, _ in staged], start, post)
        else:
            opts = dict(self._opts)
            solve = core.solve_batch_fast if self._fast or post else core.solve_batch
            if post and not self._fast:
                opts["numerics"] = core.STRICT
            results = solve(lps, log=False, start=start if any(s is not None for s in start) else None, **post, **opts)
        out = []
        for i, (st, (objective, new_rhs, form, order, _, arrays), res) in enumerate(zip(self._models, staged, results)):
            st.objective, st.rhs, st.form, st.order, st.last, st.arrays = objective, new_rhs, form, order, res, arrays
            if res.status_code in (_ffi.UNBOUNDED, _ffi.INFEASIBLE):
                exc = (UnboundedError(f"The objective is unbounded (model {i})") if res.status_code == _ffi.UNBOUNDED
                       else InfeasibleError(f"The model is infeasible (model {i})"))
                if rays:
                    exc.ray = self._model_ray(res, arrays, form, order)
                    exc = st.problem._wrap_ray(exc)
                out.append(exc)
            elif res.status_code != _ffi.OPTIMAL:
                out.append(RuntimeError(f"simplex terminated with status {res.status!r} after "
                                        f"{res.iterations} iterations (model {i})"))
            else:
                sol = rs.PySolution(res.objective, _user_values(res, form, order), res.iterations, res.numerics,
                                    (form.m, form.n))
                if duals:
                    sol.duals, sol.ranging = self._model_duals(res, arrays, form, order)
                out.append(Solution(solution=sol, sense=st.problem.sense,
                                    constraints=list(st.problem.constraints) if duals else None,
                                    objective=objective if ranging else None))
        self.pivots.append([r.iterations for r in results])
        self.cold.append(sum(s is None for s in start))
        if self._fast:
            self.strict_fallbacks.append(sum(r.numerics == "strict" for r in results))
        if not return_exceptions:
            for o in out:
                if isinstance(o, Exception):
                    raise o
        return out

    def _solve_resident(self, lps, forms, start, post=None) -> list:
        """This call on the resident handle: start[i] is what the stateless call would hand model i
        (None: cold).  The handle is built from `lps` when there is none or when a model's standard
        form no longer fits the one it holds; otherwise only what moved is sent."""
        fits = self._handle is not None and all(
            f.same_shape_as(st.form) and np.array_equal(f.basis, st.form.basis)
            and np.array_equal(f.nonbasis, st.form.nonbasis) for f, st in zip(forms, self._models))
        if not fits:
            if self._handle is not None:
                self.close()
                self.rebuilds += 1
            opts = dict(self._opts)
            if not self._fast:
                opts["numerics"] = core.STRICT
            self._handle = core.BatchSolver(lps, log_cap=0, **opts)
            for i, s in enumerate(start):
                if s is not None:
                    self._handle.set_start(i, s)
            return self._handle.solve(log=False, **(post or {}))
        changes = []
        for i, (f, st) in enumerate(zip(forms, self._models)):
            old = st.form
            b = None
            if f.x.tobytes() != old.x.tobytes():
                b = np.empty(f.m)
                b[-1 - f.var_col[f.basis]] = f.x      # by constraint row
            c = f.c if f.c.tobytes() != old.c.tobytes() else None
            same_constant = np.float64(f.constant).tobytes() == np.float64(old.constant).tobytes()
            constant = None if same_constant else float(f.constant)
            if b is not None or c is not None or constant is not None:
                changes.append((i, b, c, constant))
            if start[i] is None:
                self._handle.set_start(i, None)
        if changes:
            self._handle.update_many(changes)
        return self._handle.solve(log=False, **(post or {}))

    def close(self) -> None:
        """Frees the resident handle (resident=True); the models' last bases stay on the host, so the
        next solve() builds a new handle and carries on from them."""
        if self._handle is not None:
            self._handle.close()
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
