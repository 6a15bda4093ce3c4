"""Minimize / Maximize / Solution (python-source/dantzig/optimize.py:8-154).

The core always maximises: Minimize negates the objective on the way in and the optimal value
on the way out (optimize.py:114-117, :21-27).  A model with an integer variable is solved by
branch and bound (rust.solve_mip); Solution.mip then reports the search in the user's sense."""
from __future__ import annotations

import abc
from typing import Union

from . import rust as rs
from .model import AffExpr, Constraint, LinExpr, Variable

_SENSES = ("minimize", "maximize")


class Solution:
    def __init__(self, *, solution: rs.PySolution, sense: str) -> None:
        if sense not in _SENSES:
            raise ValueError(f"sense is {sense!r}; a Solution is built for {_SENSES[0]!r} or {_SENSES[1]!r}")
        self._solution = solution
        self._sense = sense

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

    def solve(self) -> Solution:
        """Solve on the GPU.  Raises exceptions.UnboundedError / InfeasibleError."""
        objective, constraints = self._rust_problem()
        if rs._has_integer(objective, constraints):
            return Solution(solution=rs.solve_mip(objective, constraints), sense=self.sense)
        return Solution(solution=rs.solve(objective, constraints), sense=self.sense)


class Minimize(Optimize):
    """min objective  s.t. constraints.

    >>> x = Variable(lb=1.0, ub=None); y = Variable(lb=None, ub=2.0)
    >>> result = Minimize(x - 5 * y).solve()      # result[x] == 1.0, result[y] == 2.0
    """

    sense = property(lambda self: "minimize")


class Maximize(Optimize):
    """max objective  s.t. constraints."""

    sense = property(lambda self: "maximize")


def solve_many(problems, *, return_exceptions: bool = False) -> list:
    """[p.solve() for p in problems] in one batched call (rust.solve_many): the small models share
    one launch on the GPU, one workgroup per model, bit for bit what p.solve() returns.  A model
    that is unbounded or infeasible raises the exception p.solve() raises, with the model's index
    in the message, after the whole batch is done; with return_exceptions=True the exception
    instance stands in that model's place."""
    problems = list(problems)
    for i, p in enumerate(problems):
        if not isinstance(p, Optimize):
            raise TypeError(f"problems[{i}] is a {type(p).__name__}, not a Minimize / Maximize")
    raw = rs.solve_many([p._rust_problem() for p in problems], return_exceptions=return_exceptions)
    return [r if isinstance(r, Exception) else Solution(solution=r, sense=p.sense)
            for p, r in zip(problems, raw)]
