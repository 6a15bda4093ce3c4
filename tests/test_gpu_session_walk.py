"""Sessions walked through random solve / add_constraints / remove_constraints / close sequences
(tests/session_walk.py; tests/test_session_walk_host.py checks the walks on the CPU).

After every solve() the reference is the CPU oracle, cold, on the model as rewritten so far
(ora.solve_model, not problem.solve()): the same verdict, raised as InfeasibleError / UnboundedError with
the session usable afterwards; the objective to 1e-9; the returned values inside every constraint and
bound of the model to 1e-9 (values are not compared: a re-optimised path may end on another vertex of a
degenerate optimum).  Session.pivots counts the solves, the live solver holds the form's rows plus the
rows of the constraints added since, and `rebuilds` rises exactly when a removed constraint was one of
the session's original model or one of its rows was binding at the handle's basis (the row masks,
mirrored on the host by remove_check.free_masks)."""
import numpy as np
import pytest

from dantzig_amd import core
from dantzig_amd.exceptions import InfeasibleError, UnboundedError
from tests import remove_check as rmc
from tests import session_walk as sw
from tests.test_surface import build_problem

pytestmark = pytest.mark.gpu

TOL = 1e-9
RAISES = {"infeasible": InfeasibleError, "unbounded": UnboundedError}


def _free_rows(session):
    solver = session._solver
    return rmc.free_masks(rmc.at_basis(solver._lp, solver.result(log=False)))[0]


def _walk(seed, numerics, script=None):
    model, steps = sw.recipe(seed) if script is None else script
    ns, problem = build_problem(sw.python_form(model))
    env = dict(ns)
    variables = [ns[f"v{j}"] for j in range(len(model["vars"]))]
    cons = {c["id"]: pc for c, pc in zip(model["constraints"], problem.constraints)}
    assert len(cons) == len(problem.constraints)
    shape = {c["id"]: sw.rows_of(c) for c in model["constraints"]}
    live, rebuilds, restarts, live_removals, verdicts = [], 0, 0, 0, []
    with problem.session(numerics=numerics) as session:
        for k, step in enumerate(steps):
            what = f"seed {seed} step {k} {step['kind']}"
            change, leaving = {}, []
            for action, arg in step["actions"]:
                if action == "objective":
                    change["objective"] = eval(sw._expr(*arg), {"__builtins__": {}}, env)
                elif action == "rhs":
                    change["rhs"] = {cons[i]: b for i, b in arg.items()}
                elif action == "add":
                    for con in arg:
                        if con["id"] not in cons:
                            cons[con["id"]] = eval(sw.constraint_text(con), {"__builtins__": {}}, env)
                            shape[con["id"]] = sw.rows_of(con)
                    session.add_constraints([cons[con["id"]] for con in arg])
                    for con in arg:
                        if con["id"] in leaving:
                            leaving.remove(con["id"])          # still on the solver: the removal is called off
                        elif session._solver is not None:
                            live.append(con["id"])
                elif action == "remove":
                    session.remove_constraints([cons[i] for i in arg])
                    if session._solver is not None:
                        leaving += arg
                elif action == "close":
                    session.close()
                    live = []
            if leaving:         # what the next solve() must do about them, from the handle's own basis
                rows, at = [], session._form.m
                for i in live:
                    if i in leaving:
                        rows += range(at, at + shape[i])
                    at += shape[i]
                original = any(i not in live for i in leaving)
                if original or not _free_rows(session)[rows].all():
                    rebuilds += 1
                    live = []
                else:
                    live_removals += 1
                    live = [i for i in live if i not in leaving]
            model = sw.rewrite(model, step)
            status, objective, _ = sw.reference(model)
            verdicts.append(status)
            if status in RAISES:
                with pytest.raises(RAISES[status]):
                    session.solve(**change)
            else:
                assert status == "optimal", (what, status)
                sol = session.solve(**change)
                assert abs(sol.objective_value - objective) <= TOL * max(1.0, abs(objective)), \
                    (what, sol.objective_value, objective)
                miss = sw.violation(model, [sol[v] for v in variables])
                assert miss <= TOL, (what, miss)
            if session.restarts > restarts:        # the last basis could not be carried on from: a cold start
                print(f"{what}: the session started over from the slack basis")
                restarts, live = session.restarts, []
            assert len(session.pivots) == k + 1 and all(p >= 0 for p in session.pivots), what
            assert session.rebuilds == rebuilds, (what, session.rebuilds, rebuilds)
            assert session._solver.dims()[0] == session._form.m + sum(shape[i] for i in live), (what, live)
        print(f"seed {seed}: pivots per solve {session.pivots}, {rebuilds} rebuilds, {live_removals} live removals, "
              f"{restarts} restarts")
    return rebuilds, live_removals, restarts, verdicts


@pytest.mark.parametrize("numerics", [core.AUTO, core.FAST], ids=["auto", "fast"])
@pytest.mark.parametrize("seed", sw.SEEDS)
def test_session_follows_the_oracle_on_the_model_as_rewritten(seed, numerics):
    rebuilds, live_removals, restarts, verdicts = _walk(seed, numerics)
    assert rebuilds >= 1 and live_removals >= 1, (rebuilds, live_removals)
    assert {"infeasible", "unbounded", "optimal"} <= set(verdicts)
    assert restarts == 0 or numerics == core.FAST, "a STRICT handle's basis can always be carried on from"


# The shortest walk that showed it: a box constraint of the free variable v3 goes and the objective pushes that
# way and nowhere else.  (Seed 3 of an earlier recipe; the recipe now pushes on top of the objective it finds.)
STUCK = dict(
    vars=[(None, 1.5), (-1.5, 2.0), (0.0, None), (None, None), (-1.5, 2.5), (-0.0, 1.0)], sense="min",
    objective=([3.0, -1.0, -3.0, -1.0, -3.0, 3.0], 1.0),
    constraints=[dict(id=0, coefs=[1.0, 0.0, 0.0, 0.0, 0.0, 0.0], op=">=", b=-1.75),
                 dict(id=1, coefs=[0.0, 0.0, 1.0, 0.0, 0.0, 0.0], op="<=", b=2.5),
                 dict(id=2, coefs=[0.0, 0.0, 0.0, 1.0, 0.0, 0.0], op="<=", b=1.25),
                 dict(id=3, coefs=[0.0, 0.0, 0.0, 1.0, 0.0, 0.0], op=">=", b=-3.5),
                 dict(id=4, coefs=[-2.0, 2.0, 2.0, 3.0, 2.0, -2.0], op="<=", b=-2.0),
                 dict(id=5, coefs=[1.0, 1.0, 3.0, -1.0, 3.0, -3.0], op=">=", b=3.75)])
STUCK_STEPS = [dict(kind="solve", actions=[]),
               dict(kind="objective", actions=[("objective", ([3.0, 1.0, 1.0, -2.0, -1.0, 0.0], 1.0))]),
               dict(kind="unbounded", actions=[("remove", [3]), ("objective", ([0.0, 0.0, 0.0, 1.0, 0.0, 0.0], 0.0))]),
               dict(kind="back_unbounded", actions=[("add", [STUCK["constraints"][3]])])]


def test_fast_session_stays_usable_after_an_unbounded_end_on_a_free_variable():
    """FAST counts near ties between the two halves of v3 -- parallel columns -- and ended `unbounded` on a
    basis that held both; the step back (the constraint added again) then failed in dzg_solver_extend with
    "the new basis did not refactorise (singular block)" instead of solving.  The session now starts over
    from the slack basis where the live basis cannot be carried on from (Session.restarts)."""
    *_, restarts, verdicts = _walk(0, core.FAST, script=(STUCK, STUCK_STEPS))
    assert verdicts == ["optimal", "optimal", "unbounded", "optimal"]
    print(f"restarts: {restarts}")
