"""The reference of the session walks alone, on the CPU (tests/session_walk.py): every step kind occurs,
the planted verdicts occur, the removals are the ones their names promise according to the oracle's
optimum, and HiGHS agrees with the CPU oracle's verdict and objective after every step."""
import functools

import numpy as np
import pytest
from scipy.optimize import linprog

from tests import session_walk as sw

HIGHS_VERDICT = {0: "optimal", 2: "infeasible", 3: "unbounded"}


def highs(model):
    sign = -1.0 if model["sense"] == "max" else 1.0
    coefs, constant = model["objective"]
    ub = [(c["coefs"] if c["op"] == "<=" else (-np.array(c["coefs"])).tolist(), c["b"] if c["op"] == "<=" else -c["b"])
          for c in model["constraints"] if c["op"] != "=="]
    eq = [(c["coefs"], c["b"]) for c in model["constraints"] if c["op"] == "=="]
    r = linprog(sign * np.array(coefs), A_ub=[a for a, _ in ub] or None, b_ub=[b for _, b in ub] or None,
                A_eq=[a for a, _ in eq] or None, b_eq=[b for _, b in eq] or None, bounds=model["vars"], method="highs")
    return r.status, (sign * float(r.fun) + constant if r.status == 0 else None)


@functools.lru_cache(maxsize=None)
def _survey(seed):
    model, steps = sw.recipe(seed)
    out, xs = [], None
    for step in steps:
        before, model = model, sw.rewrite(model, step)
        status, objective, values = sw.reference(model)
        out.append(dict(kind=step["kind"], status=status, objective=objective, model=model, before=before, xs=xs,
                        actions=step["actions"]))
        if status == "optimal":
            assert sw.violation(model, values) <= 1e-9, (seed, step["kind"])
            xs = values
    return out


def test_every_step_kind_occurs():
    kinds = {s["kind"] for seed in sw.SEEDS for s in _survey(seed)}
    assert kinds == set(sw.KINDS), set(sw.KINDS) - kinds
    assert len(sw.SEEDS) == 3 and all(len(_survey(seed)) == sw.STEPS == 20 for seed in sw.SEEDS)


def test_the_models_mix_bounds_operators_and_senses():
    starts = [sw.recipe(seed)[0] for seed in sw.SEEDS]
    assert all(3 <= len(m["vars"]) <= 6 for m in starts)
    bounds = {(lb is None, ub is None) for m in starts for lb, ub in m["vars"]}
    assert bounds == {(False, True), (True, True), (False, False), (True, False)}
    ops = {c["op"] for seed in sw.SEEDS for s in _survey(seed) for c in s["model"]["constraints"]}
    assert ops == {"<=", ">=", "=="} and {m["sense"] for m in starts} == {"max", "min"}


def test_the_planted_verdicts_and_the_steps_back_occur():
    for seed in sw.SEEDS:
        steps = _survey(seed)
        assert all(s["status"] != "panic" for s in steps), seed
        for k, s in enumerate(steps):
            if s["kind"] in ("infeasible", "unbounded"):
                assert s["status"] == s["kind"], (seed, k, s["status"])
                assert steps[k + 1]["kind"] == "back_" + s["kind"] and steps[k + 1]["status"] == "optimal", (seed, k)
    verdicts = {s["status"] for seed in sw.SEEDS for s in _survey(seed)}
    assert {"optimal", "infeasible", "unbounded"} <= verdicts


def test_the_removals_are_what_their_names_promise():
    """At the oracle's optimum before the step: a slack removal leaves >= 0.1 of room, a binding one none."""
    counts = {"remove_added_slack": 0, "remove_added_binding": 0, "remove_original": 0}
    for seed in sw.SEEDS:
        for s in _survey(seed):
            if s["kind"] not in counts:
                continue
            (_, ids), = s["actions"]
            con = next(c for c in s["before"]["constraints"] if c["id"] == ids[0])
            room = sw.slack_of(con, s["xs"])
            if s["kind"] == "remove_added_slack":
                assert room >= 0.1, (seed, room)
            if s["kind"] == "remove_added_binding":
                assert abs(room) <= 1e-9, (seed, room)
            counts[s["kind"]] += 1
    assert all(v >= 1 for v in counts.values()), counts


@pytest.mark.parametrize("seed", sw.SEEDS)
def test_highs_agrees_with_the_oracle_after_every_step(seed):
    for k, s in enumerate(_survey(seed)):
        status, objective = highs(s["model"])
        assert HIGHS_VERDICT.get(status) == s["status"], (seed, k, s["kind"], s["status"], status)
        if s["status"] == "optimal":
            assert abs(objective - s["objective"]) <= 1e-6 * max(1.0, abs(objective)), (seed, k, s["kind"])


def test_the_written_forms_say_the_same():
    """python_form through the modelling surface's lowering is oracle_form, as the oracle solves them."""
    from tests.test_surface import build_problem, oracle_model
    from oracle import oracle as ora

    for seed in sw.SEEDS:
        for s in _survey(seed)[::5]:
            _, problem = build_problem(sw.python_form(s["model"]))
            lowered = ora.solve_model(oracle_model(problem)[0])
            assert lowered.status == s["status"], seed
            if s["status"] == "optimal":
                sign = -1.0 if s["model"]["sense"] == "min" else 1.0
                assert abs(sign * lowered.objective - s["objective"]) <= 1e-9 * max(1.0, abs(s["objective"])), seed
