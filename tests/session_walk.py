"""Random walks of a Session over a small model (tests/test_session_walk_host.py,
tests/test_gpu_session_walk.py).

The model is kept as numbers -- `vars` [(lb, ub)], `sense`, `objective` (coefs, constant) and
`constraints` [{id, coefs, op, b}] -- and written out in the two forms of
tests/golden/reference_kats.json: `python_form` (names and expression strings, what
tests.test_surface.build_problem reads) and `oracle_form` (the core-sense dict ora.solve_model reads:
maximised, rows coef . x <= b, an == as two rows).  A step is a list of actions on the session followed
by ONE solve(); `rewrite` applies the same actions to the model, so that after every solve the reference
is the CPU oracle, cold, on the model as rewritten so far.

Every variable is boxed by its bounds or by single-variable constraints around a point x0 that every
generated constraint keeps feasible, so the model is solvable unless a step plants the opposite: a
constraint above a variable's upper bound (infeasible) or a box constraint removed with the objective
pushing that way (unbounded); the step after undoes it.
"""
from __future__ import annotations

import copy

import numpy as np

from oracle import oracle as ora

KINDS = ("solve", "objective", "rhs", "rhs_added", "add_cut", "add_slack", "add_two", "remove_added_slack",
         "remove_added_binding", "remove_original", "remove_then_add", "close", "infeasible", "back_infeasible",
         "unbounded", "back_unbounded")
SEEDS = (3, 5, 26)
STEPS = 20


# ---------------------------------------------------------------------- the two written forms
def _expr(coefs, constant=None) -> str:
    """A constraint's linear part, or with `constant` an objective.  An objective names every variable, the
    zeros included: the lowering orders variables by first appearance, and a session re-optimises only
    over an unchanged order."""
    terms = [f"{float(c)!r} * v{j}" for j, c in enumerate(coefs) if c != 0.0 or constant is not None]
    if constant is not None:
        terms.append(repr(float(constant)))
    return " + ".join(terms)


def constraint_text(con) -> str:
    return f"{_expr(con['coefs'])} {con['op']} {float(con['b'])!r}"


def python_form(model) -> dict:
    spec = {}
    for j, (lb, ub) in enumerate(model["vars"]):
        spec[f"v{j}"] = "nonneg" if (lb, ub) == (0.0, None) else "free" if (lb, ub) == (None, None) else [lb, ub]
    return dict(vars=spec, sense=model["sense"], objective=_expr(*model["objective"]),
                constraints=[constraint_text(c) for c in model["constraints"]])


def oracle_form(model) -> dict:
    sign = -1.0 if model["sense"] == "min" else 1.0
    coefs, constant = model["objective"]
    rows = []
    for con in model["constraints"]:
        for s in {"<=": (1.0,), ">=": (-1.0,), "==": (1.0, -1.0)}[con["op"]]:
            rows.append({"terms": [[j, s * c] for j, c in enumerate(con["coefs"]) if c != 0.0], "b": s * con["b"]})
    return {"vars": [{"lb": lb, "ub": ub} for lb, ub in model["vars"]],
            "objective": {"terms": [[j, sign * c] for j, c in enumerate(coefs) if c != 0.0], "constant": sign * constant},
            "constraints": rows}


def reference(model):
    """(status, objective in the model's sense, values by variable) of the CPU oracle, cold."""
    res = ora.solve_model(oracle_form(model))
    sign = -1.0 if model["sense"] == "min" else 1.0
    return res.status, sign * res.objective, res.values


def rows_of(con) -> int:
    return 2 if con["op"] == "==" else 1


def slack_of(con, x) -> float:
    lhs = float(np.dot(con["coefs"], x))
    return {"<=": con["b"] - lhs, ">=": lhs - con["b"], "==": -abs(lhs - con["b"])}[con["op"]]


def violation(model, x) -> float:
    """The largest amount by which x misses a constraint or a bound of the model."""
    worst = max([0.0] + [-slack_of(con, x) for con in model["constraints"]])
    for (lb, ub), v in zip(model["vars"], x):
        worst = max(worst, 0.0 if lb is None else lb - v, 0.0 if ub is None else v - ub)
    return worst


def rewrite(model, step) -> dict:
    """The model after the step's actions."""
    model = copy.deepcopy(model)
    for action, arg in step["actions"]:
        if action == "objective":
            model["objective"] = arg
        elif action == "rhs":
            for con in model["constraints"]:
                if con["id"] in arg:
                    con["b"] = arg[con["id"]]
        elif action == "add":
            model["constraints"] += copy.deepcopy(arg)
        elif action == "remove":
            model["constraints"] = [c for c in model["constraints"] if c["id"] not in arg]
    return model


# ---------------------------------------------------------------------- the recipe
def _base(rng):
    nv = int(rng.integers(3, 7))
    kinds = ["boxed", "free", "nonneg", "upper"] + list(rng.choice(["boxed", "free", "nonneg", "upper"], 2))
    kinds = [kinds[i] for i in rng.permutation(nv)] if nv >= 4 else ["boxed", "free", "nonneg"]
    variables, x0, cons = [], [], []
    for kind in kinds:
        if kind == "nonneg":
            variables.append((0.0, None)); x0.append(float(rng.integers(2, 9)) / 4)
        elif kind == "free":
            variables.append((None, None)); x0.append(float(rng.integers(-8, 9)) / 4)
        elif kind == "boxed":
            lb, ub = -float(rng.integers(0, 5)) / 2, float(rng.integers(2, 7)) / 2
            variables.append((lb, ub)); x0.append((lb + ub) / 2)
        else:
            ub = float(rng.integers(2, 7)) / 2
            variables.append((None, ub)); x0.append(ub - float(rng.integers(2, 9)) / 4)
    x0 = np.array(x0)
    for j, (lb, ub) in enumerate(variables):          # the box: what the bounds leave open
        unit = np.zeros(nv); unit[j] = 1.0
        if ub is None:
            cons.append(dict(coefs=unit.tolist(), op="<=", b=float(x0[j] + rng.integers(4, 13) / 4), box=(j, "up")))
        if lb is None:
            cons.append(dict(coefs=unit.tolist(), op=">=", b=float(x0[j] - rng.integers(4, 13) / 4), box=(j, "down")))
    for k in range(int(rng.integers(2, 4))):
        cons.append(_row(rng, x0, "==" if k == 0 and rng.random() < 0.5 else ("<=", ">=")[int(rng.integers(0, 2))]))
    for k, con in enumerate(cons):
        con["id"] = k
    model = dict(vars=variables, sense=("max", "min")[int(rng.integers(0, 2))], objective=_objective(rng, nv),
                 constraints=cons)
    return model, x0


def _objective(rng, nv):
    coefs = rng.integers(-3, 4, nv).astype(float)
    if not coefs.any():
        coefs[0] = 1.0
    return coefs.tolist(), float(rng.integers(-2, 3))


def _row(rng, x0, op, slack=None):
    """A constraint through x0 (==) or with x0 inside by `slack` (default 0.5 .. 2)."""
    coefs = rng.integers(-3, 4, len(x0)).astype(float)
    if np.count_nonzero(coefs) < 2:
        coefs[:2] = (1.0, -2.0)
    slack = float(rng.integers(2, 9)) / 4 if slack is None else slack
    at = float(coefs @ x0)
    return dict(coefs=coefs.tolist(), op=op, b={"<=": at + slack, ">=": at - slack, "==": at}[op])


def _cut(rng, x0, xs):
    """A constraint that x0 satisfies and the optimum xs misses, or None if they are too close."""
    for _ in range(20):
        coefs = np.round(2 * (xs - x0) + rng.uniform(-1, 1, len(x0)), 1)
        gap = float(coefs @ (xs - x0))
        if gap >= 0.3:
            b = float(coefs @ x0) + float(rng.uniform(0.2, 0.8)) * gap
            if rng.random() < 0.5:
                return dict(coefs=coefs.tolist(), op="<=", b=b)
            return dict(coefs=(-coefs).tolist(), op=">=", b=-b)
    return None


def recipe(seed: int, steps: int = STEPS):
    """(the model before the first solve, the steps): each step {kind, actions}."""
    rng = np.random.default_rng(seed)
    model, x0 = _base(rng)
    start = copy.deepcopy(model)
    nv = len(x0)
    next_id = len(model["constraints"])
    added = []                       # ids added since the walk began (some may be original to the session by now)
    todo = [k for k in KINDS if k not in ("solve", "back_infeasible", "back_unbounded", "add_slack")]
    todo = [todo[i] for i in rng.permutation(len(todo))]
    out, pending_back = [], None
    status, _, xs = reference(model)
    assert status == "optimal", (seed, status)

    def by_id(k):
        return next(c for c in model["constraints"] if c["id"] == k)

    def new(con):
        nonlocal next_id
        con = dict(con, id=next_id)
        next_id += 1
        added.append(con["id"])
        return con

    def draw(kind):
        nonlocal pending_back
        live = [k for k in added if any(c["id"] == k for c in model["constraints"])]
        if kind == "objective":
            return [("objective", _objective(rng, nv))]
        if kind in ("rhs", "rhs_added"):
            pool = [c for c in model["constraints"] if c["op"] != "==" and (c["id"] in live) == (kind == "rhs_added")]
            if not pool:
                return None
            con = pool[int(rng.integers(0, len(pool)))]
            at = float(np.dot(con["coefs"], x0))
            slack = float(rng.integers(1, 9)) / 4
            return [("rhs", {con["id"]: at + slack if con["op"] == "<=" else at - slack})]
        if kind == "add_cut":
            con = _cut(rng, x0, xs)
            return None if con is None else [("add", [new(con)])]
        if kind == "add_slack":
            con = _row(rng, x0, "<=", slack=0.0)
            con["b"] = max(con["b"], float(np.dot(con["coefs"], xs))) + 1.0
            return [("add", [new(con)])]
        if kind == "add_two":
            second = _cut(rng, x0, xs) or _row(rng, x0, ">=")
            return [("add", [new(_row(rng, x0, "==")), new(second)])]
        if kind in ("remove_added_slack", "remove_added_binding"):
            want_slack = kind == "remove_added_slack"
            pool = [k for k in live if by_id(k)["op"] != "==" and
                    (slack_of(by_id(k), xs) >= 0.1 if want_slack else abs(slack_of(by_id(k), xs)) <= 1e-9)]
            return [("remove", [pool[int(rng.integers(0, len(pool)))]])] if pool else None
        if kind == "remove_original":
            pool = [c["id"] for c in model["constraints"] if c["id"] not in added and "box" not in c]
            return [("remove", [pool[int(rng.integers(0, len(pool)))]])] if pool else None
        if kind == "remove_then_add":
            if not live:
                return None
            con = by_id(live[int(rng.integers(0, len(live)))])
            return [("remove", [con["id"]]), ("add", [copy.deepcopy(con)])]
        if kind == "close":
            return [("close", None)]
        if kind == "infeasible":
            j = next(j for j, (lb, ub) in enumerate(model["vars"]) if ub is not None)
            unit = np.zeros(nv); unit[j] = 1.0
            con = new(dict(coefs=unit.tolist(), op=">=", b=model["vars"][j][1] + 1.0))
            pending_back = ("back_infeasible", con)
            return [("add", [con])]
        if kind == "unbounded":
            sign = 1.0 if model["sense"] == "max" else -1.0
            for con in model["constraints"]:
                if "box" not in con:
                    continue
                j, side = con["box"]
                push = np.array(model["objective"][0])      # the objective as it is, with the push on top:
                push[j] = sign * (4.0 if side == "up" else -4.0)   # (one nonzero alone would make every ratio a tie)
                actions = [("remove", [con["id"]]), ("objective", (push.tolist(), model["objective"][1]))]
                if reference(rewrite(model, dict(actions=actions)))[0] == "unbounded":
                    pending_back = ("back_unbounded", copy.deepcopy(con))
                    return actions
            return None
        raise ValueError(kind)

    for step in range(steps):
        kind, actions = None, None
        if step == 0:
            kind, actions = "solve", []
        elif pending_back is not None:
            kind, con = pending_back
            pending_back = None
            if kind == "back_unbounded":
                added.append(con["id"])
                actions = [("add", [con])]
            elif rng.random() < 0.5:
                actions = [("rhs", {con["id"]: float(x0[int(np.argmax(con["coefs"]))]) - 1.0})]
            else:
                actions = [("remove", [con["id"]])]
        while actions is None:
            blocked = []
            if rng.random() < 0.85:
                for kind in list(todo):             # the first kind still owed that is possible now
                    actions = draw(kind)
                    if actions is not None:
                        todo.remove(kind)
                        break
                    blocked.append(kind)
            if actions is None:                     # a filler: what a blocked kind waits for, if any
                fillers = ["add_slack"] if "remove_added_slack" in blocked else []
                fillers += ["add_cut"] if set(blocked) & {"remove_added_binding", "rhs_added", "remove_then_add"} else []
                fillers = fillers or ["objective", "rhs", "add_cut", "add_slack"]
                kind = fillers[int(rng.integers(0, len(fillers)))]
                actions = draw(kind)
        out.append(dict(kind=kind, actions=actions))
        model_next = rewrite(model, out[-1])
        if kind in ("close", "remove_original", "remove_added_binding", "unbounded"):
            added.clear()       # the session starts over: what it holds is its original model from here on
        model = model_next
        status, _, values = reference(model)
        if status == "optimal":
            xs = values
    return start, out
