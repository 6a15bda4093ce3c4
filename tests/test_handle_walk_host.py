"""The reference of the handle walks alone, on the CPU (tests/handle_walk.py): the walks' coverage, so
that a GPU walk cannot pass by doing nothing; no walk meets the oracle's panic; HiGHS agrees with the
mirror after every run to the end; and the mirror's own double-precision restart and carried states
stay a factor of 10 inside the bounds the FAST walk is held to (reopt_check.C_RESTART,
state_check.C_STATE_SHORT).  A seed that misses one of these is replaced; no bound is raised."""
import functools

import numpy as np
import pytest

from tests import extend_check as ec
from tests import handle_walk as hw
from tests import reopt_check as rc
from tests import state_check as sc

HIGHS_VERDICT = {0: "optimal", 2: "infeasible", 3: "unbounded"}


@functools.lru_cache(maxsize=None)
def _survey(walk):
    """One pass of the mirror through the walk; everything the tests below look at."""
    a, b, c, ops = hw.recipe_of(walk)
    mir = hw.Mirror(a, b, c)
    out = dict(applied=set(), rises=0, falls=0, cols_only=set(), remove_both=0, extend_both=0, ends=[],
               restart_d=[], restart_err=[], carried_d=[], highs=[], ms=[mir.lp.m], sizes=[])
    for step, op in enumerate(ops):
        m0, it0 = mir.lp.m, mir.iterations
        if op.call != "run":
            if mir.status != "running" or mir.runs == 0:      # running: before any run
                out["applied"].add((op.call, mir.status))
            if op.call == "remove":
                if not op.kw["rows"]:
                    out["cols_only"].add(m0 % 2)
                out["remove_both"] += bool(op.kw["rows"] and op.kw["cols"])
            if op.call == "extend":
                out["extend_both"] += "rows" in op.kw and "cols" in op.kw
        hw.apply(mir, op)
        out["ms"].append(mir.lp.m)
        out["sizes"].append((mir.lp.m, mir.lp.n_struct))
        out["rises"] += hw.ceil16(mir.lp.m) > hw.ceil16(m0)
        out["falls"] += hw.ceil16(mir.lp.m) < hw.ceil16(m0)
        if op.call == "run":
            out["ends"].append((step, mir.status, mir.iterations - it0))
            out["carried_d"].append((step, hw.exact_carried(mir).drift(mir)["D"]))
            if op.kw["max_new_iters"] == 0:
                status, objective, _, _ = ec.highs(mir.lp)
                out["highs"].append((step, mir.status, mir.objective - mir.lp.constant, status, objective))
        else:
            ex = hw.exact_restart(mir)
            out["restart_d"].append((step, rc.restart_drift(ex, mir)["D"]))
            out["restart_err"].append((step, max(ex.err["x"], ex.err["z"])))
    return out


def test_the_walks_are_the_ones_the_issue_fixes():
    assert [(w.m, w.ns, w.steps) for w in hw.SMALL] == [(14, 20, 40)] * 4
    assert (hw.LARGE.m, hw.LARGE.ns, hw.LARGE.steps, hw.LARGE.m_range[1], hw.LARGE.ns_range[1]) == (60, 70, 25, 72, 80)
    for w in hw.WALKS:
        ops = hw.recipe_of(w)[3]
        assert len(ops) == w.steps
        for m, ns in _survey(w)["sizes"]:
            assert w.m_range[0] <= m <= w.m_range[1] and w.ns_range[0] <= ns <= w.ns_range[1], (w.name, m, ns)


def test_every_call_is_applied_from_every_status():
    applied = set().union(*(_survey(w)["applied"] for w in hw.WALKS))
    missing = [(call, st) for call in hw.RESTARTS for st in hw.STATUSES if (call, st) not in applied]
    assert not missing, missing


def test_the_leading_dimension_rises_and_falls():
    assert sum(_survey(w)["rises"] for w in hw.WALKS) >= 2
    assert sum(_survey(w)["falls"] for w in hw.WALKS) >= 2
    ms = _survey(hw.LARGE)["ms"]
    assert any(x <= 64 < y for x, y in zip(ms, ms[1:])), "the 60x70 walk never crosses 64 rows"


def test_the_removals_and_extensions_take_every_form():
    cols_only = set().union(*(_survey(w)["cols_only"] for w in hw.WALKS))
    assert cols_only == {0, 1}, "a columns-only removal at odd m and one at even m"
    assert sum(_survey(w)["remove_both"] for w in hw.WALKS) >= 1
    assert sum(_survey(w)["extend_both"] for w in hw.WALKS) >= 1


@pytest.mark.parametrize("walk", hw.WALKS, ids=lambda w: w.name)
def test_the_last_run_ends_optimal_after_a_pivot_and_nothing_panics(walk):
    ends = _survey(walk)["ends"]
    assert all(status != "panic" for _, status, _ in ends), ends
    step, status, pivots = ends[-1]
    assert step == walk.steps - 1 and status == "optimal" and pivots >= 1, ends[-1]


@pytest.mark.parametrize("walk", hw.WALKS, ids=lambda w: w.name)
def test_highs_agrees_with_the_mirror_after_every_run_to_the_end(walk):
    checked = 0
    for step, status, objective, h_status, h_objective in _survey(walk)["highs"]:
        assert HIGHS_VERDICT.get(h_status) == status, (walk.name, step, status, h_status)
        if status == "optimal":
            assert abs(objective - h_objective) <= 1e-6 * max(1.0, abs(h_objective)), (walk.name, step)
            checked += 1
    assert checked >= 1


@pytest.mark.parametrize("walk", hw.WALKS, ids=lambda w: w.name)
def test_the_mirrors_own_states_are_a_factor_of_ten_inside_the_bounds(walk):
    s = _survey(walk)
    worst = max(s["restart_d"], key=lambda v: v[1])
    err = max(s["restart_err"], key=lambda v: v[1])
    carried = max(s["carried_d"], key=lambda v: v[1])
    print(f"{walk.name}: {len(s['restart_d'])} restarts, worst D {worst[1]:.2e} at step {worst[0]} (helper error "
          f"{err[1]:.1e}); {len(s['carried_d'])} stops, worst carried D {carried[1]:.2e} at step {carried[0]}")
    assert worst[1] <= rc.C_RESTART / 10, worst
    assert err[1] <= rc.C_RESTART / 100, err
    assert carried[1] <= sc.C_STATE_SHORT / 10, carried


# ---------------------------------------------------------------------- the mirror's rules, one by one
def test_the_mirror_follows_core_and_the_oracle_on_a_hand_written_script():
    """extend then remove of the same rows is the LP again; a cold solve of the extended LP has the
    objective the mirror reaches by carrying on."""
    rng = np.random.default_rng(7)
    a, b, c, x0, _ = hw.base_lp(rng, 9, 11)
    mir = hw.Mirror(a, b, c)
    assert mir.run(3) == "iter_limit" and mir.iterations == 3
    rows = rng.uniform(-1, 1, (2, 11))
    mir.extend(rows=rows, rhs=rows @ x0)
    assert mir.dims() == (11, 22, 11) and mir.basis[-2:].tolist() == [20, 21] and mir.status == "running"
    assert len(mir.pivots) == 3 and mir.iterations == 3
    assert mir.run(0) == "optimal"
    cold = hw.Mirror(np.vstack([a, rows]), np.concatenate([b, rows @ x0]), c)
    assert cold.run(0) == "optimal"
    assert abs(cold.objective - mir.objective) <= 1e-9 * max(1.0, abs(cold.objective))
    free_rows, _ = mir.removable()
    with pytest.raises(ValueError):
        mir.remove(rows=[int(np.flatnonzero(~free_rows)[0])])
    drop = np.flatnonzero(free_rows)[:1].tolist()
    var_map, row_map = mir.remove(rows=drop)
    assert row_map[drop[0]] == -1 and mir.dims() == (10, 21, 11) and sorted(mir.basis.tolist() + mir.nonbasis.tolist()) == list(range(21))
    before = mir.iterations
    assert mir.run(0) == "optimal" and mir.iterations == before     # a free row costs no pivot


def test_max_iter_bounds_the_total_across_the_calls():
    a, b, c, ops, total = hw.capped(hw.CAPPED)
    free, held = hw.Mirror(a, b, c), hw.Mirror(a, b, c, max_iter=total)
    assert total >= 2
    for step, op in enumerate(ops):
        hw.apply(free, op)
        hw.apply(held, op)
        assert held.iterations == min(free.iterations, total), step
        if step < 20:
            assert held.pivots == free.pivots and held.basis.tolist() == free.basis.tolist(), step
    assert free.status == "optimal" and free.iterations > total, "the tail takes no pivot: nothing is bounded"
    assert held.status == "iter_limit" and held.iterations == total
