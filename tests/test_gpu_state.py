"""The state FAST numerics carries (x, xbar, z, zbar), read back at stops of real solves and checked
against the state its basis defines, computed in long double (tests/state_check.py):

a. state_drift is truthful: at a refactorisation, k_drift's number agrees with D computed from the
   same carried state, to within what the GPU's own recomputation can be off by (derived from the
   inverse it reads back and the rounding of its sums: state_check.recompute_floor).
b. the carried state is the basis's: D <= C_STATE[family] at stops that straddle the pricing
   regimes, the eta flushes, CSC input, a warm start and a resumed solve.
c. the gate referee: the next pivot FAST takes from each stop of b is the one the CPU oracle takes
   from the exact state, or FAST flagged it.
d. who drifts: FAST's D and the oracle's D (tests/golden/oracle_states_2001_512x1024.npz) at the
   same pivots of the same solve.
"""
import os

import numpy as np
import pytest

from tests import inverse_check as ic
from tests import state_check as sc
from tests.lp_families import log3, make_lp

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
WORST = {}   # family -> worst D seen (printed at the end: pytest -s)
SEEN = []    # (test, stop, numbers) lines printed at the end


@pytest.fixture(scope="module")
def core():
    from dantzig_amd import core as c

    yield c
    for fam, d in sorted(WORST.items()):
        print(f"state D, worst of family {fam}: {d:.3e} (C_STATE {sc.C_STATE[fam]:.1e}, "
              f"observed {sc.C_STATE_OBSERVED[fam]:.3e})")
    for line in SEEN:
        print(line)


# ------------------------------------------------------------------ a. state_drift is truthful
drift_vs_exact = sc.drift_vs_exact


def _run_to_odd_k(s, pivots):
    """pivots, then one at a time until k (the structural basics) is odd."""
    s.run(pivots)
    for _ in range(8):
        if s.result(log=False).dense_columns % 2:
            return
        s.run(1)
    raise AssertionError("k stayed even")


@pytest.mark.parametrize("m,ns,seed,pivots,big_k", [
    (37, 74, 5137, 25, False),      # m < 64: chunks of B^-T c_B without rows
    (700, 1400, 5800, 301, False),  # k < 512: k_drift_x<16>
    (1037, 2074, 6137, 620, False),  # m not a multiple of 64
    (1024, 2048, 1002, 8500, True),  # config 2 past k = 512: k_drift_x<64>
])
def test_state_drift_is_the_drift_of_the_carried_state(core, m, ns, seed, pivots, big_k):
    """Dense G1 LPs from the slack basis, stopped at an odd k (FTRAN's row function pads to an even
    k), refactorised: k_drift's number is D to within the recomputation's own error."""
    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    a = np.asarray(a)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=-1, poll_interval=64) as s:
        _run_to_odd_k(s, pivots)
        r, d, floor = drift_vs_exact(s, lp, a, ns)
    k = r.dense_columns
    assert k % 2 == 1 and (k > 512) == big_k, k
    assert 0 < r.state_drift < 1e-8 and floor < 1e-9, (r.state_drift, floor)
    assert (r.basis >= ns).sum() > 0, "no basic slack: the slack correction is not exercised"
    SEEN.append(f"a {m}x{ns} pivot {r.iterations} k={k}: state_drift {r.state_drift:.3e}, D {d['D']:.3e}, floor {floor:.2e}")


def test_state_drift_past_65536_nonbasic_columns(core):
    """40 x 70 000: k_drift_z's grid-stride loop covers q > 65 536 positions."""
    a, b, c = core.gen_dense_lp(seed=9397, m=40, n_struct=70000)
    a = np.asarray(a)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=-1, poll_interval=16) as s:
        s.run(30)
        r, d, floor = drift_vs_exact(s, lp, a, 70000)
    assert len(r.nonbasis) > 65536 and floor < 1e-9
    SEEN.append(f"a 40x70000: state_drift {r.state_drift:.3e}, D {d['D']:.3e}, floor {floor:.2e}")


@pytest.mark.parametrize("seed,kind", [(9610, 1), (9611, 2)])
def test_state_drift_with_slacks_in_many_positions(core, seed, kind):
    """Integer and 0/1 LPs: slacks enter and leave, so the basic slacks sit in scattered positions
    (k_drift_x's b0[-1 - bcode] and k_drift_y_slack)."""
    a, b, c = make_lp(seed, kind, 120, 200)
    a = np.asarray(a, dtype=np.float64)
    ns = a.shape[1]
    lp = core.CoreLP.from_inequality_form(a, b, c)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=-1, poll_interval=16) as s:
        s.run(90)
        r, d, floor = drift_vs_exact(s, lp, a, ns)
    slack_pos = np.flatnonzero(r.basis >= ns)
    assert len(slack_pos) > 8 and np.any(r.basis[slack_pos] - ns != slack_pos)
    SEEN.append(f"a kind {kind}: state_drift {r.state_drift:.3e}, D {d['D']:.3e}, floor {floor:.2e}")


@pytest.mark.parametrize("where", ["last", "first"])
def test_state_drift_sees_an_error_at_either_end(core, where):
    """A solve started with z off by 1e-6 at the first or the last nonbasic position (made less
    attractive, so the variable stays there): the carried z keeps that error, D (from the starting
    state z = -c) sees it, and so must k_drift -- every position counts."""
    m, ns = 200, 400
    a, b, c = core.gen_dense_lp(seed=5300, m=m, n_struct=ns)
    a = np.asarray(a)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    import dataclasses

    z0 = lp.z.copy()
    pos = ns - 1 if where == "last" else 0
    z0[pos] += 1e-6 * max(1.0, np.abs(z0).max())
    off = dataclasses.replace(lp, z=z0)
    with core.Solver(off, numerics=core.FAST, refactor_interval=-1, poll_interval=16) as s:
        s.run(60)
        r, d, floor = drift_vs_exact(s, lp, a, ns)
    assert r.nonbasis[pos] == pos
    assert d["z"] > 1e-8 and r.state_drift > 1e-8, (d, r.state_drift)
    SEEN.append(f"a z error at the {where} position: state_drift {r.state_drift:.3e}, D {d['D']:.3e}")


# ------------------------------------------------------------------ b + c. stops and the referee
def check_stop(s, a, ns, start, family, c, var_col=None):
    """b at s's current state, then c: one more pivot against the referee's from the exact state."""
    r = s.result(log=False)
    ex = sc.exact_state(a, ns, start, r.basis, r.nonbasis, var_col=var_col)
    d = ex.drift(r)["D"]
    WORST[family] = max(WORST.get(family, 0.0), d)
    SEEN.append(f"b {family} pivot {r.iterations} k={r.dense_columns}: D {d:.3e}")
    assert max(ex.err.values()) * 1e3 <= sc.C_STATE[family], ex.err
    assert d <= sc.C_STATE[family], (family, r.iterations, ex.drift(r))
    if r.status not in ("iter_limit", "running"):
        return r, d
    status, piv = sc.referee(a, ns, c, ex, var_col=var_col)
    before = r.near_ties
    s.run(1)
    r2 = s.result(log=True, log_cap=r.iterations + 1)
    got = log3(r2.pivots[r.iterations:]) if r2.iterations > r.iterations else []
    if piv is None:
        assert not got or r2.near_ties > before, (family, r.iterations, status, got)
    else:
        assert got == [piv] or r2.near_ties > before, (family, r.iterations, got, piv)
    return r2, d


def run_stops(s, a, ns, start, family, c, stops, var_col=None):
    done = s.result(log=False).iterations
    for stop in stops:
        status = s.run(max(0, stop - done)) if stop > done else "iter_limit"
        r, _ = check_stop(s, a, ns, start, family, c, var_col)
        done = r.iterations
        if status != "iter_limit":
            break
    return s.result(log=False)


# config 2: k >= 127 from pivot 791, k >= 480 from 6 030, k >= rows_T = 635 from 9 033; 21 642 pivots
CONFIG2_STOPS = (700, 800, 6000, 6100, 9000, 9100, 15000, 30000)


@pytest.mark.parametrize("interval,family", [(0, "config 2"), (2500, "config 2 refactorised")])
def test_config2_state_is_the_basis_state_across_the_pricing_regimes(core, interval, family):
    a, b, c = core.gen_dense_lp(seed=1002, m=1024, n_struct=2048)
    a = np.asarray(a)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    opts = dict(refactor_interval=interval) if interval else {}
    with core.Solver(lp, numerics=core.FAST, poll_interval=64, **opts) as s:
        r = run_stops(s, a, 2048, lp, family, lp.c, CONFIG2_STOPS)
    assert r.status == "optimal" and r.iterations == 21642 and r.near_ties == 0
    assert (r.refactors > 0) == (interval > 0)


def test_state_at_the_eta_flushes(core):
    m, ns = 256, 512
    a, b, c = core.gen_dense_lp(seed=4242, m=m, n_struct=ns)
    a = np.asarray(a)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    with core.Solver(lp, numerics=core.FAST, refactor_interval=-1, poll_interval=16) as s:
        run_stops(s, a, ns, lp, "eta flush", lp.c, (62, 64, 126, 128, 190, 192, 400))


@pytest.mark.parametrize("m,per_col", [(150, 4), (1000, 6)])
def test_state_of_a_csc_solve(core, m, per_col):
    """CSC input on the sparse-basis path, from its first pivots to the end of the solve."""
    ns = 5 * m // 2
    cp, ri, val, b, c = core.gen_sparse_lp(8400 + m, m, ns, per_col)
    lp = core.CoreLP.from_csc(m, cp, ri, val, b, c)
    a = ic.Csc(m, cp, ri, val)
    with core.Solver(lp, numerics=core.FAST, poll_interval=16) as s:
        r = run_stops(s, a, ns, lp, "csc", lp.c, (10, 64, 200, 500, 10 ** 6))
    assert r.status == "optimal" and r.dense_columns > 0


def test_state_of_a_warm_start(core):
    """core.warm_started: x = 1, z = -1 on a factorised non-slack basis, matching no b or c."""
    m, ns = 300, 600
    a, b, c = core.gen_dense_lp(seed=5400, m=m, n_struct=ns)
    a = np.asarray(a)
    lp = core.warm_started(core.CoreLP.from_inequality_form(a, b, c), 150)
    with core.Solver(lp, numerics=core.FAST, poll_interval=16) as s:
        run_stops(s, a, ns, lp, "warm start", lp.c, (1, 63, 64, 65, 200))


def test_state_of_a_resumed_solve(core):
    """A solve resumed from another's result at pivot 1 000 (xbar, zbar carried over)."""
    a, b, c = core.gen_dense_lp(seed=2001, m=512, n_struct=1024)
    a = np.asarray(a)
    lp0 = core.CoreLP.from_inequality_form(a, b, c)
    with core.Solver(lp0, numerics=core.FAST, poll_interval=50) as s:
        s.run(1000)
        mid = s.result(log=False)
    lp = core.resumed_from(lp0, mid)
    with core.Solver(lp, numerics=core.FAST, poll_interval=50) as s:
        check_stop(s, a, 1024, lp, "resumed", lp.c)
        run_stops(s, a, 1024, lp, "resumed", lp.c, (65, 1500, 3000))


# ------------------------------------------------------------------ d. who drifts
def test_fast_drifts_no_more_than_the_oracle(core):
    """The oracle's carried state and FAST's at the same pivots of the 512 x 1024 seed-2001 solve
    (whose pivot logs are equal: test_gpu_parity.py), both against the exact state of that basis."""
    fx = np.load(os.path.join(GOLDEN, "oracle_states_2001_512x1024.npz"))
    m, ns = int(fx["m"]), int(fx["n_struct"])
    a, b, c = core.gen_dense_lp(seed=int(fx["seed"]), m=m, n_struct=ns)
    a = np.asarray(a)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    out = []
    with core.Solver(lp, numerics=core.FAST, poll_interval=50) as s:
        done = 0
        for stop in fx["stops"]:
            s.run(int(stop) - done)
            r = s.result(log=False)
            done = r.iterations
            assert done == stop
            assert np.array_equal(r.basis, fx[f"basis_{stop}"].astype(np.int64))
            ex = sc.exact_state(a, ns, lp, r.basis, r.nonbasis)
            d_fast = ex.drift(r)["D"]
            d_ora = ex.drift({k: fx[f"{k}_{stop}"] for k in sc.VECTORS})["D"]
            out.append((int(stop), d_fast, d_ora))
            SEEN.append(f"d pivot {stop}: D_FAST {d_fast:.3e}, D_oracle {d_ora:.3e}")
    for stop, d_fast, d_ora in out[1:]:
        assert d_fast <= d_ora, (stop, d_fast, d_ora)
