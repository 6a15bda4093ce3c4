"""The reference check of the carried state (tests/state_check.py) on the CPU oracle's own states:
it accepts the state the oracle carries after hundreds of pivots, gives the dense and the CSC form
of an LP the same exact state, rejects each of the ways a carried state goes subtly wrong at the
thresholds the GPU tests use, and its referee takes the oracle's own next pivot."""
import os

import numpy as np
import pytest

from oracle import oracle as ora
from tests import inverse_check as ic
from tests import state_check as sc
from tests.lp_families import log3, make_lp

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
# (seed, kind): LPs of at most 128 rows whose oracle solves run a few hundred pivots
CASES = [(8000, 0), (8002, 0), (8001, 1), (8002, 1), (8002, 2), (8009, 2)]


def _start(a, b, c):
    """The slack start of from_inequality_form, as a mapping (no GPU: the core module is not needed)."""
    m, ns = a.shape
    return dict(basis=np.arange(ns, ns + m), nonbasis=np.arange(ns), x=np.asarray(b, dtype=np.float64),
                xbar=None, z=-np.asarray(c, dtype=np.float64), zbar=None)


def _lp(seed, kind):
    a, b, c = make_lp(seed, kind, 90, 128)
    return np.asarray(a, dtype=np.float64), b, c


def _oracle(a, b, c, pivots):
    return ora.simplex_solve(ora.stdform_from_dense(a, b, c), max_iter=pivots)


def _state(res):
    return {k: np.asarray(getattr(res, k)).copy() for k in ("basis", "nonbasis") + sc.VECTORS}


@pytest.fixture(scope="module")
def oracle_stops():
    """Per case: the oracle's state at a few stops (at most 400 pivots) and the exact state there."""
    out = {}
    for seed, kind in CASES:
        a, b, c = _lp(seed, kind)
        full = _oracle(a, b, c, 400)
        stops = sorted({max(1, full.iterations // 3), max(1, 2 * full.iterations // 3), full.iterations})
        rows = []
        for p in stops:
            res = _oracle(a, b, c, p)
            ex = sc.exact_state(a, a.shape[1], _start(a, b, c), res.basis, res.nonbasis)
            rows.append((p, res, ex))
        out[(seed, kind)] = (a, b, c, full, rows)
    return out


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("case", CASES)
def test_accepts_the_oracles_carried_state(oracle_stops, case):
    a, b, c, full, rows = oracle_stops[case]
    assert full.iterations >= 100, "the family does not run long enough to test anything"
    for p, res, ex in rows:
        d = ex.drift(res)
        assert d["D"] <= 0.5 * sc.C_STATE_SHORT, (case, p, d)
        assert max(ex.err.values()) * 1e3 <= min(sc.C_STATE.values()), (case, p, ex.err)


def test_dense_and_csc_give_the_same_exact_state(oracle_stops):
    a, b, c, _, rows = oracle_stops[(8002, 2)]
    m, ns = a.shape
    cols = [np.flatnonzero(a[:, j]) for j in range(ns)]
    csc = ic.Csc(m, np.concatenate([[0], np.cumsum([len(r) for r in cols])]), np.concatenate(cols),
                 np.concatenate([a[r, j] for j, r in enumerate(cols)]))
    for p, res, ex in rows:
        ex2 = sc.exact_state(csc, ns, _start(a, b, c), res.basis, res.nonbasis)
        for name in sc.VECTORS:
            got, want = getattr(ex2, name), getattr(ex, name)
            tol = 1e-3 * sc.C_STATE_MAX * max(1.0, float(np.abs(want).max()))
            assert float(np.abs(got - want).max()) <= tol, (p, name)


def _rejected(ex, state):
    """Rejected at every GPU family's constant but the whole config-2 solve's (state_check.py)."""
    return ex.drift(state)["D"] > sc.C_STATE_SHORT


def test_rejects_the_state_one_pivot_earlier():
    for seed, kind in CASES[:3]:
        a, b, c = _lp(seed, kind)
        later = _oracle(a, b, c, 120)
        earlier = _oracle(a, b, c, 119)
        ex = sc.exact_state(a, a.shape[1], _start(a, b, c), later.basis, later.nonbasis)
        st = _state(earlier)
        st["basis"], st["nonbasis"] = later.basis, later.nonbasis
        assert not _rejected(ex, later)
        assert _rejected(ex, st), (seed, kind)


@pytest.mark.parametrize("name", sc.VECTORS)
def test_rejects_one_entry_off_by_1e_10(oracle_stops, name):
    for case in CASES:
        a, b, c, _, rows = oracle_stops[case]
        p, res, ex = rows[-1]
        st = _state(res)
        v = st[name]
        i = int(np.argmax(np.abs(v)))
        v[i] *= 1.0 + 1e-10
        assert _rejected(ex, st), (case, name, ex.drift(st))


def test_rejects_x_and_xbar_swapped(oracle_stops):
    for case in CASES:
        _, _, _, _, rows = oracle_stops[case]
        _, res, ex = rows[-1]
        st = _state(res)
        st["x"], st["xbar"] = st["xbar"], st["x"]
        assert _rejected(ex, st), case


def test_rejects_a_slack_mapped_to_the_wrong_row(oracle_stops):
    """B with a basic slack's unit column in the wrong row: the state no longer is that basis's."""
    for case in CASES:
        a, b, c, _, rows = oracle_stops[case]
        m, ns = a.shape
        _, res, ex = rows[-1]
        basis = np.asarray(res.basis)
        sl = np.flatnonzero(basis >= ns)
        assert len(sl) >= 2
        # the slack codes as var_col gives them, two rows swapped
        codes = sc.var_codes(len(basis) + len(res.nonbasis), ns)
        r0, r1 = basis[sl[0]] - ns, basis[sl[1]] - ns
        codes[ns + r0], codes[ns + r1] = -1 - r1, -1 - r0
        bad = sc.exact_state(a, ns, _start(a, b, c), basis, res.nonbasis, var_col=codes)
        assert not _rejected(ex, res)
        assert _rejected(bad, res), case


@pytest.mark.parametrize("seed", [8000, 8002, 8003])
def test_the_referee_takes_the_oracles_next_pivot(seed):
    """Kind-0 data: from the exact state of every stop, the referee's pivot is the oracle's."""
    a, b, c = _lp(seed, 0)
    ns = a.shape[1]
    full = _oracle(a, b, c, 400)
    want = log3(full.pivots)
    cfull = np.concatenate([c, np.zeros(a.shape[0])])
    for p in range(0, full.iterations + 1, max(1, full.iterations // 12)):
        res = _oracle(a, b, c, p)
        ex = sc.exact_state(a, ns, _start(a, b, c), res.basis, res.nonbasis)
        status, piv = sc.referee(a, ns, cfull, ex)
        if p < len(want):
            assert piv == want[p], (seed, p, piv, want[p])
        else:
            assert piv is None and status == full.status


def test_the_oracles_drift_in_the_512x1024_solve():
    """The oracle's carried state at pivots 1 000, 4 000, 7 692 of the seed-2001 solve
    (tests/golden/oracle_states_2001_512x1024.npz) against the exact state of its basis: the
    reference's own rounding, which tests/test_gpu_state.py compares FAST's with."""
    fx = np.load(os.path.join(GOLDEN, "oracle_states_2001_512x1024.npz"))
    m, ns = int(fx["m"]), int(fx["n_struct"])
    gen = np.load(os.path.join(GOLDEN, "oracle_pivots_2001_512x1024.npz"))
    assert int(gen["iterations"]) == int(fx["stops"][-1])
    a, b, c = _g1(int(fx["seed"]), m, ns)
    ds = []
    for stop in fx["stops"]:
        st = {k: fx[f"{k}_{stop}"] for k in ("basis", "nonbasis") + sc.VECTORS}
        ex = sc.exact_state(a, ns, _start(a, b, c), st["basis"].astype(np.int64),
                            st["nonbasis"].astype(np.int64))
        ds.append(ex.drift(st)["D"])
        assert max(ex.err.values()) < 1e-14
    print("oracle D at", list(fx["stops"]), ["%.3e" % d for d in ds])
    assert np.allclose(ds, ORACLE_D, rtol=1e-3), ds


# the oracle's D at pivots 1 000, 4 000, 7 692 (FAST's at the same pivots: tests/test_gpu_state.py)
ORACLE_D = (6.421e-12, 7.810e-12, 7.207e-10)


def _g1(seed, m, ns):
    from dantzig_amd import core

    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    return np.asarray(a), b, c
