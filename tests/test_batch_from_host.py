"""Batches re-optimised from their last bases, the part that needs no GPU: the new names, the
argument checks of dzg_batch_solve_from / core.solve_batch(start=...) / dantzig_amd.sessions (all
raised before any device call), and -- with the CPU oracle alone -- the cases
tests/test_gpu_batch_from.py runs, whose seeds are fixed here so that every warm continuation takes
at least one pivot, ends optimal at a basis that passes the independent certificate, and at scale
1e-3 costs fewer pivots than the cold solve of the same changed LP.

The seeds (gen_dense_lp's; reopt_check.moved is seeded with seed + 1000):
  RAGGED       one LP per shape, scale 1: found as the first seed from 100 whose continuation pivots
  MIXED_24x40  scale 1e-3: the first six seeds from 200 whose continuation pivots at all (about one
               24x40 LP in thirty leaves its basis for a change that small)
  CHUNK        257 LPs of 65x8 from seed 3000, scale 1: every one of them pivots (at most 20 times)
  PLANTED      tests/planted.py's seed for the all-structural basis
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi, core
from dantzig_amd import rust as rs
from oracle import oracle as ora
from tests import batch_from_reference as bfr
from tests import planted
from tests import reopt_check as rc
from tests import state_check as sc
from tests.optimality import certificate
from tests.test_reopt_host import CHANGES, _kat
from tests.test_surface import build_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RAGGED = {(1, 3): 105, (2, 3): 103, (16, 24): 100, (17, 24): 100, (33, 40): 100, (64, 40): 100, (65, 72): 100,
          (128, 40): 100}
MIXED_24x40 = [216, 252, 303, 329, 337, 371]
MIXED_SCALE = 1e-3
CHUNK_SEED0, CHUNK_COUNT, CHUNK_SHAPE = 3000, 257, (65, 8)
PLANTED = dict(seed=5, m=12, ns=20)
# seed, m, ns: the first six seeds from 401 (m, ns drawn from the seed) whose continuation pivots
SESSION_SEEDS = [(402, 7, 4), (403, 6, 4), (404, 8, 5), (405, 5, 9), (406, 7, 3), (409, 3, 5)]
KAT_MOVE = dict(seed=11, size=2.0)
# name, {constraint index: new b}, the changed model's constraints as written: changes that pivot
SESSION_KATS = [("non_standard_variables", {0: -2.0}, ["y == -2.0", "-3.0 <= x <= 3.0", "z >= -1"]),
                next(ch[:3] for ch in CHANGES if ch[0] == "inventory_balance")]
# model 6 (non_standard_variables): z >= 0.5 with z <= 0, and the b that takes it back (z >= -1)
SESSION_INFEASIBLE = (6, {2: 0.5}, {2: -1.0})


# ------------------------------------------------------------------ the cases (shared with the GPU tests)
def _case(seed, m, ns, scale=1.0, **kw):
    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    return bfr.warm_case(a, b, c, seed + 1000, scale=scale, **kw)


@functools.lru_cache(maxsize=None)
def ragged_cases():
    return [_case(seed, m, ns) for (m, ns), seed in RAGGED.items()]


@functools.lru_cache(maxsize=None)
def mixed_cases():
    return [_case(seed, 24, 40, scale=MIXED_SCALE) for seed in MIXED_24x40]


@functools.lru_cache(maxsize=None)
def chunk_cases():
    return [_case(CHUNK_SEED0 + k, *CHUNK_SHAPE) for k in range(CHUNK_COUNT)]


@functools.lru_cache(maxsize=None)
def permuted_case():
    """The 16x24 LP of RAGGED with its start's nonbasis handed over in reverse."""
    return _case(RAGGED[(16, 24)], 16, 24, nonbasis_order=np.arange(24)[::-1])


@functools.lru_cache(maxsize=None)
def slack_start_case():
    """An all-slack start: the restart state is (b', -c') and the continuation the cold solve."""
    a, b, c = core.gen_dense_lp(seed=RAGGED[(17, 24)], m=17, n_struct=24)
    a = np.ascontiguousarray(a)
    b2, c2 = rc.moved(7, b, c)
    ref = bfr.restart(a, None, b2, bfr.full_c(c2, 17), np.arange(24, 41), np.arange(24))
    return a, b2, c2, ref, bfr.continuation(ref)


@functools.lru_cache(maxsize=None)
def planted_case():
    """A start whose m basic variables are all structural (tests/planted.py, k = m)."""
    p = planted.planted_optimal(PLANTED["seed"], PLANTED["m"], PLANTED["ns"], PLANTED["m"])
    b2, c2 = rc.moved(PLANTED["seed"] + 1000, p.b, p.c)
    ref = bfr.restart(p.a, None, b2, bfr.full_c(c2, PLANTED["m"]), p.basis, p.nonbasis)
    return p, b2, c2, ref, bfr.continuation(ref)


def model_form(problem):
    arrays, order = rs.lower(problem._core_objective().to_rust_affexpr(), list(problem.yield_rust_inequalities()))
    return rs.standard_form(arrays), order


def rhs_by_row(form):
    """The right-hand side of a slack-basis standard form by constraint row."""
    b = np.empty(form.m)
    b[-1 - form.var_col[form.basis]] = form.x
    return b


def model_warm(form0, form1):
    """(the oracle's cold result on form0, the restart of form1's data at that basis, its continuation)."""
    sf0 = sc.stdform(form0.a, form0.n_struct, form0.c, form0, form0.var_col)
    sf0.constant = float(form0.constant)
    first = ora.simplex_solve(sf0)
    ref = bfr.restart(form0.a, form0.var_col, rhs_by_row(form1), form1.c, first.basis, first.nonbasis,
                      form1.constant)
    return first, ref, bfr.continuation(ref)


@functools.lru_cache(maxsize=None)
def kat_case():
    """non_standard_variables lowered: bound rows, a split free variable, var_col from the builder;
    the change of tests/test_gpu_reopt.py's bound-row test at four times the size (KAT_MOVE: with
    0.5 the basis stays optimal), its seed the first whose continuation takes two pivots."""
    _, problem = build_problem(_kat("non_standard_variables"))
    f, _ = model_form(problem)
    rng = np.random.default_rng(KAT_MOVE["seed"])
    x2 = f.x + KAT_MOVE["size"] * rng.random(f.m)     # by position, as the LP is handed over
    c2 = f.c - np.where(f.var_col >= 0, KAT_MOVE["size"] * rng.random(f.n), 0.0)
    sf0 = sc.stdform(f.a, f.n_struct, f.c, f, f.var_col)
    sf0.constant = float(f.constant)
    first = ora.simplex_solve(sf0)
    b2 = np.empty(f.m)
    b2[-1 - f.var_col[f.basis]] = x2
    ref = bfr.restart(f.a, f.var_col, b2, c2, first.basis, first.nonbasis, f.constant)
    return f, x2, c2, first, ref, bfr.continuation(ref)


def singular_cases():
    """(a, basis, nonbasis) with a duplicated structural column, both copies basic.  4x5: the zero
    pivot comes at step 1 and steps 2 and 3 find pivots again (the flag must be sticky).  2x3: the
    zero is the last diagonal entry, which no elimination step visits."""
    a4 = np.array([[1.0, 1.0, 0.5, -0.25, 0.75],
                   [2.0, 2.0, -1.5, 0.5, 0.25],
                   [0.5, 0.5, 3.0, 1.0, -0.5],
                   [0.25, 0.25, 1.0, -2.0, 1.5]])
    a2 = np.array([[1.0, 1.0, 0.5], [1.0, 1.0, -0.5]])
    return [(a4, np.array([0, 1, 2, 5 + 3]), np.array([3, 4, 5, 6, 7])),
            (a2, np.array([0, 1]), np.array([2, 3, 4]))]


def _dense_model(a, b, c):
    ns = a.shape[1]
    xs = [dz.Variable.nonneg() for _ in range(ns)]
    cons = [sum(float(a[i, j]) * xs[j] for j in range(ns)) <= float(b[i]) for i in range(a.shape[0])]
    return dz.Maximize(sum(float(c[j]) * xs[j] for j in range(ns))).subject_to(cons)


def session_problems():
    """Eight small models, two of them KATs: (problem, {constraint index: new b}, the changed model
    written out afresh)."""
    out = []
    for seed, m, ns in SESSION_SEEDS:
        a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
        b2, _ = rc.moved(seed + 1000, b, c)
        out.append((_dense_model(a, b, c), {i: float(b2[i]) for i in range(m)}, _dense_model(a, b2, c)))
    for name, new_b, written in SESSION_KATS:
        out.append((build_problem(_kat(name))[1], dict(new_b),
                    build_problem(dict(_kat(name), constraints=written))[1]))
    return out


@functools.lru_cache(maxsize=None)
def session_reference():
    """Per model: (the oracle's cold result, the restart, the continuation, the changed form)."""
    out = []
    for problem, new_b, _ in session_problems():
        form0, _ = model_form(problem)
        session = problem.session()
        session._change(None, {problem.constraints[i]: b for i, b in new_b.items()})
        form1 = rs.standard_form(session._lowered()[1])
        first, ref, want = model_warm(form0, form1)
        out.append((first, ref, want, form1))
    return out


# ------------------------------------------------------------------ exports
def test_the_new_names_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dantzig_amd.h")) as f:
        header = f.read()
    assert re.search(r"#define DZG_ABI_VERSION 4\b", header)
    assert re.search(r"\bint dzg_batch_solve_from\(const dzg_lp \*lps, const dzg_batch_start \*start, int64_t count,",
                     header)
    assert re.search(r"const int64_t \*basis;[^\n]*\n\s*const int64_t \*nonbasis;[^\n]*\n\} dzg_batch_start;", header)
    assert "dzg_batch_solve_from" in _ffi.EXPORTS
    lib = _ffi.lib()
    assert lib.dzg_abi_version() == 4
    assert lib.dzg_batch_solve_from.argtypes is not None and len(lib.dzg_batch_solve_from.argtypes) == 7
    assert C.sizeof(_ffi.BatchStart) == 16
    import inspect
    assert inspect.signature(core.solve_batch).parameters["start"].default is None
    assert dz.sessions is not None and isinstance(dz.SessionBatch, type)


# ------------------------------------------------------------------ argument checks: C ABI
def _call_from(lps, starts, **opts):
    """dzg_batch_solve_from on hand-made arguments: (return code, dzg_last_error)."""
    marshalled = [core._c_lp(lp) for lp in lps]
    count = len(lps)
    c_lps = (_ffi.Lp * max(count, 1))(*[c for c, _ in marshalled])
    res = (_ffi.Result * max(count, 1))()
    keep, c_start = [], None
    if starts is not None:
        c_start = (_ffi.BatchStart * max(count, 1))()
        for i, s in enumerate(starts):
            if s is None:
                continue
            basis, nonbasis = s
            arrs = [None if v is None else _ffi.i64(v) for v in (basis, nonbasis)]
            keep.append(arrs)
            c_start[i].basis, c_start[i].nonbasis = _ffi.ptr(arrs[0]), _ffi.ptr(arrs[1])
    o = _ffi.default_opts(**opts)
    rc_ = _ffi.lib().dzg_batch_solve_from(c_lps, c_start, C.c_int64(count), C.byref(o), C.c_int64(0), res, None)
    return rc_, _ffi.lib().dzg_last_error().decode()


def _lp(seed=1, m=4, ns=6):
    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    return core.CoreLP.from_inequality_form(a, b, c)


E_ARG = -2


def test_e_arg_is_the_code_the_checks_return():
    with open(os.path.join(ROOT, "include", "dantzig_amd.h")) as f:
        assert re.search(r"DZG_E_ARG\s*=\s*-2\b", f.read())


@pytest.mark.parametrize("what,make,needle", [
    ("own basis not all slack",
     lambda lp: (core.warm_started(lp, 2), (np.arange(4, 8), np.r_[np.arange(4), 8, 9])), "not all slack"),
    ("nonbasis NULL", lambda lp: (lp, (np.arange(6, 10), None)), "nonbasis is NULL"),
    ("repeated entry", lambda lp: (lp, (np.array([0, 0, 6, 7]), np.array([1, 2, 3, 4, 5, 8]))), "not a partition"),
    ("entry out of range", lambda lp: (lp, (np.array([0, 1, 6, 10]), np.array([2, 3, 4, 5, 8, 9]))),
     "not a partition"),
    ("negative entry", lambda lp: (lp, (np.array([0, 1, 6, -1]), np.array([2, 3, 4, 5, 8, 9]))), "not a partition"),
    ("shared entry", lambda lp: (lp, (np.array([0, 1, 6, 7]), np.array([1, 2, 3, 4, 5, 8]))), "not a partition"),
], ids=lambda v: v if isinstance(v, str) and " " in v else None)
def test_c_abi_refuses_a_bad_start_and_names_the_lp(what, make, needle):
    good = _lp()
    bad_lp, bad_start = make(_lp(seed=2))
    rc_, msg = _call_from([good, good, bad_lp], [None, (np.arange(6, 10), np.arange(6)), bad_start])
    assert rc_ == E_ARG, (what, rc_, msg)
    assert "lps[2]" in msg and needle in msg, (what, msg)


def test_c_abi_keeps_the_checks_of_dzg_batch_solve():
    good = _lp()
    start = [(np.arange(6, 10), np.arange(6))]
    rc_, msg = _call_from([good], start, numerics=core.FAST)
    assert rc_ == E_ARG and "STRICT" in msg, msg
    big = core.CoreLP.from_inequality_form(np.ones((129, 2)), np.ones(129), np.ones(2))
    rc_, msg = _call_from([good, big], [start[0], None])
    assert rc_ == E_ARG and "lps[1]" in msg and "DZG_BATCH_MAX_ROWS" in msg, msg
    lib = _ffi.lib()
    assert lib.dzg_batch_solve_from(None, None, C.c_int64(1), None, C.c_int64(0), None, None) == E_ARG
    assert lib.dzg_batch_solve_from(None, None, C.c_int64(-1), None, C.c_int64(0), None, None) == E_ARG
    assert lib.dzg_batch_solve_from(None, None, C.c_int64(0), None, C.c_int64(0), None, None) == 0


# ------------------------------------------------------------------ argument checks: core.solve_batch
def test_solve_batch_start_value_errors_come_before_the_call():
    lps = [_lp(seed=1), _lp(seed=2), _lp(seed=3)]
    ok = (np.arange(6, 10), np.arange(6))
    with pytest.raises(ValueError, match="2 entries for 3 LPs"):
        core.solve_batch(lps, start=[ok, None])
    with pytest.raises(ValueError, match=r"start\[1\]"):
        core.solve_batch(lps, start=[None, (np.arange(6, 9), np.arange(6)), None])
    with pytest.raises(ValueError, match=r"start\[2\]"):
        core.solve_batch(lps, start=[None, None, (np.arange(6, 10), np.arange(5))])
    with pytest.raises(ValueError, match=r"start\[1\].*partition"):
        core.solve_batch(lps, start=[None, (np.array([0, 0, 6, 7]), np.array([1, 2, 3, 4, 5, 8])), None])
    with pytest.raises(ValueError, match=r"start\[0\]"):
        core.solve_batch(lps, start=[5, None, None])
    with pytest.raises(ValueError, match=r"lps\[1\].*slack-basis form"):
        core.solve_batch([lps[0], core.warm_started(lps[1], 2), lps[2]], start=[None, ok, None])
    with pytest.raises(ValueError, match="ranging or rays"):
        core.solve_batch(lps, start=[ok, ok, ok], ranging=True)
    with pytest.raises(ValueError, match="ranging or rays"):
        core.solve_batch(lps, start=[ok, ok, ok], rays=True)
    with pytest.raises(ValueError, match="STRICT"):
        core.solve_batch(lps, start=[ok, ok, ok], numerics=core.FAST)


def test_a_singular_or_panicked_result_counts_as_no_start():
    lps = [_lp(seed=1), _lp(seed=2)]
    r = core.CoreResult(status="singular", status_code=4, numerics="strict", iterations=0, objective=0.0,
                        basis=np.arange(6, 10), nonbasis=np.arange(6), x=np.zeros(4), xbar=np.ones(4),
                        z=np.zeros(6), zbar=np.ones(6))
    import dataclasses
    p = dataclasses.replace(r, status="panic", status_code=5)
    o = dataclasses.replace(r, status="optimal", status_code=0)
    got = core._batch_starts(lps, [r, p])
    assert got == [None, None]
    got = core._batch_starts(lps, [o, None])
    assert got[1] is None and got[0][0].tolist() == [6, 7, 8, 9] and got[0][1].tolist() == list(range(6))


# ------------------------------------------------------------------ argument checks: sessions
def _model(rows, integer=False):
    x = dz.Variable.nonneg()
    y = dz.Variable.integer() if integer else dz.Variable.nonneg()
    cons = [x + (k + 1) * y <= 10.0 + k for k in range(rows)]
    return dz.Maximize(x + y).subject_to(cons)


def test_sessions_refuses_what_the_strict_batch_does_not_take():
    extra = model_form(_model(1))[0].m - 1           # the rows the lowering adds to the written ones
    assert model_form(_model(128 - extra))[0].m == 128
    dz.sessions([_model(128 - extra)])
    with pytest.raises(ValueError, match=r"problems\[1\].*129 rows"):
        dz.sessions([_model(3), _model(129 - extra)])
    with pytest.raises(ValueError, match=r"problems\[2\].*integer"):
        dz.sessions([_model(3), _model(2), _model(3, integer=True)])
    with pytest.raises(ValueError, match="STRICT"):
        dz.sessions([_model(3)], numerics=core.FAST)
    with pytest.raises(TypeError, match=r"problems\[0\]"):
        dz.sessions([object()])
    batch = dz.sessions([_model(3), _model(2)])
    assert len(batch) == 2 and batch.pivots == [] and batch.cold == []
    with pytest.raises(ValueError, match="1 entries for 2 models"):
        batch.solve(rhs=[{}])
    with pytest.raises(KeyError, match=r"rhs\[1\]"):
        batch.solve(rhs=[None, {_model(1).constraints[0]: 1.0}])
    assert batch.pivots == [] and batch.cold == []


def test_session_keeps_lowering_as_the_builder_does():
    """The lowering Session and SessionBatch share is the one Session had: a changed session lowers to
    the written model's form."""
    for problem, new_b, written in session_problems():
        session = problem.session()
        session._change(None, {problem.constraints[i]: b for i, b in new_b.items()})
        batch = dz.sessions([problem])
        st = batch._models[0]
        rhs = {id(problem.constraints[i]): -(0.0 - float(b)) for i, b in new_b.items()}
        form, _ = batch._lower(0, problem, st.objective, rhs)
        want = rs.standard_form(session._lowered()[1])
        assert form.same_shape_as(want)
        assert form.x.tobytes() == want.x.tobytes() and form.c.tobytes() == want.c.tobytes()
        fresh, _ = model_form(written)
        assert form.same_shape_as(fresh) and np.array_equal(form.x, fresh.x) and np.array_equal(form.c, fresh.c)


# ------------------------------------------------------------------ the cases the GPU tests rely on
def _passes_certificate(a, b, c, basis, objective):
    cert = certificate(a, b, c, basis)
    scale = max(1.0, abs(cert["primal_obj"]))
    assert cert["primal_infeas"] <= 1e-9 and cert["dual_infeas"] <= 1e-9, cert
    assert abs(cert["primal_obj"] - cert["dual_obj"]) <= 1e-9 * scale, cert
    assert abs(objective - cert["primal_obj"]) <= 1e-9 * scale, (objective, cert)


@pytest.mark.parametrize("cases", [ragged_cases, mixed_cases, chunk_cases, lambda: [permuted_case()]],
                         ids=["ragged", "mixed 24x40", "chunk 257 x 65x8", "permuted nonbasis"])
def test_every_warm_case_pivots_and_ends_at_a_certified_optimum(cases):
    for k, w in enumerate(cases()):
        what = f"case {k}: {w.a.shape}"
        assert w.first.status == "optimal" and not w.ref.singular, what
        assert w.want.status == "optimal" and w.want.iterations >= 1, (what, w.want.status, w.want.iterations)
        _passes_certificate(w.a, w.b2, w.c2, w.want.basis, w.want.objective)


def test_the_edge_cases_pivot_and_end_at_a_certified_optimum():
    a, b2, c2, ref, want = slack_start_case()
    assert_state = np.testing.assert_array_equal
    assert_state(ref.x, b2)            # the basis is all slack: x = b' and z = -c', exactly
    assert_state(ref.z, -c2)
    cold = bfr.cold(a, b2, c2)
    assert want.status == "optimal" and want.iterations >= 1 and want.pivots == cold.pivots
    _passes_certificate(a, b2, c2, want.basis, want.objective)
    p, b2, c2, ref, want = planted_case()
    assert (p.basis < PLANTED["ns"]).all() and not ref.singular
    assert want.status == "optimal" and want.iterations >= 1
    _passes_certificate(p.a, b2, c2, want.basis, want.objective)
    f, _, _, first, ref, want = kat_case()
    assert f.m == 7 and f.n_struct == 6 and len(f.var_col) == f.n       # bound rows, a split free variable
    assert first.status == "optimal" and not ref.singular
    assert want.status == "optimal" and want.iterations >= 1


def test_at_scale_1e_3_the_warm_24x40_batch_pivots_less_than_the_cold_one():
    warm = sum(w.want.iterations for w in mixed_cases())
    cold = sum(bfr.cold(w.a, w.b2, w.c2).iterations for w in mixed_cases())
    print(f"24x40 x {len(MIXED_24x40)} at scale {MIXED_SCALE}: {warm} pivots warm, {cold} cold")
    assert 0 < warm < cold


def test_the_duplicated_column_meets_an_exact_zero_pivot_in_the_oracles_lu():
    (a4, basis4, nonbasis4), (a2, basis2, nonbasis2) = singular_cases()
    b4 = sc.columns(a4, 4, sc.var_codes(9, 5)[basis4])
    lu, _ = ora.lu_factorize(b4)
    d = np.diag(lu)
    assert d[1] == 0.0 and d[0] != 0.0 and d[2] != 0.0 and d[3] != 0.0, d    # sticky: steps 2, 3 pivot again
    b2 = sc.columns(a2, 2, sc.var_codes(5, 3)[basis2])
    lu, _ = ora.lu_factorize(b2)
    assert np.diag(lu)[0] != 0.0 and np.diag(lu)[1] == 0.0                   # the entry no step visits
    for a, basis, nonbasis in singular_cases():
        m, ns = a.shape
        ref = bfr.restart(a, None, np.ones(m), bfr.full_c(np.ones(ns), m), basis, nonbasis)
        assert ref.singular


def test_the_session_cases_pivot_where_they_should():
    refs = session_reference()
    assert len(refs) == 8
    for k, (first, ref, want, _) in enumerate(refs):
        assert first.status == "optimal" and not ref.singular and want.status == "optimal", (k, want.status)
    assert all(want.iterations >= 1 for _, _, want, _ in refs)
    print("session continuation pivots:", [want.iterations for _, _, want, _ in refs])
