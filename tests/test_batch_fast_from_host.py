"""FAST batches re-optimised from their last bases, the part that needs no GPU: the new names, the
argument checks of dzg_batch_solve_fast_from / core.solve_batch_fast(start=...) /
dantzig_amd.sessions(fast=True) (all raised before any device call: on a machine without a GPU a
device call would answer DZG_E_DEVICE), and the float64 transcription of the restart
(tests/batch_fast_from_reference.py) on the warm cases of tests/test_batch_from_host.py: its distance
from the long-double state sets C_FAST_RESTART, and the CPU oracle continued from it takes the pivots
the STRICT reference takes -- the CPU evidence that tests/test_gpu_batch_fast_from.py's cap on LPs
skipped for a near tie is met by these inputs.

Observed (pytest -s prints them): worst D of the transcribed restart 8.097e-15 (ragged 6.705e-15,
mixed 8.097e-15, chunk 4.759e-15, edges 2.386e-15), of the STRICT restart on the same cases
2.403e-14; 275 of 275 continuations identical."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi, core
from tests import batch_fast_from_reference as ffr
from tests import reopt_check as rc
from tests import test_batch_from_host as h
from tests.lp_families import log3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = h.E_ARG


# ------------------------------------------------------------------ exports
def test_the_new_names_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dantzig_amd.h")) as f:
        header = f.read()
    assert re.search(r"#define DZG_ABI_VERSION 4\b", header)
    proto = re.search(r"\bint dzg_batch_solve_fast_from\(const dzg_lp \*lps, const dzg_batch_start \*start, "
                      r"int64_t count,([^;]*)\);", header)
    assert proto, "dzg_batch_solve_fast_from is not declared"
    assert re.search(r"\bdouble dzg_debug_batch_fast_restart_ms\(void\);", header)
    assert {"dzg_batch_solve_fast_from", "dzg_debug_batch_fast_restart_ms"} <= set(_ffi.EXPORTS)
    lib = _ffi.lib()
    assert lib.dzg_abi_version() == 4
    # one argtype per parameter of the declaration: lps, start, count, opts, pivots_per_launch,
    # refactor_every, res
    params = 3 + proto.group(1).count(",") + 1
    assert params == 7
    assert lib.dzg_batch_solve_fast_from.argtypes is not None and len(lib.dzg_batch_solve_fast_from.argtypes) == params
    assert lib.dzg_debug_batch_fast_restart_ms.restype is C.c_double
    assert lib.dzg_debug_batch_fast_restart_ms() == 0.0
    assert inspect.signature(core.solve_batch_fast).parameters["start"].default is None
    assert inspect.signature(dz.sessions).parameters["fast"].default is False


# ------------------------------------------------------------------ argument checks: C ABI
def _call(lps, starts, ppl=0, every=0, **opts):
    """dzg_batch_solve_fast_from on hand-made arguments: (return code, dzg_last_error)."""
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
            arrs = [None if v is None else _ffi.i64(v) for v in s]
            keep.append(arrs)
            c_start[i].basis, c_start[i].nonbasis = _ffi.ptr(arrs[0]), _ffi.ptr(arrs[1])
    o = _ffi.default_opts(**opts)
    rc_ = _ffi.lib().dzg_batch_solve_fast_from(c_lps, c_start, C.c_int64(count), C.byref(o), C.c_int64(ppl),
                                               C.c_int64(every), res)
    return rc_, _ffi.lib().dzg_last_error().decode()


GOOD_START = (np.arange(6, 10), np.arange(6))


@pytest.mark.parametrize("numerics", [core.FAST, core.AUTO, core.STRICT], ids=["fast", "auto", "strict"])
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
def test_c_abi_refuses_a_bad_start_and_names_the_lp(what, make, needle, numerics):
    good = h._lp()
    bad_lp, bad_start = make(h._lp(seed=2))
    rc_, msg = _call([good, good, bad_lp], [None, GOOD_START, bad_start], numerics=numerics)
    assert rc_ == E_ARG, (what, rc_, msg)
    assert "lps[2]" in msg and needle in msg, (what, msg)
    # the text is dzg_batch_solve_from's
    rc2, msg2 = h._call_from([good, good, bad_lp], [None, GOOD_START, bad_start])
    assert rc2 == E_ARG and msg == msg2, (msg, msg2)


def test_c_abi_keeps_the_checks_of_dzg_batch_solve_fast():
    good = h._lp()
    start = [GOOD_START]
    for numerics in (core.FAST, core.AUTO, core.STRICT):
        rc_, msg = _call([good], start, every=-1, numerics=numerics)
        assert rc_ == E_ARG and msg == "batch: refactor_every < 0", msg
        rc_, msg = _call([good], start, ppl=-1, numerics=numerics)
        assert rc_ == E_ARG and msg == "batch: pivots_per_launch < 0", msg
    rc_, msg = _call([good], start, numerics=99)
    assert rc_ == E_ARG and msg == "batch: opts.numerics", msg
    big = core.CoreLP.from_inequality_form(np.ones((129, 2)), np.ones(129), np.ones(2))
    for numerics in (core.FAST, core.AUTO):
        rc_, msg = _call([good, big], [start[0], None], numerics=numerics)
        assert rc_ == E_ARG and "lps[1]" in msg and "DZG_BATCH_MAX_ROWS" in msg, msg
    lib = _ffi.lib()
    call = lib.dzg_batch_solve_fast_from
    assert call(None, None, C.c_int64(1), None, C.c_int64(0), C.c_int64(0), None) == E_ARG
    assert lib.dzg_last_error().decode() == "batch: lps or res is NULL"
    assert call(None, None, C.c_int64(-1), None, C.c_int64(0), C.c_int64(0), None) == E_ARG
    assert lib.dzg_last_error().decode() == "batch: count < 0"
    assert call(None, None, C.c_int64(0), None, C.c_int64(0), C.c_int64(0), None) == 0
    assert call(None, None, C.c_int64(0), None, C.c_int64(0), C.c_int64(-1), None) == E_ARG
    # what was there stays: the STRICT entry point does not take FAST
    rc_, msg = h._call_from([good], start, numerics=core.FAST)
    assert rc_ == E_ARG and "STRICT" in msg, msg


# ------------------------------------------------------------------ argument checks: core.solve_batch_fast
def test_solve_batch_fast_start_value_errors_come_before_the_call():
    lps = [h._lp(seed=1), h._lp(seed=2), h._lp(seed=3)]
    ok = GOOD_START
    with pytest.raises(ValueError, match="2 entries for 3 LPs"):
        core.solve_batch_fast(lps, start=[ok, None])
    with pytest.raises(ValueError, match=r"start\[1\]"):
        core.solve_batch_fast(lps, start=[None, (np.arange(6, 9), np.arange(6)), None])
    with pytest.raises(ValueError, match=r"start\[1\].*partition"):
        core.solve_batch_fast(lps, start=[None, (np.array([0, 0, 6, 7]), np.array([1, 2, 3, 4, 5, 8])), None])
    with pytest.raises(ValueError, match=r"start\[0\]"):
        core.solve_batch_fast(lps, start=[5, None, None])
    with pytest.raises(ValueError, match=r"lps\[1\].*slack-basis form"):
        core.solve_batch_fast([lps[0], core.warm_started(lps[1], 2), lps[2]], start=[None, ok, None])
    with pytest.raises(ValueError, match="refactor_every"):
        core.solve_batch_fast(lps, start=[ok, ok, ok], refactor_every=-1)
    # what was there stays: the STRICT batch does not take FAST
    with pytest.raises(ValueError, match="STRICT"):
        core.solve_batch(lps, start=[ok, ok, ok], numerics=core.FAST)


def test_a_result_of_either_numerics_is_a_start_unless_it_ended_singular_or_panicked():
    lps = [h._lp(seed=1), h._lp(seed=2), h._lp(seed=3)]
    import dataclasses
    r = core.CoreResult(status="optimal", status_code=0, numerics="fast", iterations=3, objective=0.0,
                        basis=np.arange(6, 10), nonbasis=np.arange(6), x=np.zeros(4), xbar=np.ones(4),
                        z=np.zeros(6), zbar=np.ones(6))
    got = core._batch_starts(lps, [r, dataclasses.replace(r, numerics="strict"),
                                   dataclasses.replace(r, status="singular", status_code=4)])
    assert got[2] is None
    for g in got[:2]:
        assert g[0].tolist() == [6, 7, 8, 9] and g[1].tolist() == list(range(6))


# ------------------------------------------------------------------ argument checks: sessions
def test_sessions_fast_constructs_and_the_strict_batch_still_refuses_fast():
    batch = dz.sessions([h._model(3), h._model(2)], fast=True)
    assert isinstance(batch, dz.SessionBatch) and len(batch) == 2
    assert batch.pivots == [] and batch.cold == [] and batch.strict_fallbacks == []
    assert len(dz.SessionBatch([h._model(3)], fast=True, numerics=core.FAST)) == 1
    assert len(dz.sessions([h._model(3)], fast=True, numerics=core.AUTO)) == 1
    with pytest.raises(ValueError, match="FAST or AUTO"):
        dz.sessions([h._model(3)], fast=True, numerics=core.STRICT)
    with pytest.raises(ValueError, match="STRICT"):
        dz.sessions([h._model(3)], numerics=core.FAST)
    with pytest.raises(ValueError, match="STRICT"):
        dz.sessions([h._model(3)], fast=False, numerics=core.FAST)
    with pytest.raises(ValueError, match=r"problems\[1\].*integer"):
        dz.sessions([h._model(3), h._model(3, integer=True)], fast=True)
    assert dz.sessions([h._model(3)]).strict_fallbacks == []


# ------------------------------------------------------------------ the transcription sets the bound
def test_the_transcribed_restart_sets_the_bound_and_continues_as_the_strict_reference():
    worst, worst_strict, same, total = {}, 0.0, 0, 0
    for family, cases in ffr.all_cases().items():
        worst[family] = 0.0
        for w in cases:
            r = ffr.restart(w.a, w.var_col, w.b2, w.c2, w.basis, w.nonbasis)
            assert not r.singular, (family, w.name)
            exact = w.exact()
            worst[family] = max(worst[family], rc.restart_drift(exact, r.state)["D"])
            strict = SimpleNamespace(x=w.ref.x, z=w.ref.z, xbar=r.state.xbar, zbar=r.state.zbar)
            worst_strict = max(worst_strict, rc.restart_drift(exact, strict)["D"])
            got = w.continuation(r.state)
            total += 1
            ok = got.status == w.want.status and log3(got.pivots) == log3(w.want.pivots)
            same += ok
            assert ok, f"{family} {w.name}: the oracle leaves the STRICT reference's path from the transcribed state"
            assert w.want.iterations >= 1, (family, w.name)
    print(f"worst D of the transcribed FAST restart: {max(worst.values()):.3e} "
          f"({', '.join(f'{k} {v:.3e}' for k, v in worst.items())}); of the STRICT restart: {worst_strict:.3e}; "
          f"{same} of {total} continuations identical")
    assert total == 8 + 6 + 257 + 4 and same == total
    for family, d in worst.items():       # the recorded values are what this computes, not stale ones
        assert 0.5 * ffr.C_FAST_RESTART_OBSERVED[family] <= d <= 1.05 * ffr.C_FAST_RESTART_OBSERVED[family], (family, d)
    assert ffr.C_FAST_RESTART == 10 * max(ffr.C_FAST_RESTART_OBSERVED.values())
    assert max(worst.values()) <= ffr.C_FAST_RESTART


def test_the_transcription_reports_the_singular_starts():
    for a, basis, nonbasis in h.singular_cases():
        m, ns = a.shape
        r = ffr.restart(a, None, np.ones(m), np.concatenate([np.ones(ns), np.zeros(m)]), basis, nonbasis)
        assert r.singular
