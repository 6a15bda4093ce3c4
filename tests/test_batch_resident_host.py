"""A batch kept resident on the GPU, the part that needs no GPU: the new names, the host checks of
dzg_batch_create / core.BatchSolver (all made before any device call, so they answer on a machine
without a device), the arguments of SessionBatch(resident=True), and -- with a stand-in for
core.BatchSolver that records what it is told -- which models a resident SessionBatch sends, which
it tells to go cold, and when it builds its handle again."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi, core
from tests import test_batch_from_host as h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -2
NAMES = ["dzg_batch_create", "dzg_batch_destroy", "dzg_batch_update", "dzg_batch_set_start", "dzg_batch_resolve",
         "dzg_debug_batch_traffic"]


# ------------------------------------------------------------------ exports
def test_the_new_names_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "dantzig_amd.h")) as f:
        header = f.read()
    assert re.search(r"#define DZG_ABI_VERSION 4\b", header)
    assert "typedef struct dzg_batch dzg_batch;" in header
    assert re.search(r"int32_t set_constant, reserved;\s*\n\} dzg_batch_change;", header)
    lib = _ffi.lib()
    assert lib.dzg_abi_version() == 4
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _ffi.EXPORTS, name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.dzg_batch_create.argtypes) == 7 and len(lib.dzg_batch_resolve.argtypes) == 4
    assert C.sizeof(_ffi.BatchChange) == 40
    assert _ffi.BatchChange.constant.offset == 24 and _ffi.BatchChange.set_constant.offset == 32
    for out_of_scope in ("duals, ranging and rays", "adding or removing rows", "folding the restart"):
        assert out_of_scope in header, out_of_scope
    for method in ("update", "update_many", "set_start", "solve", "traffic", "close", "__enter__", "__exit__", "__del__"):
        assert callable(getattr(core.BatchSolver, method)), method
    import inspect
    assert inspect.signature(dz.sessions).parameters["resident"].default is False
    assert inspect.signature(dz.SessionBatch.__init__).parameters["resident"].default is False


# ------------------------------------------------------------------ create: the C ABI's host checks
def _lp(seed=1, m=4, ns=6):
    a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
    return core.CoreLP.from_inequality_form(a, b, c)


def _create(lps, ppl=0, refactor=0, log_cap=0, **opts):
    """dzg_batch_create on hand-made arguments: (return code, dzg_last_error)."""
    marshalled = [core._c_lp(lp) for lp in lps]
    c_lps = (_ffi.Lp * max(len(lps), 1))(*[c for c, _ in marshalled])
    o = _ffi.default_opts(**opts)
    out = C.c_void_p()
    rc = _ffi.lib().dzg_batch_create(c_lps, C.c_int64(len(lps)), C.byref(o), C.c_int64(ppl), C.c_int64(refactor),
                                     C.c_int64(log_cap), C.byref(out))
    msg = _ffi.lib().dzg_last_error().decode()
    if out.value:
        _ffi.lib().dzg_batch_destroy(out)
    return rc, msg


def test_create_refuses_bad_arguments_before_any_device_work():
    good = _lp()
    lib = _ffi.lib()
    out = C.c_void_p()
    assert lib.dzg_batch_create(None, C.c_int64(1), None, C.c_int64(0), C.c_int64(0), C.c_int64(0), C.byref(out)) == E_ARG
    assert lib.dzg_batch_create(None, C.c_int64(-1), None, C.c_int64(0), C.c_int64(0), C.c_int64(0), C.byref(out)) == E_ARG
    assert lib.dzg_batch_create(None, C.c_int64(0), None, C.c_int64(0), C.c_int64(0), C.c_int64(0), None) == E_ARG
    assert "out is NULL" in lib.dzg_last_error().decode()
    for kw, needle in ((dict(ppl=-1), "pivots_per_launch < 0"), (dict(refactor=-1), "refactor_every < 0"),
                       (dict(log_cap=-1), "log_cap < 0"), (dict(numerics=7), "numerics")):
        rc, msg = _create([good], **kw)
        assert rc == E_ARG and needle in msg, (kw, rc, msg)


def test_create_names_the_lp_it_refuses():
    good = _lp()
    big = core.CoreLP.from_inequality_form(np.ones((129, 2)), np.ones(129), np.ones(2))
    with_bars = _lp(seed=2)
    with_bars.xbar, with_bars.zbar = np.ones(4), np.ones(6)
    repeated = _lp(seed=3)
    repeated.nonbasis = np.array([0, 0, 2, 3, 4, 5])
    for bad, needle in ((big, "DZG_BATCH_MAX_ROWS"), (core.warm_started(_lp(seed=2), 2), "not all slack"),
                        (with_bars, "xbar / zbar"), (repeated, "")):
        rc, msg = _create([good, good, bad])
        assert rc == E_ARG and "lps[2]" in msg and needle in msg, (rc, msg)


def test_an_empty_handle_is_valid_and_every_call_on_it_checks_its_arguments():
    lib = _ffi.lib()
    out = C.c_void_p()
    assert lib.dzg_batch_create(None, C.c_int64(0), None, C.c_int64(0), C.c_int64(0), C.c_int64(0), C.byref(out)) == 0
    assert out.value
    try:
        assert lib.dzg_batch_resolve(out, None, C.c_int64(0), None) == 0
        assert lib.dzg_batch_update(out, None, C.c_int64(0)) == 0
        assert lib.dzg_batch_update(out, None, C.c_int64(1)) == E_ARG
        chg = (_ffi.BatchChange * 1)()
        assert lib.dzg_batch_update(out, chg, C.c_int64(1)) == E_ARG and "out of range" in lib.dzg_last_error().decode()
        which = _ffi.i64([0])
        res = (_ffi.Result * 1)()
        assert lib.dzg_batch_resolve(out, _ffi.ptr(which), C.c_int64(1), res) == E_ARG
        assert "which[0]" in lib.dzg_last_error().decode()
        assert lib.dzg_batch_resolve(out, _ffi.ptr(which), C.c_int64(-1), res) == E_ARG
        assert lib.dzg_batch_set_start(out, C.c_int64(0), None, None) == E_ARG
        nbytes, ms = (C.c_int64 * 2)(7, 7), (C.c_double * 1)(7.0)
        assert lib.dzg_debug_batch_traffic(out, nbytes, ms) == 0 and list(nbytes) == [0, 0] and ms[0] == 0.0
    finally:
        lib.dzg_batch_destroy(out)
    assert lib.dzg_batch_update(None, None, C.c_int64(0)) == E_ARG
    lib.dzg_batch_destroy(None)


# ------------------------------------------------------------------ create: core.BatchSolver
def test_batch_solver_raises_value_errors_with_the_index():
    good = _lp()
    with pytest.raises(ValueError, match=r"lps\[1\].*129 rows"):
        core.BatchSolver([good, core.CoreLP.from_inequality_form(np.ones((129, 2)), np.ones(129), np.ones(2))])
    with pytest.raises(ValueError, match=r"lps\[1\].*not all slack"):
        core.BatchSolver([good, core.warm_started(_lp(seed=2), 2)])
    with_bars = _lp(seed=2)
    with_bars.xbar = np.ones(4)
    with pytest.raises(ValueError, match=r"lps\[2\].*xbar"):
        core.BatchSolver([good, good, with_bars])
    sparse = core.CoreLP.from_csc(2, [0, 1, 2], [0, 1], [1.0, 1.0], np.ones(2), np.ones(2))
    with pytest.raises(ValueError, match=r"lps\[0\].*CSC"):
        core.BatchSolver([sparse])
    for kw in (dict(log_cap=-1), dict(pivots_per_launch=-1), dict(refactor_every=-1)):
        with pytest.raises(ValueError, match=">= 0"):
            core.BatchSolver([good], **kw)
    with pytest.raises(ValueError, match="numerics"):
        core.BatchSolver([good], numerics=7)
    with pytest.raises(ValueError, match="no_such_option"):
        core.BatchSolver([good], no_such_option=1)
    with core.BatchSolver([]) as empty:
        assert len(empty) == 0 and empty.solve() == [] and empty.traffic() == (0, 0, 0.0)
        with pytest.raises(ValueError, match="out of range"):
            empty.update(0, b=np.ones(1))
    with pytest.raises(ValueError, match="closed"):
        empty.solve()


def test_without_a_device_create_fails_loudly_after_the_checks():
    if _ffi.lib().dzg_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_ffi.DantzigAmdError, match="no HIP device"):
        core.BatchSolver([_lp()])


# ------------------------------------------------------------------ SessionBatch(resident=True)
def _model(rows, integer=False):
    x = dz.Variable.nonneg()
    y = dz.Variable.integer() if integer else dz.Variable.nonneg()
    cons = [x + (k + 1) * y <= 10.0 + k for k in range(rows)]
    return dz.Maximize(x + y).subject_to(cons)


def test_resident_sessions_check_their_arguments_as_the_stateless_ones_do():
    with pytest.raises(TypeError, match="resident"):
        dz.sessions([_model(2)], resident="yes")
    with pytest.raises(ValueError, match=r"problems\[1\].*integer"):
        dz.sessions([_model(3), _model(3, integer=True)], resident=True)
    with pytest.raises(ValueError, match="STRICT"):
        dz.sessions([_model(3)], resident=True, numerics=core.FAST)
    with pytest.raises(ValueError, match="FAST or AUTO"):
        dz.sessions([_model(3)], fast=True, resident=True, numerics=core.STRICT)
    with dz.sessions([_model(3), _model(2)], resident=True) as batch:
        assert len(batch) == 2 and batch.rebuilds == 0 and batch.pivots == []
        with pytest.raises(ValueError, match="1 entries for 2 models"):
            batch.solve(rhs=[{}])
    batch.close()     # (twice is fine)


class _Recorder:
    """Stands in for core.BatchSolver: records the calls and answers every solve with the slack basis
    as an optimal result -- or with the status planted for an LP."""
    made = []

    def __init__(self, lps, log_cap=4096, **opts):
        self.lps, self.log_cap, self.opts = list(lps), log_cap, opts
        self.calls, self.closed, self.plant = [], False, {}
        _Recorder.made.append(self)

    def update_many(self, changes):
        self.calls.append(("update_many", [(i, None if b is None else np.array(b), None if c is None else np.array(c), k)
                                           for i, b, c, k in changes]))

    def set_start(self, i, start):
        self.calls.append(("set_start", i, start))

    def solve(self, which=None, log=True):
        self.calls.append(("solve", which, log))
        out = []
        for i, lp in enumerate(self.lps):
            status = self.plant.get(i, "optimal")
            out.append(core.CoreResult(
                status=status, status_code={"optimal": 0, "singular": 4}[status], numerics="strict", iterations=i,
                objective=0.0, basis=np.array(lp.basis), nonbasis=np.array(lp.nonbasis), x=np.array(lp.x),
                xbar=np.ones(lp.m), z=np.array(lp.z), zbar=np.ones(lp.n - lp.m)))
        return out

    def close(self):
        self.closed = True


@pytest.fixture
def recorder(monkeypatch):
    _Recorder.made = []
    monkeypatch.setattr(core, "BatchSolver", _Recorder)
    return _Recorder


def test_resident_sessions_send_what_moved_and_tell_whom_to_go_cold(recorder):
    models = [_model(3), _model(2), _model(4)]
    batch = dz.sessions(models, resident=True, max_iter=77)
    batch.solve()
    assert len(recorder.made) == 1
    first = recorder.made[0]
    assert first.log_cap == 0 and first.opts == dict(max_iter=77, numerics=core.STRICT)
    assert [lp.m for lp in first.lps] == [st.form.m for st in batch._models]
    assert first.calls == [("solve", None, False)]
    assert batch.cold == [3] and batch.pivots == [[0, 1, 2]] and batch.rebuilds == 0

    # model 1's b moves: it alone is sent, by constraint row; nobody goes cold
    first.calls.clear()
    con = models[1].constraints[1]
    batch.solve(rhs=[None, {con: 5.5}, None])
    assert [c[0] for c in first.calls] == ["update_many", "solve"]
    (i, b, c, constant), = first.calls[0][1]
    assert i == 1 and c is None and constant is None
    assert b.tobytes() == h.rhs_by_row(batch._models[1].form).tobytes() and 5.5 in b.tolist()
    assert batch.cold == [3, 0]

    # an unchanged call sends nothing; a model that ended singular is told to go cold in the next
    first.calls.clear()
    first.plant = {2: "singular"}
    out = batch.solve(return_exceptions=True)
    assert isinstance(out[2], RuntimeError) and first.calls == [("solve", None, False)]
    first.calls.clear()
    first.plant = {}
    batch.solve(objectives=[2 * models[0].objective, None, None])
    assert first.calls[0] == ("set_start", 2, None)
    assert first.calls[1][0] == "update_many" and [ch[0] for ch in first.calls[1][1]] == [0]
    assert first.calls[1][1][0][1] is None and first.calls[1][1][0][2] is not None      # c alone
    assert batch.cold == [3, 0, 0, 1] and len(recorder.made) == 1


def test_a_change_of_shape_builds_the_handle_again_and_puts_the_other_bases_back(recorder):
    models = [_model(3), _model(2), _model(4)]
    with dz.sessions(models, fast=True, resident=True) as batch:
        batch.solve()
        first = recorder.made[0]
        assert "numerics" not in first.opts               # fast: AUTO, the handle's default
        last = [st.last for st in batch._models]
        w = dz.Variable(lb=0.0, ub=1.0)
        batch.solve(objectives=[models[0].objective + w, None, None])
        assert batch.rebuilds == 1 and len(recorder.made) == 2 and first.closed
        second = recorder.made[1]
        assert second.lps[0].n > first.lps[0].n and second.lps[1].n == first.lps[1].n
        assert [c[:2] for c in second.calls] == [("set_start", 1), ("set_start", 2), ("solve", None)]
        assert second.calls[0][2] is last[1] and second.calls[1][2] is last[2]
        assert batch.cold == [3, 1]
        # close() frees the handle; the next solve builds one and carries on from the last bases
        batch.close()
        assert second.closed
        batch.solve()
        third = recorder.made[2]
        assert [c[:2] for c in third.calls] == [("set_start", 0), ("set_start", 1), ("set_start", 2), ("solve", None)]
        assert batch.rebuilds == 1 and batch.cold == [3, 1, 0]
    assert third.closed
