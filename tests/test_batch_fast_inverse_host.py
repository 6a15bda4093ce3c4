"""Host side of the check of the batched FAST solver's inverse (dzg_debug_batch_fast_inverse): the
hook's ABI and argument checks, the float64 transcription of the documented algorithm
(tests/batch_fast_reference.py) that sets the bound of the GPU tests, and controls that the
criterion at that bound rejects an inverse that is subtly wrong.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

from dantzig_amd import _ffi, core
from tests import batch_fast_reference as bf
from tests import inverse_check as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F6, F7 = "6 batch inverse", "7 batch updates"


# ------------------------------------------------------------------ the hook's host side
def test_header_declares_the_hook_next_to_the_single_lp_one():
    with open(os.path.join(ROOT, "include", "dantzig_amd.h")) as f:
        h = f.read()
    decl = ("int dzg_debug_batch_fast_inverse(const dzg_lp *lps, int64_t count, const dzg_opts *opts, "
            "int64_t pivots,")
    assert decl in h and "int64_t refactor_every, double *w_out, dzg_result *res);" in h
    assert h.index("int dzg_debug_basis_inverse(") < h.index(decl) < h.index("int dzg_debug_cand_reduce(")
    assert "#define DZG_ABI_VERSION 4" in h  # an addition only
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "dzg_debug_batch_fast_inverse" in f.read()


def test_library_exports_the_hook():
    assert "dzg_debug_batch_fast_inverse" in _ffi.EXPORTS
    assert hasattr(_ffi.lib(), "dzg_debug_batch_fast_inverse")


def _lp(m=3, ns=4, seed=0):
    rng = np.random.default_rng(seed)
    return core.CoreLP.from_inequality_form(rng.uniform(-1, 1, (m, ns)), rng.uniform(0, 1, m),
                                            rng.uniform(-1, 1, ns))


def _csc_lp(m=3, ns=4):
    cp = np.arange(ns + 1, dtype=np.int64)
    ri = np.arange(ns, dtype=np.int32) % m
    return core.CoreLP.from_csc(m, cp, ri, np.ones(ns), np.ones(m), np.ones(ns))


def _call(lps, res=True, w=True, pivots=0, refactor_every=0, opts=True, **kw):
    """dzg_debug_batch_fast_inverse on CoreLPs through ctypes; returns (rc, last error)."""
    marshalled = [core._c_lp(lp) for lp in lps]
    arr = (_ffi.Lp * max(len(lps), 1))(*[c for c, _ in marshalled])
    out = (_ffi.Result * max(len(lps), 1))() if res else None
    w_out = np.zeros(sum(lp.m * lp.m for lp in lps) + 1)
    o = _ffi.default_opts(**kw)
    rc = _ffi.lib().dzg_debug_batch_fast_inverse(arr, C.c_int64(len(lps)), C.byref(o) if opts else None,
                                                 C.c_int64(pivots), C.c_int64(refactor_every),
                                                 _ffi.ptr(w_out) if w else None, out)
    return rc, _ffi.lib().dzg_last_error().decode()


@pytest.mark.parametrize("case", ["m129", "csc", "res_null", "w_null", "bad_var_col", "pivots", "refactor_every"])
def test_hook_rejects_malformed_input_on_any_machine(case):
    good = [_lp(seed=1), _lp(seed=2)]
    kw, bad = {}, None
    if case == "m129":
        lps, bad = good + [_lp(m=129, ns=3)], 2
    elif case == "csc":
        lps, bad = [good[0], _csc_lp()], 1
    elif case == "res_null":
        lps, kw = good, dict(res=False)
    elif case == "w_null":
        lps, kw = good, dict(w=False)
    elif case == "pivots":
        lps, kw = good, dict(pivots=-1)
    elif case == "refactor_every":
        lps, kw = good, dict(refactor_every=-1)
    else:
        lp = _lp(seed=3)
        lp.var_col = np.array([0, 1, 2, 99, -1, -2, -3], dtype=np.int64)  # column 99 does not exist
        lps, bad = [good[0], good[1], lp], 2
    rc, msg = _call(lps, numerics=_ffi.FAST, **kw)
    assert rc == _ffi.E_ARG, (rc, msg)
    if bad is not None:
        assert f"lps[{bad}]" in msg
    if case == "w_null":
        assert "w_out" in msg


@pytest.mark.parametrize("numerics", [_ffi.STRICT, _ffi.AUTO, None])
def test_hook_takes_fast_numerics_only(numerics):
    """STRICT keeps no inverse, AUTO (and opts == NULL, which means AUTO) would re-solve in STRICT."""
    if numerics is None:
        rc, msg = _call([_lp(seed=1)], opts=False)
    else:
        rc, msg = _call([_lp(seed=1)], numerics=numerics)
    assert rc == _ffi.E_ARG and "FAST" in msg, (rc, msg)
    with pytest.raises(ValueError, match="FAST"):
        core.debug_batch_fast_inverse([_lp()], 0, numerics=core.STRICT if numerics is None else numerics)


def test_hook_without_a_gpu_is_a_device_error():
    if _ffi.lib().dzg_device_count() > 0:
        pytest.skip("a GPU is visible: the device path is covered by tests/test_gpu_batch_fast_inverse.py")
    rc, msg = _call([_lp(seed=1), _lp(m=0, ns=2, seed=2)], numerics=_ffi.FAST, pivots=3)
    assert rc == _ffi.E_DEVICE and "no CPU path" in msg
    assert _call([], numerics=_ffi.FAST)[0] == 0  # nothing to do is not an error


def test_python_hook_checks_the_whole_batch_before_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was reached")

    lib = _ffi.lib()
    monkeypatch.setattr(_ffi, "lib", lambda: type("L", (), {"dzg_debug_batch_fast_inverse": no_device,
                                                            "dzg_opts_default": lib.dzg_opts_default})())
    good = _lp()
    with pytest.raises(ValueError, match="129 rows"):
        core.debug_batch_fast_inverse([good, _lp(m=129, ns=2)], 1)
    with pytest.raises(ValueError, match="CSC"):
        core.debug_batch_fast_inverse([good, _csc_lp()], 1)
    with pytest.raises(ValueError, match=">= 0"):
        core.debug_batch_fast_inverse([good], -1)
    with pytest.raises(ValueError, match=">= 0"):
        core.debug_batch_fast_inverse([good], 1, refactor_every=-1)
    with pytest.raises(ValueError, match="max_iter"):
        core.debug_batch_fast_inverse([good], 1, max_iter=5)  # `pivots` is the budget


# ------------------------------------------------------------------ the reference and its bound
def _ratio(w, case, basis=None):
    basis = case.lp.basis if basis is None else basis
    return float(ic.residual(w, np.arange(case.m), case.a, basis, case.ns).max())


class _Reference:
    """The transcription on every input of families 1, 2 and 4, computed once."""

    def __init__(self):
        self.f1, self.f2, self.f4 = bf.family1(core), bf.family2(core), bf.family4(core)
        self.fresh = {c.name: bf.invert(c.a, c.lp.basis, c.ns) for c in self.f1 + self.f2}
        self.logs, self.runs = {}, {}
        for c in self.f4:
            self.logs[c.name] = bf.oracle_run(c, max(bf.F4_STOPS_REBUILT)).pivots
            for stops, every in ((bf.F4_STOPS_REBUILT, bf.F4_REFACTOR), (bf.F4_STOPS_PLAIN, 1 << 20)):
                self.runs[c.name, every] = bf.follow(c.a, c.ns, c.lp.basis, self.logs[c.name], stops, every)


@pytest.fixture(scope="module")
def ref():
    return _Reference()


def test_the_reference_is_within_the_bound_and_the_bound_is_ten_times_its_worst(ref):
    """ic.residual over all rows with the default k_eff (the structural basics).  C of a family is 10x
    the worst ratio of the transcription, rounded up: measured here 1.623 (family 1, 31 rows, k = 1;
    family 2 is exact: 0) and 5.782 (family 4, the 32-row slack start after 7 pivots), both far
    below ic.C_MAX, so k_eff stays as it is."""
    worst = {F6: 0.0, F7: 0.0}
    for c in ref.f1 + ref.f2:
        worst[F6] = max(worst[F6], _ratio(ref.fresh[c.name], c))
    for c in ref.f4:
        for every in (bf.F4_REFACTOR, 1 << 20):
            for w, basis in ref.runs[c.name, every].values():
                worst[F7] = max(worst[F7], _ratio(w, c, basis))
    for fam in (F6, F7):
        print(f"float64 transcription, residual / bound, worst of family {fam}: {worst[fam]:.4g} "
              f"(C = {ic.C_INVERSE[fam]})")
        assert ic.C_INVERSE[fam] <= ic.C_MAX
        assert 10 * worst[fam] <= ic.C_INVERSE[fam] <= 1.02 * 10 * worst[fam], (fam, worst[fam])
        assert abs(worst[fam] - ic.C_REFERENCE_OBSERVED[fam]) <= 1e-3 * worst[fam]


def test_exact_families_come_out_exact_and_singular_ones_are_refused(ref):
    for c in ref.f2:
        assert np.array_equal(ref.fresh[c.name], c.exact), c.name
        assert np.array_equal(c.exact @ bf.gather(c.a, c.lp.basis, c.ns), np.eye(c.m)), c.name
    swaps = {c.name: int(np.count_nonzero(bf.eliminate(bf.gather(c.a, c.lp.basis, c.ns))[1] != np.arange(c.m)))
             for c in ref.f2}
    for m in bf.F2_ROWS:
        assert swaps[f"cyclic shift m={m}"] == m - 1 and swaps[f"reversal m={m}"] == m // 2
        assert swaps[f"bidiagonal m={m}"] == 0
    for c in bf.family3(core):
        assert bf.invert(c.a, c.lp.basis, c.ns) is None, c.name
        assert np.linalg.matrix_rank(bf.gather(c.a, c.lp.basis, c.ns)) < c.m, c.name


def test_update_family_has_entering_slacks_and_reaches_its_stops(ref):
    for c in ref.f4:
        log = ref.logs[c.name]
        if c.name.startswith("make_lp"):
            assert any(e >= c.ns for _, e, _, _ in log), f"{c.name}: no slack enters"
    long_runs = [c for c in ref.f4 if len(ref.logs[c.name]) >= max(bf.F4_STOPS_REBUILT)]
    assert {c.m for c in long_runs} >= {32, 33, 64, 65, 128}


# ------------------------------------------------------------------ the criterion bites at C
def test_criterion_rejects_one_entry_off_by_1e_9(ref):
    hit = 0
    for c in ref.f1:
        w = ref.fresh[c.name]
        bad = w.copy()
        p, r = np.unravel_index(np.argmax(np.abs(w)), w.shape)
        bad[p, r] *= 1.0 + 1e-9
        assert _ratio(w, c) <= ic.C_INVERSE[F6]
        hit += _ratio(bad, c) > ic.C_INVERSE[F6]
    assert hit == len(ref.f1)  # 1e-9 is 9e6 units of 2^-53: no input hides it


def test_criterion_rejects_swaps_undone_first_to_last(ref):
    hit = tried = 0
    for c in ref.f1 + ref.f2:
        w0, piv = bf.eliminate(bf.gather(c.a, c.lp.basis, c.ns))
        wrong = bf.undo_swaps(w0, piv, last_first=False)
        if np.array_equal(wrong, ref.fresh[c.name]):
            continue  # no two swaps share a row: the order does not matter
        tried += 1
        hit += _ratio(wrong, c) > ic.C_INVERSE[F6]
    assert tried >= 20 and hit == tried
    cyc = next(c for c in ref.f2 if c.name == "cyclic shift m=17")  # every swap shares a row with the next
    w0, piv = bf.eliminate(bf.gather(cyc.a, cyc.lp.basis, cyc.ns))
    assert _ratio(bf.undo_swaps(w0, piv, last_first=False), cyc) > ic.C_INVERSE[F6]


def test_criterion_rejects_the_inverse_of_the_basis_one_pivot_earlier(ref):
    hit = 0
    for c in ref.f4:
        run = ref.runs[c.name, 1 << 20]
        if 1 not in run or 2 not in run:
            continue
        (w1, _), (w2, basis2) = run[1], run[2]
        assert _ratio(w2, c, basis2) <= ic.C_INVERSE[F7]
        assert _ratio(w1, c, basis2) > ic.C_INVERSE[F7], c.name
        hit += 1
    assert hit >= len(ref.f4) - 2
