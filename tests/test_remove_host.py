"""Rows and columns removed from a live LP (dzg_solver_remove, core.Solver.remove, core.reduced_lp,
Session.remove_constraints), the parts that need no GPU: the entry point and its mirror, the numbering
rule and the refusals on the host, the claim that the removal is free (x and z of the survivors are
unchanged) on the CPU oracle at the bases the GPU tests use, and the session's bookkeeping against a
stand-in for core.Solver."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import _ffi, core
from oracle import oracle as ora
from tests import duals_reference as dref
from tests import extend_check as ec
from tests import remove_check as rmc
from tests import state_check as sc
from tests.test_reopt_host import _form, _kat
from tests.test_surface import build_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the C entry point
def test_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "dantzig_amd.h")).read()
    assert ("int dzg_solver_remove(dzg_solver *s, const dzg_remove *rem, int64_t *var_map, "
            "int64_t *row_map);") in text
    assert "#define DZG_ABI_VERSION 4" in text
    assert "dzg_solver_remove" in _ffi.EXPORTS and hasattr(_ffi.lib(), "dzg_solver_remove")
    assert _ffi.lib().dzg_abi_version() == 4
    assert len(_ffi.KERNEL_CLASSES) == 10          # (the gather has no timer class of its own)


def test_mirror_layout_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dantzig_amd.h"', 'int main(void) {',
             'printf("dzg_remove %zu\\n", sizeof(dzg_remove));']
    for field, _ in _ffi.Remove._fields_:
        lines.append(f'printf("dzg_remove.{field} %zu\\n", offsetof(dzg_remove, {field}));')
    lines += ['return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["dzg_remove"]) == C.sizeof(_ffi.Remove) == 32
    assert [f for f, _ in _ffi.Remove._fields_] == ["n_rows", "rows", "n_cols", "cols"]
    for field, _ in _ffi.Remove._fields_:
        assert int(got[f"dzg_remove.{field}"]) == getattr(_ffi.Remove, field).offset, field


def test_null_arguments_are_argument_errors_on_the_host():
    lib = _ffi.lib()
    one = np.zeros(1, np.int64)
    rem = _ffi.Remove(1, _ffi.ptr(one), 0, None)
    assert lib.dzg_solver_remove(None, C.byref(rem), None, None) == _ffi.E_ARG
    assert b"NULL" in lib.dzg_last_error()
    assert lib.dzg_solver_remove(None, None, None, None) == _ffi.E_ARG
    with pytest.raises(_ffi.DantzigAmdError):
        _ffi.check_extend(lib.dzg_solver_remove(None, None, None, None), "dzg_solver_remove")


def test_check_extend_maps_the_unsupported_route_of_remove():
    class _Lib:
        @staticmethod
        def dzg_last_error():
            return b"remove is not supported on CSC storage or sharded solvers"

        @staticmethod
        def dzg_status_str(code):
            return b"invalid_argument"
    real = _ffi._lib
    _ffi.lib()
    try:
        _ffi._lib = _Lib()
        with pytest.raises(NotImplementedError, match="remove is not supported"):
            _ffi.check_extend(_ffi.E_ARG, "dzg_solver_remove")
    finally:
        _ffi._lib = real


def test_solver_has_remove_and_removable_with_docstrings():
    assert "dzg_solver_remove" in core.Solver.remove.__doc__
    assert "basic" in core.Solver.removable.__doc__


# ------------------------------------------------------------------ the numbering rule, on the host
def _same_lp(got: core.CoreLP, want: core.CoreLP, what):
    assert (got.m, got.n, got.n_struct) == (want.m, want.n, want.n_struct), what
    for name in ("a", "c", "basis", "nonbasis", "x", "z", "var_col"):
        g, w = np.ascontiguousarray(getattr(got, name)), np.ascontiguousarray(getattr(want, name))
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)
    assert got.constant == want.constant and got.xbar is None and got.zbar is None, what
    assert got.col_ptr is None and got.block is None, what


@pytest.mark.parametrize("p,r,s", ec.RECIPE, ids=[f"+{p}+{r}" for p, r, _ in ec.RECIPE])
def test_reduced_lp_undoes_extended_lp(p, r, s):
    a, b, c = ec.base(31, 24, 40)
    m, ns = a.shape
    plain = core.CoreLP.from_inequality_form(a, b, c, constant=0.25)
    lp = core.CoreLP(a=a, c=plain.c, basis=plain.basis, nonbasis=plain.nonbasis, x=plain.x, z=plain.z,
                     var_col=ec.codes_of(plain), constant=0.25)          # an explicit var_col
    rng = np.random.default_rng(s)
    kw = ec.draw(lp, rng.random(ns), rng.random(m), p, r, s)
    ext = core.extended_lp(lp, **kw)
    back, var_map, row_map = core.reduced_lp(ext, rows=list(range(m, m + p)), cols=list(range(ns, ns + r)))
    _same_lp(back, lp, (p, r, s))
    n = lp.n
    assert var_map.tolist() == list(range(n)) + [-1] * (p + r)
    assert row_map.tolist() == list(range(m)) + [-1] * p
    # the benchmark convention comes back with its var_col written out
    back2, _, _ = core.reduced_lp(core.extended_lp(plain, **kw), rows=list(range(m, m + p)),
                                  cols=list(range(ns, ns + r)))
    _same_lp(back2, lp, (p, r, s, "benchmark convention"))


def _hand_lp():
    """3 x 4, variables 0..3 structural on columns 0..3, 4..6 the slacks of rows 0..2; the basis holds
    column 2 at position 0, the slack of row 2 at position 1 and column 0 at position 2."""
    a = np.array([[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0], [9.0, 10.0, 11.0, 12.0]])
    return core.CoreLP(a=a, c=np.array([1.0, 2.0, 3.0, 4.0, 0.0, 0.0, 0.0]), basis=np.array([2, 6, 0]),
                       nonbasis=np.array([5, 3, 1, 4]), x=np.array([0.1, 0.2, 0.3]),
                       z=np.array([0.4, 0.5, 0.6, 0.7]), var_col=np.array([0, 1, 2, 3, -1, -2, -3]),
                       constant=2.0)


def test_the_compression_rule_on_a_hand_written_lp():
    lp = _hand_lp()
    got, var_map, row_map = core.reduced_lp(lp, rows=[2], cols=[1])
    # row 2 goes with variable 6, column 1 with variable 1; survivors ascending
    assert var_map.tolist() == [0, -1, 1, 2, 3, 4, -1] and row_map.tolist() == [0, 1, -1]
    assert got.a.tolist() == [[1.0, 3.0, 4.0], [5.0, 7.0, 8.0]]
    assert got.var_col.tolist() == [0, 1, 2, -1, -2]
    assert got.c.tolist() == [1.0, 3.0, 4.0, 0.0, 0.0]
    assert got.basis.tolist() == [1, 0] and got.x.tolist() == [0.1, 0.3]          # positions 0 and 2, in order
    assert got.nonbasis.tolist() == [4, 2, 3] and got.z.tolist() == [0.4, 0.5, 0.7]
    assert (got.m, got.n, got.n_struct, got.constant) == (2, 5, 3, 2.0)
    # a column in the middle only: the slacks keep their rows, the later columns move up
    got, var_map, row_map = core.reduced_lp(lp, cols=[3])
    assert var_map.tolist() == [0, 1, 2, -1, 3, 4, 5] and row_map.tolist() == [0, 1, 2]
    assert got.var_col.tolist() == [0, 1, 2, -1, -2, -3] and got.basis.tolist() == [2, 5, 0]
    assert got.nonbasis.tolist() == [4, 1, 3] and got.z.tolist() == [0.4, 0.6, 0.7]
    # slacks numbered before the structural variables: the rule is by old index, whatever the kind
    perm = np.array([4, 5, 6, 0, 1, 2, 3])                 # new variable -> old variable
    inv = np.argsort(perm)
    lp2 = core.CoreLP(a=lp.a, c=lp.c[perm], basis=inv[lp.basis], nonbasis=inv[lp.nonbasis], x=lp.x, z=lp.z,
                      var_col=lp.var_col[perm])
    got, var_map, row_map = core.reduced_lp(lp2, rows=[2], cols=[1])
    assert lp2.var_col.tolist() == [-1, -2, -3, 0, 1, 2, 3]
    assert var_map.tolist() == [0, 1, -1, 2, -1, 3, 4] and got.var_col.tolist() == [-1, -2, 0, 1, 2]
    assert got.basis.tolist() == [3, 2] and got.nonbasis.tolist() == [1, 4, 0]


def test_every_refusal_is_a_value_error():
    lp = _hand_lp()
    for kw, match in [(dict(rows=[0]), "row 0 is binding"),            # slack 4 is nonbasic
                      (dict(rows=[2, 1]), "row 1 is binding"),
                      (dict(cols=[2]), "column 2 is basic"),
                      (dict(cols=[1, 0]), "column 0 is basic"),
                      (dict(rows=[2, 2]), "listed twice"),
                      (dict(cols=[1, 3, 1]), "listed twice"),
                      (dict(rows=[3]), "out of range"),
                      (dict(rows=[-1]), "out of range"),
                      (dict(cols=[4]), "out of range"),
                      (dict(), "give rows or cols"),
                      (dict(rows=[], cols=[]), "give rows or cols"),
                      (dict(rows=[0, 1, 2]), "must stay"),
                      (dict(cols=[0, 1, 2, 3]), "must stay"),
                      (dict(rows=[0.5]), "integer")]:
        with pytest.raises(ValueError, match=match):
            core.reduced_lp(lp, **kw)
    s = core.Solver.__new__(core.Solver)   # a stub: the lists are checked before the handle is touched
    s._lp, s._h = lp, None
    for kw in (dict(), dict(rows=[3]), dict(cols=[1, 1]), dict(rows=[0, 1, 2])):
        with pytest.raises(ValueError, match="remove"):
            s.remove(**kw)
    assert s._lp is lp
    col_ptr, row_idx, val, bs, cs = core.gen_sparse_lp(seed=3, m=8, n_struct=12, per_col=2)
    csc = core.CoreLP.from_csc(8, col_ptr, row_idx, val, bs, cs)
    with pytest.raises(NotImplementedError, match="remove is not supported"):
        core.reduced_lp(csc, rows=[0])
    s._lp = csc
    with pytest.raises(NotImplementedError, match="remove is not supported"):
        s.remove(rows=[0])
    with pytest.raises(NotImplementedError, match="remove is not supported"):
        s.removable()


# ------------------------------------------------------------------ the removal is free, on the CPU oracle
@pytest.mark.parametrize("seed,m,ns", ec.BASES[:2], ids=["24x40", "37x53"])
def test_what_is_free_leaves_x_and_z_of_the_survivors_unchanged(seed, m, ns):
    a, b, c = ec.base(seed, m, ns)
    lp = core.CoreLP.from_inequality_form(a, b, c)
    res = ora.simplex_solve(sc.stdform(a, ns, lp.c, lp))
    assert res.status == "optimal"
    opt = rmc.at_basis(lp, res)
    row_mask, col_mask = rmc.free_masks(opt)
    rows, cols = rmc.free_sets(opt)
    want_rows, want_cols = rmc.FREE_AT_LEAST[(seed, m, ns)]
    assert row_mask.sum() >= want_rows and col_mask.sum() >= want_cols, (row_mask.sum(), col_mask.sum())
    assert len(rows) == row_mask.sum() and len(cols) == (col_mask.sum() + 1) // 2
    red, var_map, row_map = core.reduced_lp(opt, rows=rows, cols=cols)
    assert (red.m, red.n_struct) == (m - len(rows), ns - len(cols))
    # x = B'^-1 b' and z = N'^T B'^-T c_B' - c_N' on the reduced basis, as the device recomputes them
    codes = ec.codes_of(red)
    x2 = ora.lu_solve(sc.columns(red.a, red.m, codes[red.basis]), b[row_map >= 0])
    sf = sc.stdform(red.a, red.n_struct, red.c, red, red.var_col)
    z2 = dref.core_duals(sf, red).d[red.nonbasis]
    x_keep = np.asarray(res.x)[var_map[np.asarray(res.basis)] >= 0]
    z_keep = np.asarray(res.z)[var_map[np.asarray(res.nonbasis)] >= 0]
    print(f"{m}x{ns}: {len(rows)} rows and {len(cols)} columns go; |dx| {np.abs(x2 - x_keep).max():.2e}, "
          f"|dz| {np.abs(z2 - z_keep).max():.2e}, min x {x2.min():.3e}, min z {z2.min():.3e}")
    assert np.abs(x2 - x_keep).max() <= 1e-12 and np.abs(z2 - z_keep).max() <= 1e-12
    assert x2.min() > 1e-6 and z2.min() > 1e-6        # so a continuation takes no pivot


# ------------------------------------------------------------------ the session, without a device
class _FakeSolver:
    """What Session uses of core.Solver, on the host: every added row's slack is basic unless its
    row index is listed in `binding`."""
    made = []
    binding = set()

    def __init__(self, lp, **opts):
        self.lp, self.calls, self.closed = lp, [], False
        self.m, self.ns = lp.m, lp.n_struct
        _FakeSolver.made.append(self)

    def extend(self, rows=None, rhs=None, **kw):
        self.calls.append(("extend", len(rhs)))
        self.m += len(rhs)

    def removable(self):
        mask = np.ones(self.m, bool)
        mask[[r for r in _FakeSolver.binding if r < self.m]] = False
        return mask, np.zeros(self.ns, bool)

    def remove(self, rows=None, cols=None):
        self.calls.append(("remove", list(rows)))
        self.m -= len(rows)

    def reoptimize(self, b=None, c=None, constant=None):
        assert len(b) == self.m
        self.calls.append(("reoptimize", len(b)))

    def run(self, k):
        return "optimal"

    def result(self, log=True):
        return types.SimpleNamespace(status="optimal", status_code=_ffi.OPTIMAL, iterations=0, objective=0.0,
                                     numerics="strict", basis=np.arange(self.m), x=np.zeros(self.m))

    def dims(self):
        return self.m, self.m + self.ns, self.ns

    def close(self):
        self.closed = True


@pytest.fixture
def fake_solver(monkeypatch):
    _FakeSolver.made, _FakeSolver.binding = [], set()
    monkeypatch.setattr(core, "Solver", _FakeSolver)
    return _FakeSolver


def _model():
    x, y = dz.Variable.nonneg(), dz.Variable.nonneg()
    first, second = x + 2 * y <= 4, x <= 3
    return x, y, first, second, dz.Maximize(x + y).subject_to([first, second])


def test_session_removal_before_the_first_solve(fake_solver):
    x, y, first, second, problem = _model()
    session = problem.session()
    extra = x - y <= 1
    session.add_constraints(extra)
    session._change(None, {extra: 2.0})
    assert session.remove_constraints(extra) is session
    assert session._constraints == [first, second] and id(extra) not in session._rhs
    session.remove_constraints([second])
    assert session._constraints == [first] and session.rebuilds == 0 and fake_solver.made == []
    session.solve()
    assert fake_solver.made[0].lp.m == _form(problem).m - 1 and session.rebuilds == 0      # without `second`
    session.add_constraints(second)                         # a removed constraint may come back
    session.solve()
    assert fake_solver.made[0].calls[0] == ("extend", 1)


def test_session_key_and_type_errors(fake_solver):
    x, y, first, second, problem = _model()
    for live in (False, True):
        session = problem.session()
        if live:
            session.solve()
        with pytest.raises(KeyError):
            session.remove_constraints(x - y <= 1)
        with pytest.raises(KeyError):
            session.remove_constraints([first, x - y <= 1])             # all or nothing
        with pytest.raises(KeyError):
            session.remove_constraints([first, first])
        with pytest.raises(TypeError):
            session.remove_constraints("x <= 1")
        with pytest.raises(TypeError):
            session.remove_constraints([first, "x <= 1"])
        assert session._constraints == [first, second] and session._removed == []
        session.remove_constraints(first)
        with pytest.raises(KeyError):
            session.remove_constraints(first)                           # it is gone already
        session.close()


def test_session_fast_path_and_rebuild_decision(fake_solver):
    x, y, first, second, problem = _model()
    session = problem.session()
    session.solve()
    live = fake_solver.made[0]
    m0 = live.m
    cut1, cut2, eq = x - y <= 1, x + y <= 10, x == 2 * y         # eq lowers to two rows
    session.add_constraints([cut1, eq, cut2])
    session.solve()
    assert live.calls[-2:] == [("extend", 4), ("reoptimize", m0 + 4)] and live.m == m0 + 4
    # slack constraints the session added leave the live solver: no rebuild, the rows below the form's
    session.remove_constraints(eq)
    session.solve()
    assert live.calls[-2:] == [("remove", [m0 + 1, m0 + 2]), ("reoptimize", m0 + 2)]
    assert session.rebuilds == 0 and session._added == [cut1, cut2] and session._extended == 2
    assert not live.closed and fake_solver.made == [live]
    with pytest.raises(KeyError):
        session.solve(rhs={eq: 1.0})                                       # it is not held any more
    # added again it is extended again, below the others
    session.add_constraints(eq)
    session.solve()
    assert live.calls[-2:] == [("extend", 2), ("reoptimize", m0 + 4)] and session._added == [cut1, cut2, eq]
    # a binding one: the solver goes, the model is lowered without it, `rebuilds` counts
    fake_solver.binding = {m0 + 3}                                         # eq's second row
    session.remove_constraints([cut1, eq])
    session.solve()
    assert session.rebuilds == 1 and live.closed and len(fake_solver.made) == 2
    assert not any(call[0] == "remove" for call in live.calls[-2:])
    assert session._constraints == [first, second, cut2] and session._added == []
    assert fake_solver.made[1].lp.m == m0 + 1
    # an original constraint of the model: always a rebuild
    fake_solver.binding = set()
    session.remove_constraints(second)
    session.solve()
    assert session.rebuilds == 2 and len(fake_solver.made) == 3 and fake_solver.made[2].lp.m == m0
    assert session._constraints == [first, cut2]
    # removed and added again between two solves: the removal is called off, nothing moves
    session.remove_constraints(cut2)
    session.add_constraints(cut2)
    session.solve()
    assert session.rebuilds == 2 and len(fake_solver.made) == 3 and session._constraints == [first, cut2]
    # one that was added but has not reached the solver yet just leaves the list
    cut3 = y <= 7
    session.add_constraints(cut3)
    session.remove_constraints(cut3)
    session.solve()
    assert session.rebuilds == 2 and fake_solver.made[2].calls[-1] == ("reoptimize", m0)
    assert len(session.pivots) == 8


@pytest.mark.parametrize("name", sorted(rmc.LOOSENED))
def test_the_loosened_constraints_are_slack_at_the_optimum(name):
    k = _kat(name)
    ns, problem = build_problem(k)
    f = _form(problem)
    lp = core.CoreLP(a=f.a, c=f.c, basis=f.basis, nonbasis=f.nonbasis, x=f.x, z=f.z, var_col=f.var_col,
                     constant=f.constant)
    status, _, x_star, _ = ec.highs(lp)
    assert status == 0
    session = problem.session()
    order = session._lowered()[2]
    for text, slack_at_least in ((rmc.LOOSENED[name], 0.1), (ec.ADDED[name][0], None)):
        con = eval(text, {"__builtins__": {}}, dict(ns))
        for row, b in session._rows_of(con, f, order):
            if slack_at_least is None:
                assert row @ x_star > b + 1e-6, (name, text)                # the original one is violated
            else:
                assert b - row @ x_star >= slack_at_least, (name, text, b - row @ x_star)
