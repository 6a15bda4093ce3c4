"""Host-side Python view of the Level-1 C ABI (include/dantzig_amd.h).

`CoreLP` carries the state Simplex::new leaves behind (src/simplex.rs:209-223) and `Solver`
replaces Simplex::solve (src/simplex.rs:332-343) with the HIP engine.  Everything here is
plumbing over ctypes; the arithmetic lives in dantzig_amd/csrc/*.hip.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _ffi
from ._ffi import (AUTO, FAST, STRICT, PRICE_AUTO, PRICE_SEQ, PRICE_WAVE, PRICE_TREE,  # noqa: F401
                   STEP_DUAL,
                   STEP_PRIMAL, NEAR_TIE_COUNT, NEAR_TIE_STOP, DantzigAmdError, f64, i64, ptr)

STATUS_NAMES = {0: "optimal", 1: "unbounded", 2: "infeasible", 3: "iter_limit", 4: "singular",
                5: "panic", 6: "running", 7: "near_tie"}


@dataclass
class CoreLP:
    """maximise c.x + constant  s.t.  [A | slacks] x = rhs, x >= 0, in Simplex::new's layout."""
    a: np.ndarray | None          # (m, n_struct) any layout; uploaded column-major.  None: CSC
    c: np.ndarray                 # n
    basis: np.ndarray             # m
    nonbasis: np.ndarray          # n - m
    x: np.ndarray                 # m
    z: np.ndarray                 # n - m
    var_col: np.ndarray | None = None
    constant: float = 0.0
    # sparse structural block (used when a is None): CSC, rows ascending inside a column
    col_ptr: np.ndarray | None = None
    row_idx: np.ndarray | None = None
    val: np.ndarray | None = None
    # column sharding: `a` holds only the structural columns [block[0], block[1]) of an LP with
    # n_struct_full structural columns (opts.a_is_block); everything else is complete
    block: tuple | None = None
    n_struct_full: int | None = None
    # perturbation vectors (Simplex.x_bar / z_bar); None = ones (Simplex::new).  With a non-slack
    # basis, its x and z: resume a solve from a CoreResult (CoreLP.resumed_from)
    xbar: np.ndarray | None = None
    zbar: np.ndarray | None = None

    @property
    def m(self) -> int:
        return int(self.a.shape[0]) if self.a is not None else len(self.basis)

    @property
    def n_struct(self) -> int:
        if self.n_struct_full is not None:
            return int(self.n_struct_full)
        return int(self.a.shape[1]) if self.a is not None else len(self.col_ptr) - 1

    @property
    def n(self) -> int:
        return len(self.c)

    @classmethod
    def from_inequality_form(cls, a, b, c, constant: float = 0.0) -> "CoreLP":
        """max c.x st A x <= b, x >= 0 in the benchmark convention of SURVEY 8(d): variables
        0..ns-1 structural, ns..ns+m-1 slacks, slack basis, x = b, z = -c."""
        a = np.asarray(a, dtype=np.float64)
        m, ns = a.shape
        return cls(a=a, c=np.concatenate([f64(c), np.zeros(m)]),
                   basis=np.arange(ns, ns + m, dtype=np.int64),
                   nonbasis=np.arange(ns, dtype=np.int64), x=f64(b).copy(), z=-f64(c),
                   var_col=None, constant=constant)

    @classmethod
    def from_inequality_block(cls, a_block, b, c, begin: int, end: int,
                              constant: float = 0.0) -> "CoreLP":
        """One rank's view of from_inequality_form: `a_block` = columns [begin, end) of A."""
        a_block = np.asarray(a_block, dtype=np.float64)
        m, ns = a_block.shape[0], len(c)
        if a_block.shape[1] != end - begin or not 0 <= begin <= end <= ns:
            raise ValueError("a_block does not match [begin, end)")
        return cls(a=a_block, c=np.concatenate([f64(c), np.zeros(m)]),
                   basis=np.arange(ns, ns + m, dtype=np.int64),
                   nonbasis=np.arange(ns, dtype=np.int64), x=f64(b).copy(), z=-f64(c),
                   var_col=None, constant=constant, block=(int(begin), int(end)),
                   n_struct_full=ns)

    @classmethod
    def from_csc(cls, m, col_ptr, row_idx, val, b, c, constant: float = 0.0) -> "CoreLP":
        """Same convention with the structural block in CSC (kept sparse on the device)."""
        ns = len(col_ptr) - 1
        return cls(a=None, c=np.concatenate([f64(c), np.zeros(m)]),
                   basis=np.arange(ns, ns + m, dtype=np.int64),
                   nonbasis=np.arange(ns, dtype=np.int64), x=f64(b).copy(), z=-f64(c),
                   constant=constant, col_ptr=i64(col_ptr),
                   row_idx=np.ascontiguousarray(row_idx, dtype=np.int32), val=f64(val))


def warm_started(lp: CoreLP, k: int) -> CoreLP:
    """The same LP started from the basis "first k structural columns in the place of the first k
    slacks" (x = 1, z = -1: any state will do for a benchmark -- the engine factorises the basis and
    pivots from there).  How the deep regimes of a solve -- a compact inverse k columns wide -- are
    reached without running the hundreds of thousands of pivots that lead there (bench.py,
    tests/test_gpu_fullsize.py); works on whole and on column-block LPs of the benchmark convention."""
    import dataclasses

    m, ns = lp.m, lp.n_struct
    if lp.var_col is not None or not 0 <= k <= min(m, ns):
        raise ValueError("warm_started: benchmark-convention LP and 0 <= k <= min(m, n_struct)")
    basis = np.concatenate([np.arange(k), ns + np.arange(k, m)]).astype(np.int64)
    nonbasis = np.concatenate([np.arange(k, ns), ns + np.arange(k)]).astype(np.int64)
    return dataclasses.replace(lp, basis=basis, nonbasis=nonbasis, x=np.ones(m), z=-np.ones(ns),
                               xbar=None, zbar=None)


def resumed_from(lp: CoreLP, r) -> CoreLP:
    """The same LP in the state a CoreResult (or anything with basis, nonbasis, x, xbar, z, zbar)
    left it in: a solver created on it factorises that basis and carries the solve on."""
    import dataclasses

    def get(name):  # a CoreResult, or a mapping such as an .npz archive of one
        return r[name] if hasattr(r, "keys") else getattr(r, name)
    return dataclasses.replace(lp, basis=i64(get("basis")).copy(), nonbasis=i64(get("nonbasis")).copy(),
                               x=f64(get("x")).copy(), z=f64(get("z")).copy(),
                               xbar=f64(get("xbar")).copy(), zbar=f64(get("zbar")).copy())


def _extend_blocks(m: int, ns: int, rows, rhs, cols, c_cols):
    """The four arrays of an extension as float64 (p, ns), (p,), (m + p, r), (r,); ValueError for a
    wrong shape, a half-given pair or when nothing is given."""
    if (rows is None) != (rhs is None):
        raise ValueError("extend: rows and rhs go together")
    if (cols is None) != (c_cols is None):
        raise ValueError("extend: cols and c_cols go together")
    rhs = np.zeros(0) if rhs is None else np.atleast_1d(f64(rhs))
    c_cols = np.zeros(0) if c_cols is None else np.atleast_1d(f64(c_cols))
    if rhs.ndim != 1 or c_cols.ndim != 1:
        raise ValueError("extend: rhs and c_cols are vectors")
    p, r = len(rhs), len(c_cols)
    if p == 0 and r == 0:
        raise ValueError("extend: give rows and rhs, or cols and c_cols")
    rows = np.zeros((0, ns)) if rows is None else f64(rows)
    cols = np.zeros((m + p, 0)) if cols is None else f64(cols)
    if rows.shape != (p, ns):
        raise ValueError(f"extend: rows has shape {rows.shape}, expected {(p, ns)}")
    if cols.shape != (m + p, r):
        raise ValueError(f"extend: cols has shape {cols.shape}, expected {(m + p, r)} "
                         "(the new columns over all rows, the new ones included)")
    return rows, rhs, cols, c_cols


def extended_lp(lp: CoreLP, rows=None, rhs=None, cols=None, c_cols=None) -> CoreLP:
    """Host only: the LP a handle created on `lp` holds after Solver.extend with the same arguments
    (dzg_solver_extend).  rows (p, n_struct) / rhs (p,): new constraints on the existing structural
    columns; cols (m + p, r) / c_cols (r,): new structural columns over all rows, the new ones
    included.  No existing index changes: the new structural variables are n .. n+r-1 on the columns
    n_struct .. n_struct+r-1, the slacks of the new rows n+r .. n+r+p-1 on the rows m .. m+p-1; var_col
    is explicit.  Basis positions 0 .. m-1 and nonbasic positions 0 .. q-1 keep lp's variables, the new
    slacks follow in the basis and the new structural variables in the nonbasis, x = [lp.x, rhs] and
    z = [lp.z, -c_cols]: for an `lp` in its slack start, the slack start of the extended LP.  -0.0
    entries of the new blocks are +0.0 in `a`, as on the device."""
    import dataclasses

    if lp.a is None or lp.block is not None:
        raise NotImplementedError("extend is not supported on CSC storage or sharded solvers")
    m, ns, n = lp.m, lp.n_struct, lp.n
    rows, rhs, cols, c_cols = _extend_blocks(m, ns, rows, rhs, cols, c_cols)
    p, r = len(rhs), len(c_cols)
    a = np.zeros((m + p, ns + r))
    a[:m, :ns] = np.asarray(lp.a, dtype=np.float64)
    a[m:, :ns] = rows + 0.0   # (-0.0 + 0.0 = +0.0)
    a[:, ns:] = cols + 0.0
    var_col = (i64(lp.var_col) if lp.var_col is not None
               else np.concatenate([np.arange(ns), -1 - np.arange(n - ns)]).astype(np.int64))
    var_col = np.concatenate([var_col, ns + np.arange(r), -1 - (m + np.arange(p))]).astype(np.int64)
    return dataclasses.replace(
        lp, a=a, c=np.concatenate([f64(lp.c), c_cols, np.zeros(p)]), var_col=var_col,
        basis=np.concatenate([i64(lp.basis), n + r + np.arange(p)]).astype(np.int64),
        nonbasis=np.concatenate([i64(lp.nonbasis), n + np.arange(r)]).astype(np.int64),
        x=np.concatenate([f64(lp.x), rhs]), z=np.concatenate([f64(lp.z), -c_cols]),
        xbar=None, zbar=None)


def _remove_lists(m: int, ns: int, rows, cols):
    """The two lists of a removal as boolean masks over [0, m) and [0, n_struct); ValueError for an
    index out of range or listed twice, when nothing is given, and when no row or no column would stay."""
    masks = []
    for name, idx, size in (("rows", rows, m), ("cols", cols, ns)):
        idx = np.zeros(0, np.int64) if idx is None else np.atleast_1d(np.asarray(idx))
        if idx.ndim != 1 or (idx.size and idx.dtype.kind not in "iu"):
            raise ValueError(f"remove: {name} is a list of integer indices")
        idx = idx.astype(np.int64)
        if ((idx < 0) | (idx >= size)).any():
            raise ValueError(f"remove: an index of {name} is out of range [0, {size})")
        if len(np.unique(idx)) != len(idx):
            raise ValueError(f"remove: an index of {name} is listed twice")
        mask = np.zeros(size, bool)
        mask[idx] = True
        masks.append(mask)
    if not masks[0].any() and not masks[1].any():
        raise ValueError("remove: give rows or cols")
    if masks[0].all() or masks[1].all():
        raise ValueError("remove: at least one row and one structural column must stay")
    return masks


def _codes(lp: CoreLP) -> np.ndarray:
    """The column code of every variable: >= 0 a structural column, -1 - r the slack of row r."""
    if lp.var_col is not None:
        return i64(lp.var_col)
    return np.concatenate([np.arange(lp.n_struct), -1 - np.arange(lp.n - lp.n_struct)]).astype(np.int64)


def reduced_lp(lp: CoreLP, rows=None, cols=None):
    """Host only: (the LP a handle that stands at `lp`'s basis holds after Solver.remove with the same
    arguments, var_map, row_map) (dzg_solver_remove).  rows: constraint rows to drop, with their
    slacks; cols: structural columns to drop, with their variables.  Only what is free may go, judged
    by lp.basis: a row whose slack is basic, a column whose variable is nonbasic; ValueError otherwise,
    and for everything else the C call refuses.  Survivors are compressed in ascending order of their
    old index -- variables, rows and columns alike; var_col is explicit and rewritten to match
    (structural: the new column, slack: -1 - new row); surviving basis and nonbasic positions keep
    their relative order, x and z their entries.  var_map (n) and row_map (m) hold the new index, or
    -1 for what was dropped.  The inverse of extended_lp: reduced_lp(extended_lp(lp, ...), its rows,
    its columns) is `lp` (with var_col explicit) where the new slacks are still basic and the new
    variables nonbasic."""
    import dataclasses

    if lp.a is None or lp.block is not None:
        raise NotImplementedError("remove is not supported on CSC storage or sharded solvers")
    m, ns, n = lp.m, lp.n_struct, lp.n
    drop_row, drop_col = _remove_lists(m, ns, rows, cols)
    codes = _codes(lp)
    basis, nonbasis = i64(lp.basis), i64(lp.nonbasis)
    cn, cb = codes[nonbasis], codes[basis]
    bound = nonbasis[(cn < 0) & drop_row[np.maximum(-1 - cn, 0)]]
    if len(bound):
        raise ValueError(f"remove: row {-1 - codes[bound[0]]} is binding (its slack, variable {bound[0]}, "
                         "is nonbasic)")
    held = basis[(cb >= 0) & drop_col[np.maximum(cb, 0)]]
    if len(held):
        raise ValueError(f"remove: column {codes[held[0]]} is basic (variable {held[0]})")
    row_map = np.where(drop_row, -1, np.cumsum(~drop_row) - 1).astype(np.int64)
    col_map = np.where(drop_col, -1, np.cumsum(~drop_col) - 1).astype(np.int64)
    to = np.where(codes >= 0, col_map[np.maximum(codes, 0)], row_map[np.maximum(-1 - codes, 0)])
    keep = to >= 0
    var_map = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)
    kb, kn = keep[basis], keep[nonbasis]
    a = np.asarray(lp.a, dtype=np.float64)
    if drop_row.any():          # (one axis at a time, and only where something goes: whole rows copy fast)
        a = a[~drop_row]
    if drop_col.any():
        a = a[:, ~drop_col]
    a = np.ascontiguousarray(a)
    out = dataclasses.replace(
        lp, a=a, c=f64(lp.c)[keep].copy(),
        var_col=np.where(codes >= 0, to, -1 - to)[keep].astype(np.int64),
        basis=var_map[basis[kb]], nonbasis=var_map[nonbasis[kn]],
        x=f64(lp.x)[kb].copy(), z=f64(lp.z)[kn].copy(), xbar=None, zbar=None)
    return out, var_map, row_map


@dataclass
class CoreResult:
    status: str
    status_code: int
    numerics: str
    iterations: int
    objective: float
    basis: np.ndarray
    nonbasis: np.ndarray
    x: np.ndarray
    xbar: np.ndarray
    z: np.ndarray
    zbar: np.ndarray
    pivots: list = field(default_factory=list)   # (kind, entering, leaving, mu)
    kernel_ms: dict = field(default_factory=dict)
    kernel_launches: dict = field(default_factory=dict)
    price_bytes: float = 0.0
    solve_ms: float = 0.0
    max_pivot_error: float = 0.0
    # FAST near-tie arbitration: the pivot log is certified to be the reference's up to (not
    # including) pivot first_near_tie; near_ties == 0: all of it
    near_ties: int = 0
    first_near_tie: int = -1
    min_margin: float = float("inf")
    margins: np.ndarray | None = None   # per-pivot smallest decision margin (log=True)
    dense_columns: int = 0              # k: structural basics = dense columns of the inverse
    refactors: int = 0
    chain_fallbacks: int = 0            # failed device-wide barriers recovered from (k_chain.hip)
    price_pass_used: int = 0            # bit mask: 1 row-wise pricing pass ran, 2 column-wise
    price_rows_copy: int = 0            # 1: the row-major copy of the matrix is resident
    state_drift: float = 0.0            # carried x, xbar, z, zbar vs the fresh inverse at the last refactorisation
    duals: "CoreDuals | None" = None    # solve_batch(duals=True): the LP's duals if it ended optimal
    ranging: "CoreRanging | None" = None  # solve_batch(ranging=...): the LP's ranges if it ended optimal
    ray: "CoreRay | None" = None        # solve_batch(rays=True): the LP's ray if it ended unbounded or infeasible


@dataclass
class CoreDuals:
    """Dual values and reduced costs at an optimal basis, core sense (dzg_duals): y per row, d per
    variable (0.0 for basics), the certificate scalars, and where they come from: "fresh"
    (recomputed on the device from the final basis) or "carried" (read off the carried z)."""
    source: str
    source_code: int
    y: np.ndarray
    d: np.ndarray
    primal_obj: float
    dual_obj: float
    primal_infeas: float
    dual_infeas: float
    z_diff: float


@dataclass
class CoreRanging:
    """Sensitivity ranges at an optimal basis, core sense (dzg_ranging): per requested cost direction
    and per requested right-hand-side direction the interval [lo, hi] of the step t over which the
    basis stays optimal (0 is always inside; -inf / +inf where nothing blocks) and the variable that
    blocks each end (-1: none).  duals: the CoreDuals of the same call."""
    cost_lo: np.ndarray
    cost_hi: np.ndarray
    cost_lo_var: np.ndarray
    cost_hi_var: np.ndarray
    rhs_lo: np.ndarray
    rhs_hi: np.ndarray
    rhs_lo_var: np.ndarray
    rhs_hi_var: np.ndarray
    duals: "CoreDuals | None" = None


def _core_ranging(buf: "_ffi.RangingBuffers", duals=None) -> CoreRanging:
    c, r = buf.side(0), buf.side(1)
    return CoreRanging(cost_lo=c[0], cost_hi=c[1], cost_lo_var=c[2], cost_hi_var=c[3],
                       rhs_lo=r[0], rhs_hi=r[1], rhs_lo_var=r[2], rhs_hi_var=r[3], duals=duals)


def _ranging_dirs(dirs, count: int) -> list:
    """None: every index's own unit direction; otherwise a list of {index: coefficient}."""
    if dirs is None:
        return [{j: 1.0} for j in range(count)]
    return [dict(d) for d in dirs]


@dataclass
class CoreRay:
    """What a solve that ended unbounded or infeasible shows for it, core sense (dzg_ray).  kind
    "primal": d is a direction with [A | I] d = 0 that gains `value` per unit; kind "farkas": y are
    row multipliers, d = y^T [A | I] the aggregated row and value = rhs0 . y.  var / pos: the
    variable find_first_pivot chose and its position, mu its ratio.  violation: the largest entry of d
    below zero, as a positive number (NaN if the vector holds a NaN).  proven: violation == 0 and
    value > 0 (primal) or value < 0 (farkas)."""
    kind: str
    kind_code: int
    proven: bool
    var: int
    pos: int
    mu: float
    value: float
    violation: float
    d: np.ndarray
    y: np.ndarray


_RAY_KIND_NAMES = {_ffi.RAY_PRIMAL: "primal", _ffi.RAY_FARKAS: "farkas"}


def _core_ray(u, d, y) -> CoreRay:
    return CoreRay(kind=_RAY_KIND_NAMES[int(u.kind)], kind_code=int(u.kind), proven=bool(u.proven),
                   var=int(u.var), pos=int(u.pos), mu=float(u.mu), value=float(u.value),
                   violation=float(u.violation), d=d, y=y)


def _core_duals(u, y, d) -> CoreDuals:
    return CoreDuals(source=_ffi.DUALS_SOURCE_NAMES.get(int(u.source), "none"), source_code=int(u.source),
                     y=y, d=d, primal_obj=float(u.primal_obj), dual_obj=float(u.dual_obj),
                     primal_infeas=float(u.primal_infeas), dual_infeas=float(u.dual_infeas),
                     z_diff=float(u.z_diff))


def _counters(r) -> dict:
    """The scalar tail of a dzg_result that every entry point reports alike."""
    return dict(max_pivot_error=float(r.max_pivot_error), near_ties=int(r.near_ties),
                first_near_tie=int(r.first_near_tie), min_margin=float(r.min_margin),
                dense_columns=int(r.dense_columns), refactors=int(r.refactors),
                chain_fallbacks=int(r.chain_fallbacks), price_pass_used=int(r.price_pass_used),
                price_rows_copy=int(r.price_rows_copy), state_drift=float(r.state_drift))


def _c_lp(lp: CoreLP):
    """The dzg_lp of a CoreLP, and the arrays its pointers refer to (keep them alive)."""
    m, ns, n = lp.m, lp.n_struct, lp.n
    # column-major m x ns == C-contiguous (ns, m)
    a_cm = None if lp.a is None else np.ascontiguousarray(np.asarray(lp.a, dtype=np.float64).T)
    k = dict(a=a_cm, c=f64(lp.c), basis=i64(lp.basis), nonbasis=i64(lp.nonbasis),
             x=f64(lp.x), z=f64(lp.z),
             var_col=None if lp.var_col is None else i64(lp.var_col),
             col_ptr=None if lp.col_ptr is None else i64(lp.col_ptr),
             row_idx=None if lp.row_idx is None
             else np.ascontiguousarray(lp.row_idx, dtype=np.int32),
             val=None if lp.val is None else f64(lp.val),
             xbar=None if lp.xbar is None else f64(lp.xbar),
             zbar=None if lp.zbar is None else f64(lp.zbar))
    if len(k["basis"]) != m or len(k["x"]) != m or len(k["nonbasis"]) != n - m \
            or len(k["z"]) != n - m \
            or (k["xbar"] is not None and len(k["xbar"]) != m) \
            or (k["zbar"] is not None and len(k["zbar"]) != n - m):
        raise ValueError("CoreLP vectors do not match (m, n)")
    c_lp = _ffi.Lp(m, n, ns, ptr(a_cm), max(m, 1), ptr(k["var_col"]), ptr(k["c"]),
                   float(lp.constant), ptr(k["basis"]), ptr(k["nonbasis"]),
                   ptr(k["x"]), ptr(k["z"]), ptr(k["col_ptr"]), ptr(k["row_idx"]),
                   ptr(k["val"]), ptr(k["xbar"]), ptr(k["zbar"]))
    return c_lp, k


class Solver:
    """One LP resident on one GPU.  create -> run (repeatable, budgeted) -> result."""

    def __init__(self, lp: CoreLP, **opts):
        self._prepare(lp, opts)
        rc = _ffi.lib().dzg_solver_create(C.byref(self._c_lp), C.byref(self._opts),
                                          C.byref(self._h))
        _ffi.check(rc, "dzg_solver_create")

    def _prepare(self, lp: CoreLP, opts: dict) -> "Solver":
        """Marshals the LP and the options into their C structs (no device work)."""
        _ffi.require_gpu()
        self._lp = lp
        self._c_lp, self._keep = _c_lp(lp)
        if lp.block is not None:
            if (opts.get("col_begin"), opts.get("col_end")) != tuple(lp.block):
                raise ValueError("a column-block LP needs a sharded solver on exactly that block")
            opts["a_is_block"] = 1
        self._opts = _ffi.default_opts(**opts)
        self._h = C.c_void_p(None)
        return self

    def run(self, max_new_iters: int = 0) -> str:
        rc = _ffi.lib().dzg_solver_run(self._h, int(max_new_iters))
        _ffi.check(rc, "dzg_solver_run")
        return STATUS_NAMES[rc]

    def result(self, log: bool = True, log_cap: int | None = None) -> CoreResult:
        m, q = self._lp.m, self._lp.n - self._lp.m
        basis, nonbasis = np.zeros(max(m, 1), np.int64), np.zeros(max(q, 1), np.int64)
        x, xbar = np.zeros(max(m, 1)), np.zeros(max(m, 1))
        z, zbar = np.zeros(max(q, 1)), np.zeros(max(q, 1))
        cap = int(log_cap if log_cap is not None else (1 << 22)) if log else 0
        # first learn the iteration count so the log buffer is not oversized
        r = _ffi.Result()
        r.basis, r.nonbasis, r.x, r.xbar = ptr(basis), ptr(nonbasis), ptr(x), ptr(xbar)
        r.z, r.zbar = ptr(z), ptr(zbar)
        r.log, r.log_cap = None, 0
        _ffi.check(_ffi.lib().dzg_solver_result(self._h, C.byref(r)), "dzg_solver_result")
        pivots, margins = [], None
        if log and r.iterations > 0:
            cnt = int(min(r.iterations, cap))
            buf = (_ffi.Pivot * cnt)()
            margins = np.full(cnt, np.inf)
            r.log, r.log_cap, r.margins = C.cast(buf, C.c_void_p), cnt, ptr(margins)
            _ffi.check(_ffi.lib().dzg_solver_result(self._h, C.byref(r)), "dzg_solver_result")
            arr = np.ctypeslib.as_array(buf)
            pivots = list(zip(arr["kind"].tolist(), arr["entering"].tolist(),
                              arr["leaving"].tolist(), arr["mu"].tolist()))
        return CoreResult(
            status=STATUS_NAMES.get(r.status, str(r.status)), status_code=r.status,
            numerics="strict" if r.numerics_used == STRICT else "fast",
            iterations=int(r.iterations), objective=float(r.objective),
            basis=basis[:m].copy(), nonbasis=nonbasis[:q].copy(), x=x[:m].copy(),
            xbar=xbar[:m].copy(), z=z[:q].copy(), zbar=zbar[:q].copy(), pivots=pivots,
            kernel_ms={k: r.kernel_ms[i] for i, k in enumerate(_ffi.KERNEL_CLASSES)},
            kernel_launches={k: r.kernel_launches[i] for i, k in enumerate(_ffi.KERNEL_CLASSES)},
            price_bytes=float(r.price_bytes), solve_ms=float(r.solve_ms), margins=margins,
            **_counters(r))

    def set_profile(self, mask: int) -> None:
        """Which kernel classes (bits 1 << _ffi.K_*) the following runs time with HIP events."""
        _ffi.check(_ffi.lib().dzg_solver_set_profile(self._h, int(mask)), "dzg_solver_set_profile")

    def refactor(self) -> None:
        """FAST: rebuild the basis inverse from scratch now (blocked LU + MFMA GEMMs)."""
        _ffi.check(_ffi.lib().dzg_solver_refactor(self._h), "dzg_solver_refactor")

    def duals(self) -> CoreDuals:
        """dzg_solver_duals: y = B^-T c_B and the reduced costs of the OPTIMAL basis this solver
        ended on.  A FAST solver refactorises that basis for it (create it with
        refactor_interval != 0); CSC and sharded solvers return the carried values."""
        m, n = self._lp.m, self._lp.n
        y, d = np.zeros(max(m, 1)), np.zeros(max(n, 1))
        u = _ffi.Duals()
        u.y, u.d = ptr(y), ptr(d)
        _ffi.check(_ffi.lib().dzg_solver_duals(self._h, C.byref(u)), "dzg_solver_duals")
        return _core_duals(u, y[:m].copy(), d[:n].copy())

    def ranging(self, cost_dirs=None, rhs_dirs=None, pivot_tol: float = 0.0) -> CoreRanging:
        """dzg_solver_ranging: how far each cost direction (a {variable: coefficient} dict; None: every
        variable's own coefficient) and each right-hand-side direction ({row: coefficient}; None:
        every row's own right-hand side) can be followed before the OPTIMAL basis this solver ended
        on changes.  Runs duals() first, with its preconditions and side effects; `.duals` of the
        result is that call's.  CSC and sharded solvers: NotImplementedError."""
        m, n = self._lp.m, self._lp.n
        buf = _ffi.RangingBuffers(_ranging_dirs(cost_dirs, n), _ranging_dirs(rhs_dirs, m), pivot_tol)
        req, out = _ffi.RangingReq(), _ffi.Ranging()
        buf.fill(req, out)
        y, d = np.zeros(max(m, 1)), np.zeros(max(n, 1))
        u = _ffi.Duals()
        u.y, u.d = ptr(y), ptr(d)
        _ffi.check_ranging(_ffi.lib().dzg_solver_ranging(self._h, C.byref(req), C.byref(u), C.byref(out)),
                           "dzg_solver_ranging")
        return _core_ranging(buf, _core_duals(u, y[:m].copy(), d[:n].copy()))

    def ray(self) -> CoreRay:
        """dzg_solver_ray: the primal ray of the basis an UNBOUNDED solve stopped on, or the Farkas ray
        of an INFEASIBLE one, recomputed from that basis with its sign conditions checked
        (`.proven`).  A FAST solver refactorises the basis for it (create it with
        refactor_interval != 0); CSC and sharded solvers: NotImplementedError."""
        m, n = self._lp.m, self._lp.n
        d, y = np.zeros(max(n, 1)), np.zeros(max(m, 1))
        u = _ffi.Ray()
        u.d, u.y = ptr(d), ptr(y)
        _ffi.check_ray(_ffi.lib().dzg_solver_ray(self._h, C.byref(u)), "dzg_solver_ray")
        return _core_ray(u, d[:n].copy(), y[:m].copy())

    def reoptimize(self, b=None, c=None, constant=None) -> None:
        """dzg_solver_reoptimize: replaces the right-hand side `b` (m entries, by row), the objective
        `c` (n entries, by variable, core sense) and / or the constant of the LP this solver holds,
        and recomputes the state of its CURRENT basis for them on the GPU (x = B^-1 b, z the reduced
        costs, xbar = zbar = 1); run() then carries on from that basis, and the pivot count and log
        keep accumulating.  Allowed before a run and after any end but singular / panic.  A FAST
        solver refactorises the basis for it (create it with refactor_interval != 0) and no longer
        measures state_drift afterwards; CSC and sharded solvers: NotImplementedError.  ValueError
        for a wrong length or when nothing is given."""
        m, n = self._lp.m, self._lp.n
        if b is None and c is None and constant is None:
            raise ValueError("reoptimize: give b, c or constant")
        b = None if b is None else f64(b)
        c = None if c is None else f64(c)
        if b is not None and b.shape != (m,):
            raise ValueError(f"reoptimize: b has shape {b.shape}, the LP has {m} rows")
        if c is not None and c.shape != (n,):
            raise ValueError(f"reoptimize: c has shape {c.shape}, the LP has {n} variables")
        chg = _ffi.Reopt(ptr(b), ptr(c), 0.0 if constant is None else float(constant),
                         0 if constant is None else 1, 0)
        _ffi.check_reopt(_ffi.lib().dzg_solver_reoptimize(self._h, C.byref(chg)), "dzg_solver_reoptimize")

    def extend(self, rows=None, rhs=None, cols=None, c_cols=None) -> None:
        """dzg_solver_extend: appends constraint rows (rows (p, n_struct) on the existing structural
        columns, rhs (p,)) and / or structural columns (cols (m + p, r) over all rows, the new ones
        included, c_cols (r,), core sense) to the LP this solver holds and recomputes the state of the
        extended basis -- the current one with the new slacks appended, the new variables nonbasic --
        as reoptimize() does; run() then carries on from it.  No existing index changes (see
        extended_lp, which is the LP this solver holds afterwards); the pivot count and log keep
        accumulating.  The resident matrix is re-laid on the GPU, only the new numbers are uploaded;
        both matrices are resident until the call returns.  Allowed where reoptimize() is; CSC and
        sharded solvers: NotImplementedError.  ValueError for a wrong shape or when nothing is given.
        All or nothing: a call that raises leaves the solver as it was."""
        lp2 = extended_lp(self._lp, rows, rhs, cols, c_cols)
        m, ns = self._lp.m, self._lp.n_struct
        rows, rhs, cols, c_cols = _extend_blocks(m, ns, rows, rhs, cols, c_cols)
        p, r = len(rhs), len(c_cols)
        rows_rm = np.ascontiguousarray(rows)            # (p, ns) row-major
        cols_cm = np.ascontiguousarray(cols.T)          # column-major (m + p) x r
        ext = _ffi.Extend(p, r, ptr(rows_rm) if p else None, max(ns, 1), ptr(rhs) if p else None,
                          ptr(cols_cm) if r else None, max(m + p, 1), ptr(c_cols) if r else None)
        _ffi.check_extend(_ffi.lib().dzg_solver_extend(self._h, C.byref(ext)), "dzg_solver_extend")
        self._lp = lp2

    def _at_current_basis(self) -> CoreLP:
        """The LP this solver holds with the lists and the state of the basis it stands at."""
        import dataclasses

        res = self.result(log=False)
        return dataclasses.replace(self._lp, basis=res.basis, nonbasis=res.nonbasis, x=res.x, z=res.z,
                                   xbar=None, zbar=None)

    def removable(self) -> tuple[np.ndarray, np.ndarray]:
        """(row_mask (m,), col_mask (n_struct,)) at the current basis: the rows whose slack is basic
        and the structural columns whose variable is nonbasic -- what remove() takes."""
        if self._lp.a is None or self._lp.block is not None:
            raise NotImplementedError("remove is not supported on CSC storage or sharded solvers")
        m, ns = self._lp.m, self._lp.n_struct
        res = self.result(log=False)
        codes = _codes(self._lp)
        in_basis, out_of_basis = codes[res.basis], codes[res.nonbasis]
        row_mask, col_mask = np.zeros(m, bool), np.zeros(ns, bool)
        row_mask[-1 - in_basis[in_basis < 0]] = True
        col_mask[out_of_basis[out_of_basis >= 0]] = True
        return row_mask, col_mask

    def remove(self, rows=None, cols=None) -> tuple[np.ndarray, np.ndarray]:
        """dzg_solver_remove: drops constraint rows (with their slacks) and / or structural columns
        (with their variables) from the LP this solver holds and recomputes the state of the reduced
        basis as extend() does; run() then carries on from it.  Only what is free may go (see
        removable()): a row whose slack is basic, a column whose variable is nonbasic -- an optimal
        solver stays optimal and the next run() takes no pivot.  Survivors are renumbered in ascending
        order of their old index (see reduced_lp, which is the LP this solver holds afterwards);
        returns (var_map (old n,), row_map (old m,)): the new index, or -1 for what was dropped.  The
        pivot count and log keep accumulating; the log's older entries keep the numbering of their
        time.  The matrix is gathered on the GPU from the resident one, only the lists of survivors
        are uploaded.  Allowed where extend() is; CSC and sharded solvers: NotImplementedError.
        ValueError for what the C call refuses about the lists (a binding row, a basic column, an
        index out of range or listed twice, nothing given, no row or column left).  All or nothing: a
        call that raises leaves the solver as it was."""
        if self._lp.a is None or self._lp.block is not None:
            raise NotImplementedError("remove is not supported on CSC storage or sharded solvers")
        drop_row, drop_col = _remove_lists(self._lp.m, self._lp.n_struct, rows, cols)
        lp2, _, _ = reduced_lp(self._at_current_basis(), rows, cols)
        r, c = np.flatnonzero(drop_row).astype(np.int64), np.flatnonzero(drop_col).astype(np.int64)
        var_map, row_map = np.zeros(self._lp.n, np.int64), np.zeros(self._lp.m, np.int64)
        rem = _ffi.Remove(len(r), ptr(r) if len(r) else None, len(c), ptr(c) if len(c) else None)
        _ffi.check_extend(_ffi.lib().dzg_solver_remove(self._h, C.byref(rem), ptr(var_map), ptr(row_map)),
                          "dzg_solver_remove")
        self._lp = lp2
        return var_map, row_map

    def dims(self) -> tuple[int, int, int]:
        """dzg_solver_dims: (m, n, n_struct) of the LP the solver holds now."""
        v = [C.c_int64(0), C.c_int64(0), C.c_int64(0)]
        _ffi.check(_ffi.lib().dzg_solver_dims(self._h, *(C.byref(x) for x in v)), "dzg_solver_dims")
        return tuple(int(x.value) for x in v)

    def debug_matrix(self) -> np.ndarray:
        """Test hook (dzg_debug_matrix): the (m, n_struct) matrix as the device holds it."""
        m, _, ns = self.dims()
        out = np.zeros((max(ns, 1), max(m, 1)))         # column-major m x ns
        _ffi.check(_ffi.lib().dzg_debug_matrix(self._h, 0, ns, ptr(out), max(m, 1)), "dzg_debug_matrix")
        return out[:ns, :m].T.copy()

    def debug_matrix_rows(self) -> np.ndarray | None:
        """Test hook (dzg_debug_matrix_rows): the row-major copy of the matrix the row-wise pricing
        pass reads, (m, n_struct); None where that copy is not kept."""
        m, _, ns = self.dims()
        out = np.zeros((max(m, 1), max(ns, 1)))
        got = _ffi.lib().dzg_debug_matrix_rows(self._h, 0, m, ptr(out), max(ns, 1))
        _ffi.check(int(got), "dzg_debug_matrix_rows")
        return out[:m, :ns].copy() if got == m and m > 0 else None

    def debug_extend_ms(self) -> tuple[float, float, float]:
        """dzg_debug_extend_ms: ms the last extend() spent on (the matrix, the refactorisation, the
        restart state)."""
        ms = np.zeros(3)
        _ffi.check(_ffi.lib().dzg_debug_extend_ms(self._h, ptr(ms)), "dzg_debug_extend_ms")
        return tuple(float(x) for x in ms)

    def debug_inverse(self, row0: int, row1: int) -> tuple[np.ndarray, dict]:
        """Test hook (dzg_debug_basis_inverse): rows [row0, row1) of the basis inverse FAST keeps --
        row i is basis position row0 + i, column r constraint row r -- and
        {k, neta, rows: the (first, end) rows this solver keeps}."""
        m = self._lp.m
        out = np.zeros((max(int(row1) - int(row0), 0), m))
        info = np.zeros(4, np.int64)
        _ffi.check(_ffi.lib().dzg_debug_basis_inverse(self._h, int(row0), int(row1), ptr(out), ptr(info)),
                   "dzg_debug_basis_inverse")
        return out, dict(k=int(info[0]), neta=int(info[1]), rows=(int(info[2]), int(info[3])))

    def debug_chain_price_counts(self) -> tuple[int, int]:
        """Test hook (dzg_debug_chain_price_counts): chain iterations enqueued with the small-k pricing
        pass in k_chain_pre's tail (two launches a pivot), and with the pass as a launch of its own."""
        counts = np.zeros(2, np.int64)
        _ffi.check(_ffi.lib().dzg_debug_chain_price_counts(self._h, ptr(counts)), "dzg_debug_chain_price_counts")
        return int(counts[0]), int(counts[1])

    def debug_wk_mismatch(self, clear_valid: bool = False) -> tuple[int, bool]:
        """Test hook (dzg_debug_wk_mismatch): entries of the kept compact copy of the eta rows that differ
        bitwise from a fresh gather, and whether the host held the copy valid; clear_valid: the next chain
        batch gathers it again."""
        info = np.zeros(2, np.int64)
        _ffi.check(_ffi.lib().dzg_debug_wk_mismatch(self._h, int(bool(clear_valid)), ptr(info)),
                   "dzg_debug_wk_mismatch")
        return int(info[0]), bool(info[1])

    def close(self) -> None:
        if self._h:
            _ffi.lib().dzg_solver_destroy(self._h)
            self._h = C.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def solve(lp: CoreLP, log: bool = True, **opts) -> CoreResult:
    """Simplex::solve on the GPU: create + run to termination + result."""
    with Solver(lp, **opts) as s:
        s.run(0)
        return s.result(log=log)


def core_solve(lp: CoreLP, log_cap: int = 1 << 20, **opts) -> CoreResult:
    """dzg_core_solve: one call, with the AUTO policy of the C ABI (FAST that stops at the first
    near tie and is then re-solved in STRICT, up to DZG_AUTO_STRICT_RESTART_ROWS rows)."""
    with Solver.__new__(Solver)._prepare(lp, opts) as s:
        m, q = lp.m, lp.n - lp.m
        basis, nonbasis = np.zeros(max(m, 1), np.int64), np.zeros(max(q, 1), np.int64)
        x, xbar = np.zeros(max(m, 1)), np.zeros(max(m, 1))
        z, zbar = np.zeros(max(q, 1)), np.zeros(max(q, 1))
        buf = (_ffi.Pivot * max(log_cap, 1))()
        margins = np.full(max(log_cap, 1), np.inf)
        r = _ffi.Result()
        r.basis, r.nonbasis, r.x, r.xbar = ptr(basis), ptr(nonbasis), ptr(x), ptr(xbar)
        r.z, r.zbar = ptr(z), ptr(zbar)
        r.log, r.log_cap, r.margins = C.cast(buf, C.c_void_p), log_cap, ptr(margins)
        rc = _ffi.lib().dzg_core_solve(C.byref(s._c_lp), C.byref(s._opts), C.byref(r))
        _ffi.check(rc, "dzg_core_solve")
        cnt = int(min(r.iterations, log_cap))
        arr = np.ctypeslib.as_array(buf)[:cnt]
        pivots = list(zip(arr["kind"].tolist(), arr["entering"].tolist(),
                          arr["leaving"].tolist(), arr["mu"].tolist()))
        return CoreResult(
            status=STATUS_NAMES.get(r.status, str(r.status)), status_code=r.status,
            numerics="strict" if r.numerics_used == STRICT else "fast",
            iterations=int(r.iterations), objective=float(r.objective),
            basis=basis[:m].copy(), nonbasis=nonbasis[:q].copy(), x=x[:m].copy(),
            xbar=xbar[:m].copy(), z=z[:q].copy(), zbar=zbar[:q].copy(), pivots=pivots,
            margins=margins[:cnt].copy(), **_counters(r))


_PIVOT_DTYPE = np.dtype([("kind", "<i4"), ("reserved", "<i4"), ("entering", "<i8"),
                         ("leaving", "<i8"), ("mu", "<f8")])


def _batch_starts(lps, start) -> list:
    """solve_batch's `start`, checked: per LP None or the (basis, nonbasis) pair as int64 arrays."""
    start = list(start)
    if len(start) != len(lps):
        raise ValueError(f"start: {len(start)} entries for {len(lps)} LPs (one per LP, None = cold)")
    out = []
    for i, (lp, s) in enumerate(zip(lps, start)):
        if isinstance(s, CoreResult):
            s = None if s.status in ("singular", "panic") else (s.basis, s.nonbasis)
        if s is None:
            out.append(None)
            continue
        try:
            basis, nonbasis = s
        except (TypeError, ValueError):
            raise ValueError(f"start[{i}]: None, a CoreResult or a (basis, nonbasis) pair") from None
        basis, nonbasis = i64(basis), i64(nonbasis)
        m, n = lp.m, lp.n
        if basis.shape != (m,) or nonbasis.shape != (n - m,):
            raise ValueError(f"start[{i}]: basis / nonbasis of {basis.size} / {nonbasis.size} entries, "
                             f"lps[{i}] has m = {m}, n - m = {n - m}")
        codes = _codes(lp)[i64(lp.basis)] if len(lp.basis) == m and m > 0 else np.zeros(0, np.int64)
        if (codes >= 0).any() or len(set(codes.tolist())) != m:
            raise ValueError(f"lps[{i}]: a warm LP is given in slack-basis form (its own basis all slack)")
        both = np.concatenate([basis, nonbasis])
        if both.size and (both.min() < 0 or both.max() >= n or len(set(both.tolist())) != n):
            raise ValueError(f"start[{i}]: basis / nonbasis is not a partition of 0 .. {n - 1}")
        out.append((basis, nonbasis))
    return out


def solve_batch(lps, log: bool = True, log_cap: int = 4096, pivots_per_launch: int = 0,
                duals: bool = False, ranging=False, pivot_tol: float = 0.0, rays: bool = False,
                start=None, **opts) -> list:
    """dzg_batch_solve: every LP of `lps` in STRICT numerics, one workgroup per LP, in one call.

    The whole batch is checked on the host first (ValueError: more than 128 rows, CSC input, FAST
    numerics, a column-block LP, vectors that do not match (m, n)); nothing reaches the device
    before that.  Result i is LP i's CoreResult, as `solve(lp, numerics=STRICT)` reports it; its
    solve_ms is the wall time of the whole batch call.  A result resumes through resumed_from, in a
    batch or in a single Solver.  duals=True (dzg_batch_solve_duals): every result gains `.duals`, a
    CoreDuals for an LP that ended optimal and None otherwise.  ranging=True, or one request per LP
    as (cost_dirs, rhs_dirs) with the meaning of Solver.ranging (dzg_batch_solve_ranging): every
    result gains `.ranging`, a CoreRanging, and `.duals` as well; None for an LP that did not end
    optimal.  rays=True (dzg_batch_solve_rays; composes with duals, not with ranging): every result
    gains `.ray`, a CoreRay for an LP that ended unbounded or infeasible and None otherwise.

    start (dzg_batch_solve_from; composes with duals, not with ranging or rays): one entry per LP,
    each None (solve this LP cold, exactly as without `start`), a CoreResult of an earlier solve of
    the same matrix, or a (basis, nonbasis) pair.  A CoreResult that ended singular or panicked
    counts as None.  `lps[i]` is the LP to solve now in slack-basis form (its x is the right-hand
    side, its c the costs); a warm LP gets the state its start basis defines for that data (x =
    B^-1 rhs, fresh reduced costs, xbar = zbar = 1) and is pivoted on from there.  iterations and
    pivots count from 0.  A singular start basis ends "singular" with 0 iterations."""
    import time

    lps = list(lps)
    numerics = opts.get("numerics", AUTO)
    if numerics not in (STRICT, AUTO):
        raise ValueError("solve_batch runs STRICT numerics only (numerics=STRICT or AUTO)")
    if rays and ranging is not False and ranging is not None:
        raise ValueError("rays=True and ranging: the ranging call carries no ray; ask in two calls")
    if start is not None and (rays or (ranging is not False and ranging is not None)):
        raise ValueError("start composes with duals only: ask for ranging or rays in a call without it")
    starts = None if start is None else _batch_starts(lps, start)
    for i, lp in enumerate(lps):
        if lp.block is not None:
            raise ValueError(f"lps[{i}]: a column-block LP cannot be batched")
        if lp.a is None and lp.n_struct > 0:
            raise ValueError(f"lps[{i}]: CSC input cannot be batched (dense `a` only)")
        if lp.m > _ffi.BATCH_MAX_ROWS:
            raise ValueError(f"lps[{i}]: {lp.m} rows; the batch takes at most {_ffi.BATCH_MAX_ROWS}")
    marshalled = [_c_lp(lp) for lp in lps]
    count = len(lps)
    c_lps = (_ffi.Lp * max(count, 1))(*[c for c, _ in marshalled])
    ms = [lp.m for lp in lps]
    qs = [lp.n - lp.m for lp in lps]
    mo = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    qo = np.concatenate([[0], np.cumsum(qs)]).astype(np.int64)
    basis, x, xbar = np.zeros(mo[-1] + 1, np.int64), np.zeros(mo[-1] + 1), np.zeros(mo[-1] + 1)
    nonbasis, z, zbar = np.zeros(qo[-1] + 1, np.int64), np.zeros(qo[-1] + 1), np.zeros(qo[-1] + 1)
    cap = int(log_cap) if log else 0
    logs = np.zeros((count, max(cap, 1)), dtype=_PIVOT_DTYPE)
    res = (_ffi.Result * max(count, 1))()
    for i in range(count):
        r = res[i]
        r.basis = basis.ctypes.data + 8 * int(mo[i])
        r.x = x.ctypes.data + 8 * int(mo[i])
        r.xbar = xbar.ctypes.data + 8 * int(mo[i])
        r.nonbasis = nonbasis.ctypes.data + 8 * int(qo[i])
        r.z = z.ctypes.data + 8 * int(qo[i])
        r.zbar = zbar.ctypes.data + 8 * int(qo[i])
        r.log = logs.ctypes.data + logs.strides[0] * i if cap > 0 else None
        r.log_cap = cap
    o = _ffi.default_opts(**opts)
    want_ranging = ranging is not False and ranging is not None
    if want_ranging:
        duals = True
        reqs = [(None, None)] * count if ranging is True else list(ranging)
        if len(reqs) != count:
            raise ValueError("ranging: one (cost_dirs, rhs_dirs) request per LP")
        bufs = [_ffi.RangingBuffers(_ranging_dirs(cd, lp.n), _ranging_dirs(rd, lp.m), pivot_tol)
                for (cd, rd), lp in zip(reqs, lps)]
        c_req, c_rg = (_ffi.RangingReq * max(count, 1))(), (_ffi.Ranging * max(count, 1))()
        for i, buf in enumerate(bufs):
            buf.fill(c_req[i], c_rg[i])
    if duals:
        ns = [lp.n for lp in lps]
        no = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        y_all, d_all = np.zeros(mo[-1] + 1), np.zeros(no[-1] + 1)
        du = (_ffi.Duals * max(count, 1))()
        for i in range(count):
            du[i].y = y_all.ctypes.data + 8 * int(mo[i])
            du[i].d = d_all.ctypes.data + 8 * int(no[i])
    if rays:
        ns_r = [lp.n for lp in lps]
        ro = np.concatenate([[0], np.cumsum(ns_r)]).astype(np.int64)
        rd_all, ry_all = np.zeros(ro[-1] + 1), np.zeros(mo[-1] + 1)
        ry = (_ffi.Ray * max(count, 1))()
        for i in range(count):
            ry[i].d = rd_all.ctypes.data + 8 * int(ro[i])
            ry[i].y = ry_all.ctypes.data + 8 * int(mo[i])
    if starts is not None:
        c_start = (_ffi.BatchStart * max(count, 1))()
        for i, s in enumerate(starts):
            if s is not None:
                c_start[i].basis, c_start[i].nonbasis = ptr(s[0]), ptr(s[1])
    t0 = time.perf_counter()
    if starts is not None:
        rc = _ffi.lib().dzg_batch_solve_from(c_lps, c_start, C.c_int64(count), C.byref(o),
                                             C.c_int64(int(pivots_per_launch)), res, du if duals else None)
    elif rays:
        rc = _ffi.lib().dzg_batch_solve_rays(c_lps, C.c_int64(count), C.byref(o),
                                             C.c_int64(int(pivots_per_launch)), res, du if duals else None, ry)
    elif want_ranging:
        rc = _ffi.lib().dzg_batch_solve_ranging(c_lps, C.c_int64(count), C.byref(o),
                                                C.c_int64(int(pivots_per_launch)), c_req, res, du, c_rg)
    elif duals:
        rc = _ffi.lib().dzg_batch_solve_duals(c_lps, C.c_int64(count), C.byref(o),
                                              C.c_int64(int(pivots_per_launch)), res, du)
    else:
        rc = _ffi.lib().dzg_batch_solve(c_lps, C.c_int64(count), C.byref(o),
                                        C.c_int64(int(pivots_per_launch)), res)
    wall_ms = (time.perf_counter() - t0) * 1e3
    _ffi.check_ranging(rc, "dzg_batch_solve_from" if starts is not None else "dzg_batch_solve_rays" if rays else "dzg_batch_solve_ranging" if want_ranging else
                       ("dzg_batch_solve_duals" if duals else "dzg_batch_solve"))
    out = []
    for i in range(count):
        r = res[i]
        cnt = int(min(r.iterations, cap))
        arr = logs[i, :cnt]
        pivots = list(zip(arr["kind"].tolist(), arr["entering"].tolist(), arr["leaving"].tolist(),
                          arr["mu"].tolist()))
        a0, a1, b0, b1 = int(mo[i]), int(mo[i + 1]), int(qo[i]), int(qo[i + 1])
        out.append(CoreResult(
            status=STATUS_NAMES.get(r.status, str(r.status)), status_code=r.status,
            numerics="strict", iterations=int(r.iterations), objective=float(r.objective),
            basis=basis[a0:a1].copy(), nonbasis=nonbasis[b0:b1].copy(), x=x[a0:a1].copy(),
            xbar=xbar[a0:a1].copy(), z=z[b0:b1].copy(), zbar=zbar[b0:b1].copy(), pivots=pivots,
            solve_ms=wall_ms, **_counters(r)))
        if duals:
            out[-1].duals = None if du[i].source == 0 else _core_duals(
                du[i], y_all[a0:a1].copy(), d_all[int(no[i]):int(no[i + 1])].copy())
        if want_ranging and out[-1].duals is not None:
            out[-1].ranging = _core_ranging(bufs[i], out[-1].duals)
        if rays and ry[i].kind != 0:
            out[-1].ray = _core_ray(ry[i], rd_all[int(ro[i]):int(ro[i + 1])].copy(), ry_all[a0:a1].copy())
    return out


def solve_batch_fast(lps, log: bool = True, log_cap: int = 4096, pivots_per_launch: int = 0,
                     refactor_every: int = 0, start=None, duals: bool = False, ranging=False,
                     pivot_tol: float = 0.0, rays: bool = False, **opts) -> list:
    """dzg_batch_solve_fast: every LP of `lps` in FAST numerics, one workgroup per LP with the
    explicit basis inverse in LDS, in one call.

    The same host checks as solve_batch run first (ValueError: more than 128 rows, CSC input, a
    column-block LP, vectors that do not match (m, n)).  Keywords: numerics (FAST; AUTO, the default:
    FAST that stops at the first near tie, the LPs it gave up on re-solved by the STRICT batch in the
    same call; STRICT: solve_batch's path), near_tie_action, tie_tol, max_iter, epsilon.  Result i
    is LP i's CoreResult; `.numerics` says which numerics produced it, and near_ties, first_near_tie,
    min_margin, margins, max_pivot_error and refactors mean what they mean for a single FAST solve.
    pivots_per_launch 0 = 128; refactor_every 0 = 64 pivots between two rebuilds of the inverse.

    start (dzg_batch_solve_fast_from): one entry per LP with the meaning solve_batch(start=...) gives
    it -- None, a CoreResult of either numerics (one that ended singular or panicked counts as None)
    or a (basis, nonbasis) pair; `lps[i]` is then the LP to solve now in slack-basis form.  A warm LP
    gets the FAST restart state of its start basis (x = B^-1 rhs and fresh reduced costs from the
    inverse a launch builds, xbar = zbar = 1) and is pivoted on from there; iterations and pivots
    count from 0, refactors includes the restart's inversion.  A singular start basis ends
    "singular" with 0 iterations in FAST; under AUTO the STRICT batch solves it, and every other LP
    FAST gave up on, from the same start.

    duals, ranging, pivot_tol, rays (dzg_batch_solve_post; all compose with each other and with
    start): what solve_batch's keywords of the same names ask for, from the state each LP ended in.
    ranging is True (every unit direction) or one (cost_dirs, rhs_dirs) per LP.  Results gain
    `.duals`, `.ranging` and `.ray` as solve_batch sets them, None where none was computed.  A FAST
    result's come from the inverse of its final basis, built as the batch builds it; a STRICT
    result's (numerics=STRICT, or an LP AUTO handed over) are solve_batch's own.  Without these
    keywords the call is exactly what it was."""
    lps = list(lps)
    allowed = {"numerics", "near_tie_action", "tie_tol", "max_iter", "epsilon", "device"}
    unknown = set(opts) - allowed
    if unknown:
        raise ValueError(f"solve_batch_fast takes {sorted(allowed)}, not {sorted(unknown)}")
    if opts.get("numerics", AUTO) not in (STRICT, FAST, AUTO):
        raise ValueError("solve_batch_fast: numerics is STRICT, FAST or AUTO")
    if int(pivots_per_launch) < 0 or int(refactor_every) < 0:
        raise ValueError("solve_batch_fast: pivots_per_launch and refactor_every are >= 0")

    want_ranging = ranging is not False and ranging is not None
    if not (0.0 <= float(pivot_tol)):
        raise ValueError("solve_batch_fast: pivot_tol is >= 0 (0 selects 1e-9)")
    if duals or want_ranging or rays:
        starts = None if start is None else _batch_starts(lps, start)

        def invoke_post(c_lps, count, o, res, c_post):
            c_start = None
            if starts is not None:
                c_start = (_ffi.BatchStart * max(count, 1))()
                for i, s in enumerate(starts):
                    if s is not None:
                        c_start[i].basis, c_start[i].nonbasis = ptr(s[0]), ptr(s[1])
            return _ffi.lib().dzg_batch_solve_post(c_lps, c_start, C.c_int64(count), C.byref(o),
                                                   C.c_int64(int(pivots_per_launch)),
                                                   C.c_int64(int(refactor_every)), C.byref(c_post), res)
        return _batch_fast(lps, log, log_cap, opts, "dzg_batch_solve_post", invoke_post,
                           post=(bool(duals), ranging if want_ranging else None, float(pivot_tol), bool(rays)))
    if start is None:
        def invoke(c_lps, count, o, res):
            return _ffi.lib().dzg_batch_solve_fast(c_lps, C.c_int64(count), C.byref(o),
                                                   C.c_int64(int(pivots_per_launch)),
                                                   C.c_int64(int(refactor_every)), res)
        return _batch_fast(lps, log, log_cap, opts, "dzg_batch_solve_fast", invoke)
    starts = _batch_starts(lps, start)

    def invoke_from(c_lps, count, o, res):
        c_start = (_ffi.BatchStart * max(count, 1))()
        for i, s in enumerate(starts):
            if s is not None:
                c_start[i].basis, c_start[i].nonbasis = ptr(s[0]), ptr(s[1])
        return _ffi.lib().dzg_batch_solve_fast_from(c_lps, c_start, C.c_int64(count), C.byref(o),
                                                    C.c_int64(int(pivots_per_launch)),
                                                    C.c_int64(int(refactor_every)), res)
    return _batch_fast(lps, log, log_cap, opts, "dzg_batch_solve_fast_from", invoke_from)


class _PostBuffers:
    """The dzg_batch_post of one call over `lps` and the arrays it points at; attach(i, result)
    sets result i's .duals / .ranging / .ray as solve_batch does."""

    def __init__(self, lps, duals: bool, ranging, pivot_tol: float, rays: bool):
        count = len(lps)
        self.mo = np.concatenate([[0], np.cumsum([lp.m for lp in lps])]).astype(np.int64)
        self.no = np.concatenate([[0], np.cumsum([lp.n for lp in lps])]).astype(np.int64)
        self.c_post = _ffi.BatchPost()
        self.bufs = self.du = self.ry = None
        if ranging is not None:
            duals = True
            reqs = [(None, None)] * count if ranging is True else list(ranging)
            if len(reqs) != count:
                raise ValueError("ranging: one (cost_dirs, rhs_dirs) request per LP")
            self.bufs = [_ffi.RangingBuffers(_ranging_dirs(cd, lp.n), _ranging_dirs(rd, lp.m), pivot_tol)
                         for (cd, rd), lp in zip(reqs, lps)]
            self.c_req, self.c_rg = (_ffi.RangingReq * max(count, 1))(), (_ffi.Ranging * max(count, 1))()
            for i, buf in enumerate(self.bufs):
                buf.fill(self.c_req[i], self.c_rg[i])
            self.c_post.req = C.addressof(self.c_req)
            self.c_post.rg = C.addressof(self.c_rg)
        if duals:
            self.y_all, self.d_all = np.zeros(self.mo[-1] + 1), np.zeros(self.no[-1] + 1)
            self.du = (_ffi.Duals * max(count, 1))()
            for i in range(count):
                self.du[i].y = self.y_all.ctypes.data + 8 * int(self.mo[i])
                self.du[i].d = self.d_all.ctypes.data + 8 * int(self.no[i])
            self.c_post.du = C.addressof(self.du)
        if rays:
            self.rd_all, self.ry_all = np.zeros(self.no[-1] + 1), np.zeros(self.mo[-1] + 1)
            self.ry = (_ffi.Ray * max(count, 1))()
            for i in range(count):
                self.ry[i].d = self.rd_all.ctypes.data + 8 * int(self.no[i])
                self.ry[i].y = self.ry_all.ctypes.data + 8 * int(self.mo[i])
            self.c_post.ry = C.addressof(self.ry)

    def attach(self, i: int, out) -> None:
        a0, a1, v0, v1 = int(self.mo[i]), int(self.mo[i + 1]), int(self.no[i]), int(self.no[i + 1])
        if self.du is not None:
            out.duals = None if self.du[i].source == 0 else _core_duals(
                self.du[i], self.y_all[a0:a1].copy(), self.d_all[v0:v1].copy())
        if self.bufs is not None:
            out.ranging = None if out.duals is None else _core_ranging(self.bufs[i], out.duals)
        if self.ry is not None:
            out.ray = None if self.ry[i].kind == 0 else _core_ray(
                self.ry[i], self.rd_all[v0:v1].copy(), self.ry_all[a0:a1].copy())


def _batch_fast(lps, log, log_cap, opts, name, invoke, post=None) -> list:
    """The Python-side checks, the marshalling and the results of a FAST batch entry point `name`;
    invoke(c_lps, count, opts, res) makes the call and returns its code.  post = (duals, ranging,
    pivot_tol, rays): invoke gets the dzg_batch_post as a fifth argument."""
    import time

    for i, lp in enumerate(lps):
        if lp.block is not None:
            raise ValueError(f"lps[{i}]: a column-block LP cannot be batched")
        if lp.a is None and lp.n_struct > 0:
            raise ValueError(f"lps[{i}]: CSC input cannot be batched (dense `a` only)")
        if lp.m > _ffi.BATCH_MAX_ROWS:
            raise ValueError(f"lps[{i}]: {lp.m} rows; the batch takes at most {_ffi.BATCH_MAX_ROWS}")
    marshalled = [_c_lp(lp) for lp in lps]
    count = len(lps)
    c_lps = (_ffi.Lp * max(count, 1))(*[c for c, _ in marshalled])
    mo = np.concatenate([[0], np.cumsum([lp.m for lp in lps])]).astype(np.int64)
    qo = np.concatenate([[0], np.cumsum([lp.n - lp.m for lp in lps])]).astype(np.int64)
    basis, x, xbar = np.zeros(mo[-1] + 1, np.int64), np.zeros(mo[-1] + 1), np.zeros(mo[-1] + 1)
    nonbasis, z, zbar = np.zeros(qo[-1] + 1, np.int64), np.zeros(qo[-1] + 1), np.zeros(qo[-1] + 1)
    cap = int(log_cap) if log else 0
    logs = np.zeros((count, max(cap, 1)), dtype=_PIVOT_DTYPE)
    margins = np.full((count, max(cap, 1)), np.inf)
    res = (_ffi.Result * max(count, 1))()
    for i in range(count):
        r = res[i]
        r.basis = basis.ctypes.data + 8 * int(mo[i])
        r.x = x.ctypes.data + 8 * int(mo[i])
        r.xbar = xbar.ctypes.data + 8 * int(mo[i])
        r.nonbasis = nonbasis.ctypes.data + 8 * int(qo[i])
        r.z = z.ctypes.data + 8 * int(qo[i])
        r.zbar = zbar.ctypes.data + 8 * int(qo[i])
        r.log = logs.ctypes.data + logs.strides[0] * i if cap > 0 else None
        r.margins = margins.ctypes.data + margins.strides[0] * i if cap > 0 else None
        r.log_cap = cap
    o = _ffi.default_opts(**opts)
    pb = _PostBuffers(lps, *post) if post is not None else None
    t0 = time.perf_counter()
    rc = invoke(c_lps, count, o, res, pb.c_post) if pb else invoke(c_lps, count, o, res)
    wall_ms = (time.perf_counter() - t0) * 1e3
    _ffi.check(rc, name)
    out = []
    for i in range(count):
        r = res[i]
        cnt = int(min(r.iterations, cap))
        arr = logs[i, :cnt]
        pivots = list(zip(arr["kind"].tolist(), arr["entering"].tolist(), arr["leaving"].tolist(),
                          arr["mu"].tolist()))
        a0, a1, b0, b1 = int(mo[i]), int(mo[i + 1]), int(qo[i]), int(qo[i + 1])
        fast = r.numerics_used != STRICT
        out.append(CoreResult(
            status=STATUS_NAMES.get(r.status, str(r.status)), status_code=r.status,
            numerics="fast" if fast else "strict", iterations=int(r.iterations), objective=float(r.objective),
            basis=basis[a0:a1].copy(), nonbasis=nonbasis[b0:b1].copy(), x=x[a0:a1].copy(),
            xbar=xbar[a0:a1].copy(), z=z[b0:b1].copy(), zbar=zbar[b0:b1].copy(), pivots=pivots,
            solve_ms=wall_ms, margins=margins[i, :cnt].copy() if fast and log else None, **_counters(r)))
        if pb:
            pb.attach(i, out[-1])
    return out


class BatchSolver:
    """dzg_batch: a batch of small LPs kept on the GPU between solves, the batched sibling of
    Solver.reoptimize.  The matrices go up once; update() / update_many() change right-hand sides
    (by constraint row), costs (by variable) and constants, and solve() re-solves the LPs it lists,
    each from the basis its last solve ended on (cold before the first solve and after one that ended
    singular or panicked; set_start overrides).  A solve is, result for result and bit for bit,
    solve_batch_fast(lps_now, start=last results) -- with numerics=STRICT, solve_batch's.

    lps: dense CoreLPs of at most 128 rows in slack-basis form.  log_cap: pivots of log kept per LP
    and solve.  opts: fields of dzg_opts with solve_batch_fast's meaning (numerics STRICT, FAST or AUTO,
    the default; near_tie_action, tie_tol, max_iter, epsilon, device).  ValueError for anything the
    host checks refuse, before a byte goes to the device."""

    def __init__(self, lps, log_cap: int = 4096, pivots_per_launch: int = 0, refactor_every: int = 0, **opts):
        lps = list(lps)
        if opts.get("numerics", AUTO) not in (STRICT, FAST, AUTO):
            raise ValueError("BatchSolver: numerics is STRICT, FAST or AUTO")
        try:
            o = _ffi.default_opts(**opts)
        except TypeError as exc:
            raise ValueError(f"BatchSolver: {exc}") from None
        if int(pivots_per_launch) < 0 or int(refactor_every) < 0 or int(log_cap) < 0:
            raise ValueError("BatchSolver: pivots_per_launch, refactor_every and log_cap are >= 0")
        for i, lp in enumerate(lps):
            if lp.block is not None:
                raise ValueError(f"lps[{i}]: a column-block LP cannot be batched")
            if lp.a is None and lp.n_struct > 0:
                raise ValueError(f"lps[{i}]: CSC input cannot be batched (dense `a` only)")
            if lp.m > _ffi.BATCH_MAX_ROWS:
                raise ValueError(f"lps[{i}]: {lp.m} rows; the batch takes at most {_ffi.BATCH_MAX_ROWS}")
            if lp.xbar is not None or lp.zbar is not None:
                raise ValueError(f"lps[{i}]: xbar / zbar given; a resident LP is given in slack-basis form")
        self._h = None
        self._shapes = [(lp.m, lp.n) for lp in lps]
        self._lps = [_ShapeOnly(lp) for lp in lps]      # what _batch_starts reads of an LP
        self._log_cap = int(log_cap)
        marshalled = [_c_lp(lp) for lp in lps]
        count = len(lps)
        c_lps = (_ffi.Lp * max(count, 1))(*[c for c, _ in marshalled])
        h = C.c_void_p()
        rc = _ffi.lib().dzg_batch_create(c_lps, C.c_int64(count), C.byref(o), C.c_int64(int(pivots_per_launch)),
                                         C.c_int64(int(refactor_every)), C.c_int64(self._log_cap), C.byref(h))
        if rc == _ffi.E_ARG:   # the host checks, as the other batch entry points raise them
            raise ValueError(f"dzg_batch_create: {_ffi.lib().dzg_last_error().decode()}")
        _ffi.check(rc, "dzg_batch_create")
        self._h = h

    def __len__(self) -> int:
        return len(self._shapes)

    def _handle(self):
        if self._h is None:
            raise ValueError("BatchSolver: the handle is closed")
        return self._h

    def _index(self, i, what: str) -> int:
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)):
            raise ValueError(f"{what}: an LP is named by its index in the batch, not {i!r}")
        if not 0 <= int(i) < len(self._shapes):
            raise ValueError(f"{what}: LP {int(i)} out of range (the batch holds {len(self._shapes)})")
        return int(i)

    def update(self, i: int, b=None, c=None, constant=None) -> None:
        """LP i's right-hand side (m, by constraint row), costs (n, by variable) and / or constant from
        its next solve on."""
        self.update_many([(i, b, c, constant)])

    def update_many(self, changes) -> None:
        """update() for several LPs in one call: (i, b, c, constant) tuples, None = keep.  An LP is
        listed once per call.  ValueError, and nothing changed, for a bad entry."""
        h = self._handle()
        changes = [tuple(ch) + (None,) * (4 - len(tuple(ch))) for ch in changes]
        keep, seen = [], set()
        chg = (_ffi.BatchChange * max(len(changes), 1))()
        for k, (i, b, c, constant) in enumerate(changes):
            i = self._index(i, f"changes[{k}]")
            if i in seen:
                raise ValueError(f"changes[{k}]: LP {i} listed twice")
            seen.add(i)
            m, n = self._shapes[i]
            if b is None and c is None and constant is None:
                raise ValueError(f"changes[{k}]: LP {i}: no b, no c, no constant")
            chg[k].lp = i
            for name, arr, size in (("b", b, m), ("c", c, n)):
                if arr is None:
                    continue
                arr = f64(arr)
                if arr.shape != (size,):
                    raise ValueError(f"changes[{k}]: LP {i}: {name} has {arr.size} entries, the LP {size}")
                bad = np.flatnonzero(~np.isfinite(arr))
                if bad.size:
                    raise ValueError(f"changes[{k}]: LP {i}: {name}[{int(bad[0])}] is not finite")
                keep.append(arr)
                setattr(chg[k], "rhs" if name == "b" else "c", arr.ctypes.data)
            if constant is not None:
                if not np.isfinite(float(constant)):
                    raise ValueError(f"changes[{k}]: LP {i}: constant is not finite")
                chg[k].constant, chg[k].set_constant = float(constant), 1
        rc = _ffi.lib().dzg_batch_update(h, chg, C.c_int64(len(changes)))
        if rc == _ffi.E_ARG:
            raise ValueError(f"dzg_batch_update: {_ffi.lib().dzg_last_error().decode()}")
        _ffi.check(rc, "dzg_batch_update")

    def set_start(self, i: int, start) -> None:
        """The basis LP i starts its next solve from: None (cold), a CoreResult (one that ended singular
        or panicked counts as None) or a (basis, nonbasis) pair."""
        h = self._handle()
        i = self._index(i, "set_start")
        starts = [None] * len(self._lps)
        starts[i] = start
        try:
            s = _batch_starts(self._lps, starts)[i]
        except ValueError as exc:
            raise ValueError(str(exc).replace(f"start[{i}]", f"set_start({i})")) from None
        if s is None:
            rc = _ffi.lib().dzg_batch_set_start(h, C.c_int64(i), None, None)
        else:
            rc = _ffi.lib().dzg_batch_set_start(h, C.c_int64(i), ptr(s[0]), ptr(s[1]))
        if rc == _ffi.E_ARG:
            raise ValueError(f"dzg_batch_set_start: {_ffi.lib().dzg_last_error().decode()}")
        _ffi.check(rc, "dzg_batch_set_start")

    def solve(self, which=None, log: bool = True, duals: bool = False, ranging=False, pivot_tol: float = 0.0,
              rays: bool = False) -> list:
        """Solve the LPs `which` lists (None: all, in index order); result k is LP which[k]'s
        CoreResult, as solve_batch_fast reports it.  duals, ranging (True, or one (cost_dirs, rhs_dirs)
        per listed LP), pivot_tol and rays (dzg_batch_resolve_post) mean what they mean for
        solve_batch_fast: results gain .duals, .ranging and .ray, None where none was computed.
        Without them the call is dzg_batch_resolve, exactly as before."""
        import time
        from types import SimpleNamespace

        want_ranging = ranging is not False and ranging is not None
        if not (0.0 <= float(pivot_tol)):
            raise ValueError("BatchSolver.solve: pivot_tol is >= 0 (0 selects 1e-9)")

        h = self._handle()
        if which is None:
            ids = list(range(len(self._shapes)))
        else:
            ids = [self._index(i, f"which[{k}]") for k, i in enumerate(which)]
            if len(set(ids)) != len(ids):
                dup = next(i for k, i in enumerate(ids) if i in ids[:k])
                raise ValueError(f"which: LP {dup} listed twice")
        count = len(ids)
        mo = np.concatenate([[0], np.cumsum([self._shapes[i][0] for i in ids])]).astype(np.int64)
        qo = np.concatenate([[0], np.cumsum([self._shapes[i][1] - self._shapes[i][0] for i in ids])]).astype(np.int64)
        basis, x, xbar = np.zeros(mo[-1] + 1, np.int64), np.zeros(mo[-1] + 1), np.zeros(mo[-1] + 1)
        nonbasis, z, zbar = np.zeros(qo[-1] + 1, np.int64), np.zeros(qo[-1] + 1), np.zeros(qo[-1] + 1)
        cap = self._log_cap if log else 0
        logs = np.zeros((count, max(cap, 1)), dtype=_PIVOT_DTYPE)
        margins = np.full((count, max(cap, 1)), np.inf)
        res = (_ffi.Result * max(count, 1))()
        for k in range(count):
            r = res[k]
            r.basis = basis.ctypes.data + 8 * int(mo[k])
            r.x = x.ctypes.data + 8 * int(mo[k])
            r.xbar = xbar.ctypes.data + 8 * int(mo[k])
            r.nonbasis = nonbasis.ctypes.data + 8 * int(qo[k])
            r.z = z.ctypes.data + 8 * int(qo[k])
            r.zbar = zbar.ctypes.data + 8 * int(qo[k])
            r.log = logs.ctypes.data + logs.strides[0] * k if cap > 0 else None
            r.margins = margins.ctypes.data + margins.strides[0] * k if cap > 0 else None
            r.log_cap = cap
        c_which = i64(ids)
        pb = None
        if duals or want_ranging or rays:
            pb = _PostBuffers([SimpleNamespace(m=self._shapes[i][0], n=self._shapes[i][1]) for i in ids], bool(duals),
                              ranging if want_ranging else None, float(pivot_tol), bool(rays))
        t0 = time.perf_counter()
        if pb is None:
            rc = _ffi.lib().dzg_batch_resolve(h, None if which is None else ptr(c_which), C.c_int64(count), res)
        else:
            rc = _ffi.lib().dzg_batch_resolve_post(h, None if which is None else ptr(c_which), C.c_int64(count),
                                                   C.byref(pb.c_post), res)
        wall_ms = (time.perf_counter() - t0) * 1e3
        if rc == _ffi.E_ARG:
            raise ValueError(f"dzg_batch_resolve: {_ffi.lib().dzg_last_error().decode()}")
        _ffi.check(rc, "dzg_batch_resolve")
        out = []
        for k in range(count):
            r = res[k]
            cnt = int(min(r.iterations, cap))
            arr = logs[k, :cnt]
            pivots = list(zip(arr["kind"].tolist(), arr["entering"].tolist(), arr["leaving"].tolist(),
                              arr["mu"].tolist()))
            a0, a1, b0, b1 = int(mo[k]), int(mo[k + 1]), int(qo[k]), int(qo[k + 1])
            fast = r.numerics_used != STRICT
            out.append(CoreResult(
                status=STATUS_NAMES.get(r.status, str(r.status)), status_code=r.status,
                numerics="fast" if fast else "strict", iterations=int(r.iterations), objective=float(r.objective),
                basis=basis[a0:a1].copy(), nonbasis=nonbasis[b0:b1].copy(), x=x[a0:a1].copy(),
                xbar=xbar[a0:a1].copy(), z=z[b0:b1].copy(), zbar=zbar[b0:b1].copy(), pivots=pivots,
                solve_ms=wall_ms, margins=margins[k, :cnt].copy() if fast and log else None, **_counters(r)))
            if pb:
                pb.attach(k, out[-1])
        return out

    def traffic(self) -> tuple[int, int, float]:
        """(host-to-device bytes, device-to-host bytes, stage + restart device ms) of the last solve()."""
        nbytes, ms = (C.c_int64 * 2)(), (C.c_double * 1)()
        _ffi.check(_ffi.lib().dzg_debug_batch_traffic(self._handle(), nbytes, ms), "dzg_debug_batch_traffic")
        return int(nbytes[0]), int(nbytes[1]), float(ms[0])

    def close(self) -> None:
        if self._h is not None:
            _ffi.lib().dzg_batch_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ShapeOnly:
    """What BatchSolver keeps of a CoreLP for _batch_starts: m, n and the slack-basis codes."""

    def __init__(self, lp: CoreLP):
        self.m, self.n, self.n_struct = lp.m, lp.n, lp.n_struct
        self.basis = i64(lp.basis).copy()
        self.var_col = None if lp.var_col is None else i64(lp.var_col).copy()


def core_solve_full_csc(m: int, n: int, col_ptr, row_idx, val, c, constant, basis, nonbasis, x, z,
                        log_cap: int = 1 << 16, **opts) -> CoreResult:
    """dzg_core_solve_full_csc: Level 1 on the reference's own `Simplex` fields -- ONE CSC over all n
    columns, slack columns included, 64-bit indices (src/simplex.rs:84-112, src/linalg.rs:161-168).
    The in/out arrays of the C call are copies here; the final state comes back in the result."""
    _ffi.require_gpu()
    q = n - m
    col_ptr, row_idx, val, c = i64(col_ptr), i64(row_idx), f64(val), f64(c)
    basis, nonbasis = i64(basis).copy(), i64(nonbasis).copy()
    x, z = f64(x).copy(), f64(z).copy()
    if len(row_idx) == 0:
        row_idx, val = np.zeros(1, np.int64), np.zeros(1)
    xbar, zbar = np.zeros(max(m, 1)), np.zeros(max(q, 1))
    buf = (_ffi.Pivot * max(log_cap, 1))()
    margins = np.full(max(log_cap, 1), np.inf)
    r = _ffi.Result()
    r.xbar, r.zbar = ptr(xbar), ptr(zbar)
    r.log, r.log_cap, r.margins = C.cast(buf, C.c_void_p), log_cap, ptr(margins)
    o = _ffi.default_opts(**opts)
    rc = _ffi.lib().dzg_core_solve_full_csc(
        int(m), int(n), ptr(col_ptr), ptr(row_idx), ptr(val), ptr(c), float(constant),
        ptr(basis if m else np.zeros(1, np.int64)), ptr(nonbasis if q else np.zeros(1, np.int64)),
        ptr(x if m else np.zeros(1)), ptr(z if q else np.zeros(1)), C.byref(o), C.byref(r))
    _ffi.check(rc, "dzg_core_solve_full_csc")
    cnt = int(min(r.iterations, log_cap))
    arr = np.ctypeslib.as_array(buf)[:cnt]
    pivots = list(zip(arr["kind"].tolist(), arr["entering"].tolist(), arr["leaving"].tolist(),
                      arr["mu"].tolist()))
    return CoreResult(
        status=STATUS_NAMES.get(r.status, str(r.status)), status_code=r.status,
        numerics="strict" if r.numerics_used == STRICT else "fast",
        iterations=int(r.iterations), objective=float(r.objective),
        basis=basis[:m], nonbasis=nonbasis[:q], x=x[:m], xbar=xbar[:m].copy(), z=z[:q],
        zbar=zbar[:q].copy(), pivots=pivots, margins=margins[:cnt].copy(), **_counters(r))


# ------------------------------------------------------------------ synthetic LPs
def gen_dense_lp(seed: int, m: int, n_struct: int):
    """Generator G1.  Returns (A as an (m, n_struct) Fortran-ordered array, b, c)."""
    a = np.empty((n_struct, m), dtype=np.float64)  # C-contiguous (ns, m) == column-major m x ns
    b = np.empty(m)
    c = np.empty(n_struct)
    rc = _ffi.lib().dzg_gen_dense_lp(C.c_uint64(seed), m, n_struct, ptr(a), m, ptr(b), ptr(c))
    _ffi.check(rc, "dzg_gen_dense_lp")
    return a.T, b, c


def gen_dense_lp_block(seed: int, m: int, n_struct: int, begin: int, end: int):
    """Generator G1, columns [begin, end) of A only (bit-identical to that slice of
    gen_dense_lp); b and c are complete.  Returns (A block (m, end-begin), b, c)."""
    a = np.empty((max(end - begin, 1), m), dtype=np.float64)
    b = np.empty(m)
    c = np.empty(n_struct)
    rc = _ffi.lib().dzg_gen_dense_lp_block(C.c_uint64(seed), m, n_struct, begin, end, ptr(a), m,
                                           ptr(b), ptr(c))
    _ffi.check(rc, "dzg_gen_dense_lp_block")
    return a[:end - begin].T, b, c


def gen_sparse_lp(seed: int, m: int, n_struct: int, per_col: int):
    """Generator G2.  Returns (col_ptr, row_idx, val, b, c) with `per_col` nonzeros per column."""
    col_ptr = np.zeros(n_struct + 1, dtype=np.int64)
    row_idx = np.zeros(n_struct * per_col, dtype=np.int32)
    val = np.zeros(n_struct * per_col)
    b, c = np.empty(m), np.empty(n_struct)
    rc = _ffi.lib().dzg_gen_sparse_lp(C.c_uint64(seed), C.c_int64(m), C.c_int64(n_struct),
                                      C.c_int64(per_col), ptr(col_ptr), ptr(row_idx), ptr(val),
                                      ptr(b), ptr(c))
    _ffi.check(rc, "dzg_gen_sparse_lp")
    return col_ptr, row_idx, val, b, c


# ------------------------------------------------------------------ single reference functions
def lu_solve(a: np.ndarray, b: np.ndarray, device: int = 0):
    """lu_solve (src/linalg.rs:8-10) on the GPU.  Returns (x, packed LU, pivots)."""
    _ffi.require_gpu()
    a, b = f64(a), f64(b)
    n = a.shape[0]
    x, lu, p = np.empty(n), np.empty((n, n)), np.zeros(max(n - 1, 1), np.int64)
    rc = _ffi.lib().dzg_kernel_lu_solve(C.c_int64(n), ptr(a), ptr(b), ptr(x), ptr(lu), ptr(p),
                                        C.c_int32(device))
    _ffi.check(rc, "dzg_kernel_lu_solve")
    return x, lu, p[: n - 1]


def neg_t_dot(a: np.ndarray, cols, v, kernel: int = PRICE_SEQ, device: int = 0) -> np.ndarray:
    """collect_columns(cols).neg_t_dot(v) (src/linalg.rs:188-207) on the GPU, a is (m, ns)."""
    _ffi.require_gpu()
    a = np.asarray(a, dtype=np.float64)
    m, ns = a.shape
    a_cm = np.ascontiguousarray(a.T)
    cols, v = i64(cols), f64(v)
    out = np.empty(max(len(cols), 1))
    rc = _ffi.lib().dzg_kernel_neg_t_dot(C.c_int64(m), C.c_int64(ns), ptr(a_cm), C.c_int64(m),
                                         ptr(cols), C.c_int64(len(cols)), ptr(v), ptr(out),
                                         C.c_int32(kernel), C.c_int32(device))
    _ffi.check(rc, "dzg_kernel_neg_t_dot")
    return out[: len(cols)]


def neg_t_dot_csc(m: int, col_ptr, row_idx, val, cols, v, device: int = 0) -> np.ndarray:
    """neg_t_dot over a CSC matrix kept sparse on the device (k_price_csc)."""
    _ffi.require_gpu()
    col_ptr, cols, v, val = i64(col_ptr), i64(cols), f64(v), f64(val)
    row_idx = np.ascontiguousarray(row_idx, dtype=np.int32)
    out = np.empty(max(len(cols), 1))
    rc = _ffi.lib().dzg_kernel_neg_t_dot_csc(
        C.c_int64(m), C.c_int64(len(col_ptr) - 1), ptr(col_ptr), ptr(row_idx), ptr(val), ptr(cols),
        C.c_int64(len(cols)), ptr(v), ptr(out), C.c_int32(device))
    _ffi.check(rc, "dzg_kernel_neg_t_dot_csc")
    return out[: len(cols)]


def first_pivot(y, ybar, device: int = 0) -> int:
    _ffi.require_gpu()
    y, ybar = f64(y), f64(ybar)
    out = C.c_int64(-1)
    rc = _ffi.lib().dzg_kernel_first_pivot(C.c_int64(len(y)), ptr(y), ptr(ybar), C.byref(out),
                                           C.c_int32(device))
    _ffi.check(rc, "dzg_kernel_first_pivot")
    return int(out.value)


def second_pivot(mu, y, ybar, dy, device: int = 0) -> int:
    _ffi.require_gpu()
    y, ybar, dy = f64(y), f64(ybar), f64(dy)
    out = C.c_int64(-1)
    rc = _ffi.lib().dzg_kernel_second_pivot(C.c_int64(len(y)), C.c_double(mu), ptr(y), ptr(ybar),
                                            ptr(dy), C.byref(out), C.c_int32(device))
    _ffi.check(rc, "dzg_kernel_second_pivot")
    return int(out.value)


def merge_candidates(cands) -> int:
    """cands: iterable of (ratio, pos, y, ybar, dy); pos < 0 means empty."""
    arr = (_ffi.Candidate * max(len(cands), 1))()
    for i, (r, p, y, yb, dy) in enumerate(cands):
        arr[i] = _ffi.Candidate(r, p if p >= 0 else (1 << 63) - 1, y, yb, dy)
    return int(_ffi.lib().dzg_merge_candidates(arr, C.c_int64(len(cands))))


def debug_batch_fast_inverse(lps, pivots: int, refactor_every: int = 0, log: bool = True,
                             log_cap: int = 4096, **opts) -> list:
    """Test hook (dzg_debug_batch_fast_inverse): what one launch of the FAST batch kernel keeps in LDS.
    Every LP's inverse W is built from its starting basis, at most `pivots` pivots run (refactor_every
    as in solve_batch_fast; above `pivots`: no rebuild inside the launch), and LP i comes back as
    (CoreResult, W): the result as solve_batch_fast reports it ("iter_limit" if the budget ended it)
    and W as an (m, m) array, row p basis position p, column r constraint row r.  FAST numerics only;
    keywords near_tie_action, tie_tol, epsilon, device."""
    lps = list(lps)
    allowed = {"numerics", "near_tie_action", "tie_tol", "epsilon", "device"}
    unknown = set(opts) - allowed
    if unknown:
        raise ValueError(f"debug_batch_fast_inverse takes {sorted(allowed)}, not {sorted(unknown)}")
    if opts.setdefault("numerics", FAST) != FAST:
        raise ValueError("debug_batch_fast_inverse: FAST numerics only")
    if int(pivots) < 0 or int(refactor_every) < 0:
        raise ValueError("debug_batch_fast_inverse: pivots and refactor_every are >= 0")
    wo = np.concatenate([[0], np.cumsum([lp.m * lp.m for lp in lps])]).astype(np.int64)
    w = np.full(int(wo[-1]) + 1, np.nan)

    def invoke(c_lps, count, o, res):
        return _ffi.lib().dzg_debug_batch_fast_inverse(c_lps, C.c_int64(count), C.byref(o), C.c_int64(int(pivots)),
                                                       C.c_int64(int(refactor_every)), ptr(w), res)
    out = _batch_fast(lps, log, log_cap, opts, "dzg_debug_batch_fast_inverse", invoke)
    return [(r, w[int(wo[i]):int(wo[i + 1])].reshape(lp.m, lp.m).copy()) for i, (r, lp) in enumerate(zip(out, lps))]
