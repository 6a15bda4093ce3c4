"""Drop-in for the reference's compiled extension module `dantzig.rust`.

The reference exposes five PyO3 classes and one function (src/lib.rs:29-38,
src/pyobjs.rs:10-175).  This module offers the same names, constructor signatures, getters
and operator behaviour, backed by the HIP engine through the C ABI
(include/dantzig_amd.h, dzg_model_solve) instead of the Rust simplex:

    Variable(*, lb, ub)            .id .lb .ub                      src/pyobjs.rs:10-38
    PyLinExpr(coefs, vars)         map_ids_to_coefs, -e, e+e, e*k   src/pyobjs.rs:40-112
    PyAffExpr(*, linexpr, constant) .pylinexpr .constant            src/pyobjs.rs:114-133
    PyInequality(*, linexpr, b)                                     src/pyobjs.rs:135-152
    PySolution                     .objective_value, [Variable]     src/pyobjs.rs:154-175
    solve(objective, constraints)  -> PySolution                    src/lib.rs:16-27

Additions of this package: Variable(..., integer=True) and solve_mip() (branch and bound,
dzg_mip_solve), set_options() / set_mip_options() for the engine's knobs, solve_many().
"""
from __future__ import annotations

import ctypes as C
import itertools
import threading
import warnings

import numpy as np

from . import _ffi
from .exceptions import InfeasibleError, MipLimitWarning, NearTieWarning, UnboundedError

_counter = itertools.count()          # static COUNTER: AtomicUsize, src/pyobjs.rs:8
_counter_lock = threading.Lock()

# options applied by solve(); see set_options()
_options: dict = {}
# options applied by solve_mip(); see set_mip_options()
_mip_options: dict = {}


def set_options(**opts) -> None:
    """Engine options for subsequent solve() calls (fields of dzg_opts), e.g.
    set_options(numerics=_ffi.STRICT).  The reference has no such knob."""
    _ffi.default_opts(**opts)  # validates names
    _options.clear()
    _options.update(opts)


def set_mip_options(**opts) -> None:
    """Branch-and-bound knobs for subsequent solve_mip() calls (fields of dzg_mip_opts: node_limit,
    nodes_per_round, pivots_per_launch, int_tol, abs_gap, rel_gap, and warm_start: True starts a
    child's node LP from its parent's final basis where the two share a standard form, see
    dzg_mip_solve) and the node options of dzg_mip_solve_nodes: node_numerics="fast" solves the
    batched node LPs in FAST numerics first, each result certified from its final basis and each
    rejected attempt solved again in STRICT; fast_pivots_per_launch and refactor_every are that
    kernel's knobs -- results depend on them in the last bits."""
    search, node = _split_mip_options(opts)
    _ffi.default_mip_opts(**search)  # validates names
    _node_opts(node)
    _mip_options.clear()
    _mip_options.update(opts)


_NODE_OPTION_NAMES = {"node_numerics": "numerics", "fast_pivots_per_launch": "pivots_per_launch",
                      "refactor_every": "refactor_every"}


def _split_mip_options(opts: dict):
    """(fields of dzg_mip_opts, node options by their solve_mip() names)."""
    node = {k: v for k, v in opts.items() if k in _NODE_OPTION_NAMES}
    return {k: v for k, v in opts.items() if k not in _NODE_OPTION_NAMES}, node


def _node_opts(node: dict):
    """dzg_mip_node_opts of the node options, or None when none was passed."""
    if not node:
        return None
    return _ffi.default_mip_node_opts(**{_NODE_OPTION_NAMES[k]: v for k, v in node.items()})


def _opt_float(v, what: str):
    if v is None:
        return None
    if not isinstance(v, (int, float)):
        raise TypeError(f"{what} must be a float or None")
    return float(v)


class Variable:
    __slots__ = ("_id", "_lb", "_ub", "_integer")

    def __init__(self, *, lb, ub, integer: bool = False):
        self._lb = _opt_float(lb, "lb")
        self._ub = _opt_float(ub, "ub")
        self._integer = bool(integer)
        with _counter_lock:
            self._id = next(_counter)

    id = property(lambda self: self._id)
    lb = property(lambda self: self._lb)
    ub = property(lambda self: self._ub)
    is_integer = property(lambda self: self._integer)

    def __repr__(self) -> str:
        extra = ", integer=True" if self._integer else ""
        return f"rust.Variable(id={self._id}, lb={self._lb}, ub={self._ub}{extra})"


def _check_number(k, what: str) -> float:
    if not isinstance(k, (int, float)):
        raise TypeError(f"{what} must be an int or a float")
    return float(k)


class PyLinExpr:
    """sum coef_i * var_i, terms kept in first-seen order (the order defines the LP's
    column order and therefore its tie-breaks, src/simplex.rs:168-176)."""
    __slots__ = ("coefs", "vars", "_slot")

    def __init__(self, coefs, vars):
        self.coefs = [_check_number(c, "coefficient") for c in coefs]
        self.vars = list(vars)
        if len(self.coefs) != len(self.vars):
            raise ValueError("coefs and vars differ in length")
        for v in self.vars:
            if not isinstance(v, Variable):
                raise TypeError("vars must hold rust.Variable objects")
        self._slot = {v.id: i for i, v in enumerate(self.vars)}

    def map_ids_to_coefs(self) -> dict:
        return {v.id: c for c, v in zip(self.coefs, self.vars)}

    def __neg__(self) -> "PyLinExpr":
        return PyLinExpr([-c for c in self.coefs], self.vars)

    def __add__(self, other: "PyLinExpr") -> "PyLinExpr":
        if not isinstance(other, PyLinExpr):
            return NotImplemented
        coefs, vars_ = list(self.coefs), list(self.vars)
        slot = dict(self._slot)
        for c, v in zip(other.coefs, other.vars):   # merge by id, src/pyobjs.rs:86-98
            i = slot.get(v.id)
            if i is None:
                slot[v.id] = len(vars_)
                vars_.append(v)
                coefs.append(c)
            else:
                coefs[i] += c
        out = PyLinExpr.__new__(PyLinExpr)
        out.coefs, out.vars, out._slot = coefs, vars_, slot
        return out

    def __mul__(self, constant) -> "PyLinExpr":
        k = _check_number(constant, "multiplier")
        return PyLinExpr([k * c for c in self.coefs], self.vars)


class PyAffExpr:
    __slots__ = ("_linexpr", "_constant")

    def __init__(self, *, linexpr: PyLinExpr, constant):
        if not isinstance(linexpr, PyLinExpr):
            raise TypeError("linexpr must be a PyLinExpr")
        self._linexpr = linexpr
        self._constant = _check_number(constant, "constant")

    pylinexpr = property(lambda self: self._linexpr)
    constant = property(lambda self: self._constant)


class PyInequality:
    """linexpr <= b"""
    __slots__ = ("_linexpr", "_b")

    def __init__(self, *, linexpr: PyLinExpr, b):
        if not isinstance(linexpr, PyLinExpr):
            raise TypeError("linexpr must be a PyLinExpr")
        self._linexpr = linexpr
        self._b = _check_number(b, "b")


class MipInfo:
    """What the branch and bound of solve_mip() did (core sense: maximised).  `log` is the node
    log, a list of dzg_mip_node tuples (id, parent, branch_var, direction, bound, status,
    iterations, objective) when solve_mip(..., node_log=N) asked for one.  nodes_warm counts the
    node LPs started from their parent's basis (warm_start=True), nodes_restarted those of them
    that were discarded and solved again cold.  nodes_fast_accepted / nodes_fast_rejected count the
    FAST node attempts that stood and those solved again in STRICT; both are None unless a node
    option (node_numerics, fast_pivots_per_launch, refactor_every) was passed.  With
    node_numerics="fast" nodes_warm counts only the warm attempts that FAST accepted and
    nodes_restarted is 0: a warm node that FAST rejects is solved cold in STRICT and is counted in
    nodes_fast_rejected instead."""
    __slots__ = ("status", "nodes", "rounds", "lp_iterations", "best_bound", "gap", "objective",
                 "nodes_batched", "nodes_sequential", "nodes_pruned", "nodes_dropped",
                 "incumbent_node", "failed_node", "log", "nodes_warm", "nodes_restarted",
                 "nodes_fast_accepted", "nodes_fast_rejected")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def __repr__(self) -> str:
        return (f"MipInfo(status={self.status!r}, nodes={self.nodes}, rounds={self.rounds}, "
                f"lp_iterations={self.lp_iterations}, best_bound={self.best_bound}, gap={self.gap})")


class PyDuals:
    """Duals of one solve(..., duals=True), in the core sense (the model is maximised, every row
    is linexpr <= b): con_dual[r] the dual value of inequality r in the order they were passed,
    var_rc / lb_dual / ub_dual keyed by Variable.id (dzg_model_map_duals), and the certificate
    scalars of dzg_duals with their source, "fresh" or "carried"."""
    __slots__ = ("source", "con_dual", "var_rc", "lb_dual", "ub_dual", "primal_objective",
                 "dual_objective", "primal_infeasibility", "dual_infeasibility", "z_diff")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class PyRanging:
    """Ranges of one solve(..., ranging=...), in the core sense (the model is maximised, every row is
    linexpr <= b): var_lo / var_hi keyed by Variable.id, the interval of the step t on that
    variable's objective coefficient over which the optimal basis holds; group_lo / group_hi per
    requested group of rows, the interval of the step t when every row r of the group has its b
    moved by coefficient * t.  *_var: the blocking variable of the standard form, -1 if none."""
    __slots__ = ("var_lo", "var_hi", "var_lo_var", "var_hi_var", "group_lo", "group_hi",
                 "group_lo_var", "group_hi_var")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class PyRay:
    """The ray of one solve(..., rays=True) that ended unbounded (kind "primal") or infeasible (kind
    "farkas"), in the core sense (the model is maximised, every row is linexpr <= b), as
    dzg_model_map_ray lays it out: var / lb / ub keyed by Variable.id, con[r] per inequality in the
    order they were passed.  primal: var is the direction, con / lb / ub how fast each row's slack
    grows along it, value the objective's gain per unit.  farkas: con / lb / ub are the rows'
    multipliers, var the aggregated coefficient of each variable, value the aggregated right-hand
    side.  violation and proven: dzg_ray's."""
    __slots__ = ("kind", "proven", "value", "violation", "mu", "var", "con", "lb", "ub")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class PySolution:
    __slots__ = ("_objective_value", "_values", "iterations", "numerics", "shape", "mip", "duals",
                 "ranging")

    def __init__(self, objective_value: float, values: dict, iterations: int = 0,
                 numerics: str = "", shape=(0, 0), mip: "MipInfo | None" = None,
                 duals: "PyDuals | None" = None):
        self.ranging = None             # None unless solve(..., ranging=...)
        self._objective_value = objective_value
        self._values = values
        self.iterations = iterations    # extras the reference does not expose
        self.numerics = numerics
        self.shape = shape
        self.mip = mip                  # None for an LP
        self.duals = duals              # None unless solve(..., duals=True)

    objective_value = property(lambda self: self._objective_value)

    def __getitem__(self, variable: Variable) -> float:
        return self._values.get(variable.id, 0.0)   # src/pyobjs.rs:163-165


def lower(objective: PyAffExpr, constraints):
    """Flattens the call arguments into the arrays of dzg_model.  Returns (arrays, table)."""
    table: dict = {}
    order = []

    def slot(v: Variable) -> int:
        i = table.get(v.id)
        if i is None:
            i = table[v.id] = len(order)
            order.append(v)
        return i

    le = objective.pylinexpr
    obj_var = [slot(v) for v in le.vars]
    obj_coef = list(le.coefs)
    con_ptr, con_var, con_coef, con_b = [0], [], [], []
    for ineq in constraints:
        if not isinstance(ineq, PyInequality):
            raise TypeError("constraints must hold PyInequality objects")
        for c, v in zip(ineq._linexpr.coefs, ineq._linexpr.vars):
            con_var.append(slot(v))
            con_coef.append(c)
        con_ptr.append(len(con_var))
        con_b.append(ineq._b)
    arrays = dict(
        has_lb=np.array([v.lb is not None for v in order] + [False], dtype=np.int32),
        has_ub=np.array([v.ub is not None for v in order] + [False], dtype=np.int32),
        lb=np.array([0.0 if v.lb is None else v.lb for v in order] + [0.0]),
        ub=np.array([0.0 if v.ub is None else v.ub for v in order] + [0.0]),
        obj_var=np.array(obj_var + [0], dtype=np.int64), obj_coef=np.array(obj_coef + [0.0]),
        con_ptr=np.array(con_ptr, dtype=np.int64), con_var=np.array(con_var + [0], dtype=np.int64),
        con_coef=np.array(con_coef + [0.0]), con_b=np.array(con_b + [0.0]),
        nvars=len(order), obj_nterms=len(obj_var), ncons=len(con_b),
        obj_const=objective.constant)
    return arrays, order


def _c_model(a: dict) -> _ffi.Model:
    p = _ffi.ptr
    return _ffi.Model(a["nvars"], p(a["has_lb"]), p(a["has_ub"]), p(a["lb"]), p(a["ub"]),
                      a["obj_nterms"], p(a["obj_var"]), p(a["obj_coef"]), a["obj_const"],
                      a["ncons"], p(a["con_ptr"]), p(a["con_var"]), p(a["con_coef"]), p(a["con_b"]))


class StandardForm:
    """dzg_build_standard_form of lower()'s arrays (Simplex::new, src/simplex.rs:123-224) as numpy
    arrays: a is (m, n_struct); pos_var / neg_var the variable of x+ / x- per user variable (-1: unseen)."""
    __slots__ = ("m", "n", "n_struct", "a", "var_col", "c", "constant", "basis", "nonbasis", "x", "z",
                 "pos_var", "neg_var")

    def same_shape_as(self, other: "StandardForm") -> bool:
        """Everything but b, c and the constant agrees: what a live solver can be re-optimised over."""
        return ((self.m, self.n, self.n_struct) == (other.m, other.n, other.n_struct)
                and np.array_equal(self.a, other.a) and np.array_equal(self.var_col, other.var_col)
                and np.array_equal(self.pos_var, other.pos_var) and np.array_equal(self.neg_var, other.neg_var))


def standard_form(arrays: dict) -> StandardForm:
    """The standard form of a lowered model, built on the host by the library (two-call protocol)."""
    md = _c_model(arrays)
    sf = _ffi.StdForm()
    _ffi.check(_ffi.lib().dzg_build_standard_form(C.byref(md), C.byref(sf)), "dzg_build_standard_form")
    m, n, nst, nv = int(sf.m), int(sf.n), int(sf.n_struct), int(arrays["nvars"])
    a = np.zeros((max(nst, 1), max(int(sf.lda), 1)))
    var_col, c = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1))
    basis, nonbasis = np.zeros(max(m, 1), np.int64), np.zeros(max(n - m, 1), np.int64)
    x, z = np.zeros(max(m, 1)), np.zeros(max(n - m, 1))
    pos, neg = np.zeros(nv + 1, np.int64), np.zeros(nv + 1, np.int64)
    p = _ffi.ptr
    sf.a, sf.var_col, sf.c, sf.basis, sf.nonbasis = p(a), p(var_col), p(c), p(basis), p(nonbasis)
    sf.x, sf.z, sf.pos_var, sf.neg_var = p(x), p(z), p(pos), p(neg)
    _ffi.check(_ffi.lib().dzg_build_standard_form(C.byref(md), C.byref(sf)), "dzg_build_standard_form")
    out = StandardForm()
    out.m, out.n, out.n_struct, out.constant = m, n, nst, float(sf.constant)
    out.a = np.ascontiguousarray(a[:nst, :m].T)
    out.var_col, out.c = var_col[:n].copy(), c[:n].copy()
    out.basis, out.nonbasis = basis[:m].copy(), nonbasis[:n - m].copy()
    out.x, out.z = x[:m].copy(), z[:n - m].copy()
    out.pos_var, out.neg_var = pos[:nv].copy(), neg[:nv].copy()
    return out


class _DualBuffers:
    """The caller-owned arrays of one dzg_model_duals and the struct that points at them."""

    def __init__(self, arrays: dict):
        nv, nc = arrays["nvars"], arrays["ncons"]
        self.con_dual, self.var_rc = np.zeros(max(nc, 1)), np.zeros(max(nv, 1))
        self.lb_dual, self.ub_dual = np.zeros(max(nv, 1)), np.zeros(max(nv, 1))
        self.ncons = nc

    def fill(self, c: "_ffi.ModelDuals") -> None:
        c.con_dual, c.var_rc = _ffi.ptr(self.con_dual), _ffi.ptr(self.var_rc)
        c.lb_dual, c.ub_dual = _ffi.ptr(self.lb_dual), _ffi.ptr(self.ub_dual)

    def pyduals(self, c: "_ffi.ModelDuals", order) -> "PyDuals | None":
        core = c.core
        if core.source == 0:
            return None
        by_id = lambda a: {v.id: float(a[i]) for i, v in enumerate(order)}  # noqa: E731
        return PyDuals(source=_ffi.DUALS_SOURCE_NAMES[int(core.source)],
                       con_dual=[float(v) for v in self.con_dual[:self.ncons]],
                       var_rc=by_id(self.var_rc), lb_dual=by_id(self.lb_dual), ub_dual=by_id(self.ub_dual),
                       primal_objective=float(core.primal_obj), dual_objective=float(core.dual_obj),
                       primal_infeasibility=float(core.primal_infeas),
                       dual_infeasibility=float(core.dual_infeas), z_diff=float(core.z_diff))


class _RayBuffers:
    """The caller-owned arrays of one dzg_model_ray and the struct that points at them."""

    def __init__(self, arrays: dict):
        nv, nc = arrays["nvars"], arrays["ncons"]
        self.var, self.con = np.zeros(max(nv, 1)), np.zeros(max(nc, 1))
        self.lb, self.ub = np.zeros(max(nv, 1)), np.zeros(max(nv, 1))
        self.ncons = nc

    def fill(self, c: "_ffi.ModelRay") -> None:
        c.var, c.con = _ffi.ptr(self.var), _ffi.ptr(self.con)
        c.lb, c.ub = _ffi.ptr(self.lb), _ffi.ptr(self.ub)

    def pyray(self, c: "_ffi.ModelRay", order) -> "PyRay | None":
        core = c.core
        if core.kind == 0:
            return None
        by_id = lambda a: {v.id: float(a[i]) for i, v in enumerate(order)}  # noqa: E731
        return PyRay(kind="primal" if core.kind == _ffi.RAY_PRIMAL else "farkas", proven=bool(core.proven),
                     value=float(core.value), violation=float(core.violation), mu=float(core.mu),
                     var=by_id(self.var), con=[float(v) for v in self.con[:self.ncons]],
                     lb=by_id(self.lb), ub=by_id(self.ub))


class _RangingBuffers:
    """One dzg_model_ranging_req over every variable of the lowered model and the given groups of
    rows (True: every inequality by itself), with the dzg_ranging it fills."""

    def __init__(self, arrays: dict, order, groups, pivot_tol: float = 0.0):
        if groups is True:
            groups = [[(r, 1.0)] for r in range(arrays["ncons"])]
        self.groups = [list(g) for g in groups]
        self.buf = _ffi.RangingBuffers([{}] * len(order), [{}] * len(self.groups), pivot_tol)
        self.var = _ffi.i64(list(range(len(order))) + [0])
        ptr_, idx, coef = [0], [], []
        for g in self.groups:
            for r, k in g:
                idx.append(int(r))
                coef.append(float(k))
            ptr_.append(len(idx))
        self.row_ptr, self.row_idx = _ffi.i64(ptr_), _ffi.i64(idx + [0])
        self.row_coef = _ffi.f64(coef + [0.0])
        self.nvar, self.pivot_tol = len(order), float(pivot_tol)

    def fill(self, req: "_ffi.ModelRangingReq", out: "_ffi.Ranging") -> None:
        req.nvar, req.var = self.nvar, _ffi.ptr(self.var)
        req.nrow, req.row_ptr = len(self.groups), _ffi.ptr(self.row_ptr)
        req.row_idx, req.row_coef = _ffi.ptr(self.row_idx), _ffi.ptr(self.row_coef)
        req.pivot_tol = self.pivot_tol
        self.buf.fill_out(out)

    def pyranging(self, order) -> PyRanging:
        c, r = self.buf.side(0), self.buf.side(1)
        by_id = lambda a, cast: {v.id: cast(a[i]) for i, v in enumerate(order)}  # noqa: E731
        return PyRanging(var_lo=by_id(c[0], float), var_hi=by_id(c[1], float),
                         var_lo_var=by_id(c[2], int), var_hi_var=by_id(c[3], int),
                         group_lo=[float(v) for v in r[0]], group_hi=[float(v) for v in r[1]],
                         group_lo_var=[int(v) for v in r[2]], group_hi_var=[int(v) for v in r[3]])


def _outcome(res, values, order, where: str = "", stacklevel: int = 4):
    """The PySolution of one dzg_model_result, or the exception the reference raises for it."""
    rc = int(res.status)
    if rc == _ffi.UNBOUNDED:
        return UnboundedError("The objective is unbounded" + where)      # src/lib.rs:24
    if rc == _ffi.INFEASIBLE:
        return InfeasibleError("The model is infeasible" + where)        # src/lib.rs:25
    if rc != _ffi.OPTIMAL:
        # PANIC / ITER_LIMIT / SINGULAR: the reference would panic (PanicException) or recurse
        return RuntimeError(f"simplex terminated with status {_ffi.status_str(rc)!r} after "
                            f"{res.iterations} iterations{where}")
    if res.near_ties > 0 and res.numerics_used != _ffi.STRICT:
        warnings.warn(
            f"{res.near_ties} of {res.iterations} pivots (the first: pivot {res.first_near_tie}) were "
            "decided within rounding distance of a tie and the model is too large to be re-solved "
            "in the reference's own arithmetic: the optimum is valid, but the vertex may differ "
            f"from the one the reference implementation reports when the optimum is not unique{where}",
            NearTieWarning, stacklevel=stacklevel)
    return PySolution(float(res.objective), {v.id: float(values[i]) for i, v in enumerate(order)},
                      int(res.iterations), "strict" if res.numerics_used == _ffi.STRICT else "fast",
                      (int(res.m), int(res.n)))


def _want_ranging(ranging) -> bool:
    return ranging is not False and ranging is not None


def solve(objective: PyAffExpr, constraints, duals: bool = False, ranging=False,
          pivot_tol: float = 0.0, rays: bool = False) -> PySolution:
    """Maximise `objective` subject to `constraints` on the GPU (src/lib.rs:16-27).  duals=True
    (dzg_model_solve_duals): the same solution with .duals, a PyDuals.  ranging=True, or a list of
    groups [(row, coefficient), ...] of inequalities (dzg_model_solve_ranging): also .ranging, a
    PyRanging over every variable and every group (True: every inequality by itself); implies
    duals.  NotImplementedError when the solve ends on a route without ranging (CSC storage).
    rays=True (dzg_model_solve_rays; composes with duals, not with ranging): the UnboundedError or
    InfeasibleError this raises carries .ray, a PyRay (None on a route without rays)."""
    if not isinstance(objective, PyAffExpr):
        raise TypeError("objective must be a PyAffExpr")
    constraints = list(constraints)
    want_ranging = _want_ranging(ranging)
    if rays and want_ranging:
        raise ValueError("rays=True and ranging: the ranging call carries no ray; ask in two calls")
    if rays and _has_integer(objective, constraints):
        raise ValueError("rays=True: rays are not defined for a model with integer variables")
    if want_ranging and _has_integer(objective, constraints):
        raise ValueError("ranging=True: ranges are not defined for a model with integer variables")
    duals = duals or want_ranging
    if duals and _has_integer(objective, constraints):
        raise ValueError("duals=True: dual values are not defined for a model with integer variables")
    arrays, order = lower(objective, constraints)
    _ffi.require_gpu()
    values = np.zeros(max(len(order), 1))
    res = _ffi.ModelResult()
    res.values = _ffi.ptr(values)
    opts = _ffi.default_opts(**_options)
    md = _c_model(arrays)
    if duals:
        buf, cdu = _DualBuffers(arrays), _ffi.ModelDuals()
        buf.fill(cdu)
    if rays:
        ybuf, cry = _RayBuffers(arrays), _ffi.ModelRay()
        ybuf.fill(cry)
        rc = _ffi.lib().dzg_model_solve_rays(C.byref(md), C.byref(opts), C.byref(res),
                                             C.byref(cdu) if duals else None, C.byref(cry))
        _ffi.check(rc, "dzg_model_solve_rays")
    elif want_ranging:
        rbuf, creq, crg = _RangingBuffers(arrays, order, ranging, pivot_tol), _ffi.ModelRangingReq(), _ffi.Ranging()
        rbuf.fill(creq, crg)
        rc = _ffi.lib().dzg_model_solve_ranging(C.byref(md), C.byref(opts), C.byref(creq), C.byref(res),
                                                C.byref(cdu), C.byref(crg))
        _ffi.check_ranging(rc, "dzg_model_solve_ranging")
    elif duals:
        rc = _ffi.lib().dzg_model_solve_duals(C.byref(md), C.byref(opts), C.byref(res), C.byref(cdu))
        _ffi.check(rc, "dzg_model_solve_duals")
    else:
        rc = _ffi.lib().dzg_model_solve(C.byref(md), C.byref(opts), C.byref(res))
        _ffi.check(rc, "dzg_model_solve")
    out = _outcome(res, values, order)
    if isinstance(out, Exception):
        if rays:
            out.ray = ybuf.pyray(cry, order)
        raise out
    if duals:
        out.duals = buf.pyduals(cdu, order)
    if want_ranging and out.duals is not None:
        out.ranging = rbuf.pyranging(order)
    return out


def _has_integer(objective: PyAffExpr, constraints) -> bool:
    if any(v.is_integer for v in objective.pylinexpr.vars):
        return True
    return any(v.is_integer for ineq in constraints for v in ineq._linexpr.vars)


def _mip_call(arrays: dict, is_integer, node_log: int = 0, **mip_opts):
    """dzg_mip_solve on lowered arrays (is_integer: one flag per variable of the table):
    (result struct, values, log entries)."""
    is_int = np.array(list(is_integer) + [0], dtype=np.int32)
    values = np.zeros(max(arrays["nvars"], 1))
    res = _ffi.MipResult()
    res.values = _ffi.ptr(values)
    log = (_ffi.MipNode * max(int(node_log), 1))()
    if node_log:
        res.log = C.cast(log, C.c_void_p)
        res.log_cap = int(node_log)
    opts = _ffi.default_opts(**_options)
    search, node = _split_mip_options({**_mip_options, **mip_opts})
    mo = _ffi.default_mip_opts(**search)
    no = _node_opts(node)
    md = _c_model(arrays)
    rc = _ffi.lib().dzg_mip_solve_nodes(C.byref(md), _ffi.ptr(is_int), C.byref(opts), C.byref(mo),
                                        C.byref(no) if no is not None else None, C.byref(res))
    _ffi.check(rc, "dzg_mip_solve")
    stats = _ffi.mip_last_warm_stats()
    res.warm_stats = (int(stats.nodes_warm), int(stats.nodes_restarted), int(stats.warm_iterations),
                      int(stats.restart_iterations))
    res.fast_stats = None  # not asked for
    if no is not None:
        fs = _ffi.mip_last_fast_stats()
        res.fast_stats = (int(fs.nodes_fast) - int(fs.nodes_rejected), int(fs.nodes_rejected))
    entries = [(e.id, e.parent, e.branch_var, e.direction, e.bound, e.status, e.iterations,
                e.objective) for e in log[:res.log_count]]
    return res, values, entries


def _mip_outcome(res, values, order, entries, where: str = "", stacklevel: int = 4):
    """The PySolution of one dzg_mip_result, or the exception solve_mip() raises for it."""
    rc = int(res.status)
    gap = abs(res.best_bound - res.objective) if res.has_incumbent else float("inf")
    info = MipInfo(status=_ffi.status_str(rc), nodes=int(res.nodes_solved), rounds=int(res.rounds),
                   lp_iterations=int(res.lp_iterations), best_bound=float(res.best_bound), gap=gap,
                   objective=float(res.objective) if res.has_incumbent else None,
                   nodes_batched=int(res.nodes_batched), nodes_sequential=int(res.nodes_sequential),
                   nodes_pruned=int(res.nodes_pruned), nodes_dropped=int(res.nodes_dropped),
                   incumbent_node=int(res.incumbent_node), failed_node=int(res.failed_node),
                   log=entries, nodes_warm=res.warm_stats[0], nodes_restarted=res.warm_stats[1],
                   nodes_fast_accepted=res.fast_stats[0] if res.fast_stats else None,
                   nodes_fast_rejected=res.fast_stats[1] if res.fast_stats else None)
    if rc == _ffi.INFEASIBLE:
        return InfeasibleError("The model is infeasible (no integral point)" + where)
    if rc == _ffi.UNBOUNDED and res.failed_node == 0:
        return UnboundedError("The objective is unbounded (the root relaxation is unbounded)" + where)
    if rc == _ffi.NODE_LIMIT:
        if not res.has_incumbent:
            return RuntimeError(f"branch and bound hit the node limit after {res.nodes_solved} nodes "
                                f"without an integral solution{where}")
        warnings.warn(f"branch and bound hit the node limit after {res.nodes_solved} nodes: the "
                      f"incumbent is returned, best bound {res.best_bound!r}{where}", MipLimitWarning,
                      stacklevel=stacklevel)
    elif rc != _ffi.OPTIMAL:
        return RuntimeError(f"branch and bound stopped: node {res.failed_node} ended with status "
                            f"{_ffi.status_str(rc)!r}{where}")
    # "fast" when at least one node LP was too large for STRICT under AUTO (dzg_model_solve's rule)
    numerics = "fast" if res.nodes_fast > 0 else "strict"
    return PySolution(float(res.objective), {v.id: float(values[i]) for i, v in enumerate(order)},
                      int(res.lp_iterations), numerics, (0, 0), info)


def solve_mip(objective: PyAffExpr, constraints, *, node_log: int = 0, **mip_opts) -> PySolution:
    """Maximise `objective` subject to `constraints` with the variables marked integer=True held
    integral: branch and bound on the GPU (dzg_mip_solve).  Options: set_mip_options(), overridden
    per call by keyword.  The returned PySolution carries .mip (a MipInfo); its .numerics is
    "strict" unless some node LP ran in FAST numerics.  Raises InfeasibleError (no integral
    point), UnboundedError (the root relaxation is unbounded: such a model may in fact be
    infeasible), RuntimeError (a node LP failed, or the node limit was hit with no incumbent); at
    the node limit with an incumbent it warns MipLimitWarning and returns the incumbent."""
    if not isinstance(objective, PyAffExpr):
        raise TypeError("objective must be a PyAffExpr")
    arrays, order = lower(objective, list(constraints))
    _ffi.require_gpu()
    res, values, entries = _mip_call(arrays, [v.is_integer for v in order], node_log, **mip_opts)
    out = _mip_outcome(res, values, order, entries if node_log else None)
    if isinstance(out, Exception):
        raise out
    return out


def solve_many(problems, *, duals: bool = False, ranging=False, pivot_tol: float = 0.0,
               rays: bool = False, return_exceptions: bool = False, fast: bool = False) -> list:
    """solve() for every (objective, constraints) pair of `problems`, in one dzg_model_solve_batch
    call: the models that solve() would run in STRICT numerics on at most 128 rows share one batch
    on the GPU (one workgroup per model), the others are solved one at a time.  Results keep the
    order of `problems` and equal solve()'s one for one.  A model that ends unbounded or infeasible
    raises solve()'s exception, its index in the message, once the whole batch is done; with
    return_exceptions=True the exception instance stands in that model's place instead.  Models with
    an integer variable are solved one by one through solve_mip(), after the batch.  duals=True
    (dzg_model_solve_batch_duals): every solution carries .duals as solve(..., duals=True) gives
    it; a model with an integer variable is then a ValueError.  ranging=True, or one list of row
    groups per problem (dzg_model_solve_batch_ranging): every solution carries .ranging as
    solve(..., ranging=...) gives it; implies duals.  rays=True (dzg_model_solve_batch_rays): every
    UnboundedError / InfeasibleError carries .ray as solve(..., rays=True)'s does.  fast=True
    (dzg_model_solve_batch_fast): the shared batch runs FAST numerics under the AUTO policy -- a model
    whose pivot rule comes within rounding of a tie is re-solved in STRICT inside the same call; not
    yet together with duals, ranging or rays (ValueError)."""
    problems = [(objective, list(constraints)) for objective, constraints in problems]
    want_ranging = _want_ranging(ranging)
    if fast and (duals or want_ranging or rays):
        raise ValueError("fast=True does not combine with duals, ranging or rays yet")
    if rays and want_ranging:
        raise ValueError("rays=True and ranging: the ranging call carries no ray; ask in two calls")
    duals = duals or want_ranging
    for i, (objective, _) in enumerate(problems):
        if not isinstance(objective, PyAffExpr):
            raise TypeError(f"problems[{i}]: objective must be a PyAffExpr")
    mip = [_has_integer(objective, constraints) for objective, constraints in problems]
    if rays and any(mip):
        raise ValueError(f"problems[{mip.index(True)}]: rays=True: rays are not defined for a model "
                         "with integer variables")
    if duals and any(mip):
        raise ValueError(f"problems[{mip.index(True)}]: {'ranging' if want_ranging else 'duals'}=True: "
                         f"{'ranges' if want_ranging else 'dual values'} are not defined for a "
                         "model with integer variables")
    lp_idx = [i for i in range(len(problems)) if not mip[i]]
    out: list = [None] * len(problems)
    lowered = [lower(*problems[i]) for i in lp_idx]
    count = len(lowered)
    keep = [(_c_model(arrays), np.zeros(max(len(order), 1))) for arrays, order in lowered]
    models = (_ffi.Model * max(count, 1))(*[md for md, _ in keep])
    results = (_ffi.ModelResult * max(count, 1))()
    for i, (_, values) in enumerate(keep):
        results[i].values = _ffi.ptr(values)
    opts = _ffi.default_opts(**_options)
    if duals:
        bufs = [_DualBuffers(arrays) for arrays, _ in lowered]
        cdu = (_ffi.ModelDuals * max(count, 1))()
        for k, buf in enumerate(bufs):
            buf.fill(cdu[k])
    if rays:
        ybufs = [_RayBuffers(arrays) for arrays, _ in lowered]
        cry = (_ffi.ModelRay * max(count, 1))()
        for k, ybuf in enumerate(ybufs):
            ybuf.fill(cry[k])
        rc = _ffi.lib().dzg_model_solve_batch_rays(models, C.c_int64(count), C.byref(opts), results,
                                                   cdu if duals else None, cry)
        _ffi.check(rc, "dzg_model_solve_batch_rays")
    elif want_ranging:
        groups = [True] * count if ranging is True else [list(ranging)[i] for i in lp_idx]
        rbufs = [_RangingBuffers(arrays, order, g, pivot_tol) for (arrays, order), g in zip(lowered, groups)]
        creq, crg = (_ffi.ModelRangingReq * max(count, 1))(), (_ffi.Ranging * max(count, 1))()
        for k, rbuf in enumerate(rbufs):
            rbuf.fill(creq[k], crg[k])
        rc = _ffi.lib().dzg_model_solve_batch_ranging(models, C.c_int64(count), C.byref(opts), creq, results,
                                                      cdu, crg)
        _ffi.check_ranging(rc, "dzg_model_solve_batch_ranging")
    elif duals:
        rc = _ffi.lib().dzg_model_solve_batch_duals(models, C.c_int64(count), C.byref(opts), results, cdu)
        _ffi.check(rc, "dzg_model_solve_batch_duals")
    elif fast:
        rc = _ffi.lib().dzg_model_solve_batch_fast(models, C.c_int64(count), C.byref(opts), results)
        _ffi.check(rc, "dzg_model_solve_batch_fast")
    else:
        rc = _ffi.lib().dzg_model_solve_batch(models, C.c_int64(count), C.byref(opts), results)
        _ffi.check(rc, "dzg_model_solve_batch")
    for k, i in enumerate(lp_idx):
        out[i] = _outcome(results[k], keep[k][1], lowered[k][1], f" (model {i})", stacklevel=3)
        if rays and isinstance(out[i], Exception):
            out[i].ray = ybufs[k].pyray(cry[k], lowered[k][1])
        if duals and not isinstance(out[i], Exception):
            out[i].duals = bufs[k].pyduals(cdu[k], lowered[k][1])
            if want_ranging and out[i].duals is not None:
                out[i].ranging = rbufs[k].pyranging(lowered[k][1])
    for i in range(len(problems)):
        if mip[i]:
            arrays, order = lower(*problems[i])
            res, values, _ = _mip_call(arrays, [v.is_integer for v in order])
            out[i] = _mip_outcome(res, values, order, None, f" (model {i})", stacklevel=3)
    if not return_exceptions:
        for o in out:
            if isinstance(o, Exception):
                raise o
    return out
