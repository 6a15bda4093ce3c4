"""The batched STRICT solver on the GPU (dzg_batch_solve, core.solve_batch, solve_many): every LP
of a batch follows the CPU oracle bit for bit, and neither the launch slicing nor the company an LP
keeps in a batch changes anything about it."""
import dataclasses
import itertools
import json
import os
import random

import numpy as np
import pytest

import dantzig_amd as dz
from dantzig_amd import core
from oracle import oracle as ora
from tests.lp_families import make_lp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def assert_bit_equal(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    # zeros of either sign compare equal, and so do NaNs of any payload (the sign of a NaN the
    # hardware makes differs from x86's) -- as in tests/test_gpu_parity.py
    same = (_bits(got) == _bits(want)) | ((got == 0.0) & (want == 0.0)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"{what}: {np.count_nonzero(~same)} of {same.size} values differ"


def assert_same_run(got, want, what=""):
    """status, iterations, the whole pivot log (mu bit for bit), basis, nonbasis, x, xbar, z, zbar,
    objective."""
    assert got.status == want.status, what
    assert got.iterations == want.iterations, what
    assert [p[:3] for p in got.pivots] == [tuple(p[:3]) for p in want.pivots], what
    assert_bit_equal([p[3] for p in got.pivots], [p[3] for p in want.pivots], f"{what} mu")
    assert np.asarray(got.basis).tolist() == np.asarray(want.basis).tolist(), what
    assert np.asarray(got.nonbasis).tolist() == np.asarray(want.nonbasis).tolist(), what
    for name in ("x", "xbar", "z", "zbar"):
        assert_bit_equal(getattr(got, name), getattr(want, name), f"{what} {name}")
    assert_bit_equal([got.objective], [want.objective], f"{what} objective")


def _family(seed, kind, m, ns):
    """make_lp's data at a chosen shape."""
    rng = np.random.default_rng(seed)
    if kind == 0:
        a, b, c = core.gen_dense_lp(seed=seed, m=m, n_struct=ns)
        return np.array(a), b, c
    if kind == 1:
        return (rng.integers(-3, 4, (m, ns)).astype(np.float64),
                rng.integers(-2, 9, m).astype(np.float64), rng.integers(-4, 5, ns).astype(np.float64))
    return ((rng.uniform(size=(m, ns)) < 0.3).astype(np.float64),
            rng.integers(0, 4, m).astype(np.float64), rng.integers(-1, 6, ns).astype(np.float64))


def _parity_set():
    out = []
    for i in range(280):
        kind = i % 3
        a, b, c = make_lp(9100 + i, kind, 1, 129)
        out.append((a, b, c))
    out += [_family(1, 0, 1, 3), _family(2, 1, 1, 1), _family(3, 0, 128, 200),
            _family(4, 2, 128, 256), _family(5, 0, 60, 20), _family(6, 1, 90, 40),
            _family(7, 0, 128, 1024), _family(8, 2, 3, 1)]
    # an unbounded LP (a column with no positive entry and a positive cost) and an infeasible one
    out.append((np.array([[1.0, -1.0], [1.0, 0.0]]), np.array([1.0, 2.0]), np.array([0.0, 1.0])))
    out.append((np.array([[1.0, 1.0], [-1.0, -1.0]]), np.array([1.0, -2.0]), np.array([1.0, 1.0])))
    return out


def test_oracle_parity_in_one_batch():
    data = _parity_set()
    lps = [core.CoreLP.from_inequality_form(a, b, c) for a, b, c in data]
    got = core.solve_batch(lps, log_cap=1 << 14)
    statuses = set()
    for i, ((a, b, c), g) in enumerate(zip(data, got)):
        want = ora.simplex_solve(ora.stdform_from_dense(a, b, c))
        assert_same_run(g, want, f"LP {i} ({a.shape[0]} x {a.shape[1]})")
        statuses.add(want.status)
    assert {"optimal", "unbounded", "infeasible"} <= statuses, statuses
    ms = [a.shape[0] for a, _, _ in data]
    assert min(ms) == 1 and max(ms) == 128


def test_launch_slicing_is_invisible():
    data = [make_lp(9500 + i, i % 3, 4, 100) for i in range(24)] + [_family(9, 0, 128, 256)]
    lps = [core.CoreLP.from_inequality_form(a, b, c) for a, b, c in data]
    base = core.solve_batch(lps)
    for ppl in (1, 7):
        for i, (g, w) in enumerate(zip(core.solve_batch(lps, pivots_per_launch=ppl), base)):
            assert_same_run(g, w, f"ppl {ppl} LP {i}")
    # a max_iter cut, resumed once by the batch and once by the single STRICT Solver
    long = [i for i, r in enumerate(base) if r.iterations >= 6]
    assert long
    cut = core.solve_batch(lps, max_iter=5)
    for i in long:
        assert cut[i].status == "iter_limit" and cut[i].iterations == 5
        assert cut[i].pivots == base[i].pivots[:5]
    resumed = [core.resumed_from(lps[i], cut[i]) for i in long]
    again = core.solve_batch(resumed)
    for i, r in zip(long, again):
        w = base[i]
        assert r.status == w.status and r.iterations == w.iterations - 5
        assert r.pivots == w.pivots[5:]
        for name in ("basis", "nonbasis", "x", "xbar", "z", "zbar"):
            assert_bit_equal(getattr(r, name), getattr(w, name), f"batch resume {i} {name}")
    for i in long[:3]:
        s = core.solve(core.resumed_from(lps[i], cut[i]), numerics=core.STRICT)
        w = base[i]
        assert s.status == w.status and s.pivots == w.pivots[5:]
        for name in ("basis", "nonbasis", "x", "xbar", "z", "zbar"):
            assert_bit_equal(getattr(s, name), getattr(w, name), f"Solver resume {i} {name}")


def test_batch_composition_is_invisible():
    small = core.CoreLP.from_inequality_form(*_family(11, 1, 3, 5))
    big = core.CoreLP.from_inequality_form(*_family(12, 0, 128, 200))
    others = [core.CoreLP.from_inequality_form(*make_lp(9700 + i, i % 3, 1, 129)) for i in range(20)]
    one_small, one_big = core.solve_batch([small])[0], core.solve_batch([big])[0]
    mixed = others + [small, big]
    order = list(range(len(mixed)))
    random.Random(5).shuffle(order)
    shuffled = core.solve_batch([mixed[i] for i in order])
    got = {order[k]: r for k, r in enumerate(shuffled)}
    assert_same_run(got[len(others)], one_small, "m = 3 in a mixed batch")
    assert_same_run(got[len(others) + 1], one_big, "m = 128 in a mixed batch")
    alone = core.solve(small, numerics=core.STRICT)
    assert_same_run(one_small, alone, "batch of one vs the single solver")
    # edge shapes: no rows, no nonbasic columns
    edges = [core.CoreLP.from_inequality_form(np.zeros((0, 3)), np.zeros(0), np.array([1.0, -1.0, 0.0])),
             core.CoreLP.from_inequality_form(np.zeros((0, 2)), np.zeros(0), np.array([-1.0, -2.0])),
             core.CoreLP(a=np.zeros((2, 0)), c=np.zeros(2), basis=np.array([0, 1]),
                         nonbasis=np.zeros(0, np.int64), x=np.array([1.0, -1.0]), z=np.zeros(0)),
             core.CoreLP(a=np.zeros((2, 0)), c=np.zeros(2), basis=np.array([0, 1]),
                         nonbasis=np.zeros(0, np.int64), x=np.array([1.0, 2.0]), z=np.zeros(0))]
    for i, (g, lp) in enumerate(zip(core.solve_batch(edges), edges)):
        w = core.solve(lp, numerics=core.STRICT)
        assert g.status == w.status and g.iterations == w.iterations, (i, g.status, w.status)
        for name in ("basis", "nonbasis", "x", "xbar", "z", "zbar"):
            assert_bit_equal(getattr(g, name), getattr(w, name), f"edge {i} {name}")


def _kat_problems():
    with open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")) as f:
        kats = json.load(f)
    return kats


def test_model_level_kats_in_one_call():
    from tests.test_surface import build_problem

    kats = _kat_problems()
    probs, expect = [], []
    for k in kats["python"]:
        ns, p = build_problem(k)
        probs.append(p)
        expect.append((ns, k["expect"]))
    got = dz.solve_many(probs, return_exceptions=True)
    for (ns, exp), g in zip(expect, got):
        if "error" in exp:
            assert type(g) is getattr(dz.exceptions, exp["error"]), g
            continue
        assert not isinstance(g, Exception), g
        if "objective" in exp:
            assert g.objective_value == exp["objective"]
        for name, v in exp["values"].items():
            assert g[ns[name]] == v
    # the solver KATs through the model batch entry point (dzg_model_solve_batch)
    from dantzig_amd import rust as rs

    pairs, table, want = [], [], []
    for k in kats["solver"]:
        md = k["model"]
        vs = [rs.Variable(lb=v["lb"], ub=v["ub"]) for v in md["vars"]]
        obj = rs.PyAffExpr(linexpr=rs.PyLinExpr([t[1] for t in md["objective"]["terms"]],
                                                [vs[t[0]] for t in md["objective"]["terms"]]),
                           constant=md["objective"]["constant"])
        cons = [rs.PyInequality(linexpr=rs.PyLinExpr([t[1] for t in c["terms"]],
                                                     [vs[t[0]] for t in c["terms"]]), b=c["b"])
                for c in md["constraints"]]
        pairs.append((obj, cons))
        table.append(vs)
        want.append(k["expect"])
    got = rs.solve_many(pairs, return_exceptions=True)
    for vs, exp, g, pair in zip(table, want, got, pairs):
        try:
            single = rs.solve(*pair)
        except Exception as e:  # noqa: BLE001
            single = e
        assert type(g) is type(single)
        if exp["status"] == "unbounded":
            assert isinstance(g, dz.exceptions.UnboundedError)
        elif exp["status"] == "infeasible":
            assert isinstance(g, dz.exceptions.InfeasibleError)
        else:
            assert abs(g.objective_value - exp["objective"]) <= 1e-12
            assert g.objective_value == single.objective_value
            assert [g[v] for v in vs] == [single[v] for v in vs]


def _random_problem(rng, rows):
    nv = int(rng.integers(1, 8))
    kinds = rng.integers(0, 4, nv)
    vs = []
    for k in kinds:
        if k == 0:
            vs.append(dz.Variable.nonneg())
        elif k == 1:
            vs.append(dz.Variable.free())
        elif k == 2:
            vs.append(dz.Variable(lb=float(rng.integers(-3, 1)), ub=float(rng.integers(1, 5))))
        else:
            vs.append(dz.Variable(lb=None, ub=float(rng.integers(0, 4))))
    obj = sum(float(rng.integers(-3, 4)) * v for v in vs) + float(rng.integers(-2, 3))
    cons = []
    for _ in range(rows):
        idx = rng.choice(nv, size=int(rng.integers(1, nv + 1)), replace=False)
        lhs = sum(float(rng.integers(-3, 4)) * vs[i] for i in idx)
        rhs = float(rng.integers(-2, 8))
        op = int(rng.integers(0, 5))
        cons.append(lhs == rhs if op == 0 else (lhs >= rhs if op == 1 else lhs <= rhs))
    cls = dz.Minimize if rng.integers(0, 2) else dz.Maximize
    return vs, cls(obj).subject_to(cons)


def test_solve_many_equals_one_solve_per_model():
    rng = np.random.default_rng(77)
    items = [_random_problem(rng, int(rng.integers(0, 12))) for _ in range(250)]
    items += [_random_problem(rng, int(rng.integers(130, 150))) for _ in range(4)]  # over 128 rows
    order = list(range(len(items)))
    random.Random(3).shuffle(order)
    items = [items[i] for i in order]
    got = dz.solve_many([p for _, p in items], return_exceptions=True)
    assert len(got) == len(items)
    kinds = set()
    for i, ((vs, p), g) in enumerate(zip(items, got)):
        try:
            w = p.solve()
        except Exception as e:  # noqa: BLE001
            assert type(g) is type(e), (i, g, e)
            assert f"(model {i})" in str(g)
            kinds.add(type(e).__name__)
            continue
        assert not isinstance(g, Exception), (i, g)
        assert_bit_equal([g.objective_value], [w.objective_value], f"model {i}")
        assert_bit_equal([g[v] for v in vs], [w[v] for v in vs], f"model {i} values")
        kinds.add("optimal")
    assert "optimal" in kinds and len(kinds) >= 2, kinds
    with pytest.raises((dz.exceptions.UnboundedError, dz.exceptions.InfeasibleError), match=r"\(model \d+\)"):
        dz.solve_many([p for _, p in items])


def assert_same_extra(got, want, what=""):
    """A CoreDuals, CoreRanging or CoreRay (or None on both sides), every field bit for bit."""
    assert (got is None) == (want is None), what
    if got is None:
        return
    for f in dataclasses.fields(got):
        g, w = getattr(got, f.name), getattr(want, f.name)
        if dataclasses.is_dataclass(g) or g is None or w is None:
            assert_same_extra(g, w, f"{what} {f.name}")
        elif isinstance(g, (float, np.ndarray)) and np.asarray(g).dtype.kind == "f":
            assert_bit_equal(g, w, f"{what} {f.name}")
        else:
            assert np.array_equal(g, w), f"{what} {f.name}"


_FOUR_WAYS = (dict(), dict(duals=True), dict(ranging=True), dict(rays=True, duals=True))


def test_the_passes_disturb_neither_the_solve_nor_each_other():
    rows = (1, 16, 17, 32, 33, 64, 65, 128)  # both sides of every bucket edge
    # seeds at which every bucket holds an LP that ends optimal (m = 1, 17, 64, 65) for the duals and
    # ranging passes, and the first three one that ends unbounded (m = 16, 33) for the rays pass
    data = [_family(46 + k, k % 3, m, 2 * m if m <= 64 else 80) for k, m in enumerate(rows)]
    data += _parity_set()[-2:]  # the unbounded LP and the infeasible one
    data.append((np.zeros((0, 3)), np.zeros(0), np.array([1.0, -1.0, 0.0])))  # no rows
    lps = [core.CoreLP.from_inequality_form(a, b, c) for a, b, c in data]
    full = [core.solve_batch(lps, **kw) for kw in _FOUR_WAYS]
    assert {"optimal", "unbounded", "infeasible"} <= {r.status for r in full[0]}
    assert [full[0][rows.index(m)].status for m in (1, 17, 64, 65)] == ["optimal"] * 4
    assert [full[0][rows.index(m)].status for m in (16, 33)] == ["unbounded"] * 2
    for i in range(len(lps)):
        for (p, a), (q, b) in itertools.combinations(enumerate(full), 2):
            assert_same_run(a[i], b[i], f"LP {i}, calls {p} and {q}")
        assert (full[1][i].duals is not None) == (full[0][i].status == "optimal"), i
        assert (full[2][i].ranging is not None) == (full[0][i].status == "optimal"), i
        assert (full[3][i].ray is not None) == (full[0][i].status in ("unbounded", "infeasible")), i
        assert_same_extra(full[2][i].duals, full[1][i].duals, f"LP {i} duals, ranging call")
        assert_same_extra(full[3][i].duals, full[1][i].duals, f"LP {i} duals, rays call")
    # buckets 1 and 2 empty: every LP is what it was in the full batch
    keep = [i for i, lp in enumerate(lps) if lp.m <= 16 or lp.m > 64]
    assert len(keep) == len(lps) - 4
    for kw, whole in zip(_FOUR_WAYS, full):
        part = core.solve_batch([lps[i] for i in keep], **kw)
        for g, i in zip(part, keep):
            assert_same_run(g, whole[i], f"LP {i} {kw}")
            for name in ("duals", "ranging", "ray"):
                assert_same_extra(getattr(g, name), getattr(whole[i], name), f"LP {i} {kw} {name}")


def test_the_grid_cap_is_invisible_to_the_passes():
    count, m, ns = 257, 65, 8  # the largest bucket's smallest LPs, one more than its 256 workgroups
    data = [_family(9300 + i, 2 * (i % 2), m, ns) for i in range(count)]
    want = [ora.simplex_solve(ora.stdform_from_dense(a, b, c)).status for a, b, c in data]
    ended = [i for i, s in enumerate(want) if s in ("unbounded", "infeasible")]
    # enough OPTIMAL LPs that their 2 directions each need a second launch, LP 256 among them
    assert want[256] == "optimal" and want.count("optimal") > 128 and ended, want
    lps = [core.CoreLP.from_inequality_form(a, b, c) for a, b, c in data]
    reqs = [([{i % (m + ns): 1.0}], [{i % m: 1.0}]) for i in range(count)]
    certified = core.solve_batch(lps, duals=True, rays=True)
    ranged = core.solve_batch(lps, ranging=reqs)
    assert [r.status for r in certified] == want
    for i in (256, ended[-1]):  # and the last LP of the rays pass's list
        one = core.solve_batch([lps[i]], duals=True, rays=True)[0]
        assert_same_run(certified[i], one, f"LP {i}")
        assert_same_extra(certified[i].duals, one.duals, f"LP {i} duals")
        assert_same_extra(certified[i].ray, one.ray, f"LP {i} ray")
        one = core.solve_batch([lps[i]], ranging=[reqs[i]])[0]
        assert_same_run(ranged[i], one, f"LP {i}, ranging call")
        assert_same_extra(ranged[i].ranging, one.ranging, f"LP {i} ranges")
    assert certified[256].duals is not None and ranged[256].ranging is not None
    assert certified[ended[-1]].ray is not None
