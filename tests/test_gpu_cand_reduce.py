"""The straight-line argmax reduction of the small-k three-launch iteration (csrc/common.h,
dzg_wave_best2_flat; the four-slot form chain_spec_reduce of k_chain.hip; the two-stage block form),
run on the device through dzg_debug_cand_reduce and checked against a fold of dzg_better2 that is
written HERE, in numpy.  Nothing is compared against the code under test.

r and k are compared by bits; h with ==: the pairwise fold itself leaves the sign of a zero h to the
grouping (`a.h > b.h ? a.h : b.h` on +0.0 / -0.0), which the second test pins down on the CPU: two lane
orders and the butterfly's tree agree in everything but that sign.

Inputs are what the call sites can produce (common.h): the k of valid lanes are pairwise different, a
lane without candidate is (r = +0.0, k = -1), no NaN anywhere; +-inf and +-0.0 are ordinary values."""
import ctypes as C

import numpy as np
import pytest

INF = np.inf
FORMS = {0: 64, 1: 256, 2: 512}  # dzg_debug_cand_reduce: candidates per case
COUNTS = (1, 63, 64, 65, 255, 256)  # of the four-slot form


# ---------------------------------------------------------------------------------------------
# the reference: dzg_better2 and folds of it, over arrays of cases
# ---------------------------------------------------------------------------------------------
def better2(a, b):
    """dzg_better2 (common.h), element-wise: a, b = (r, k, h)"""
    ar, ak, ah = a
    br, bk, bh = b
    b_wins = (ak < 0) | ((bk >= 0) & ((br > ar) | ((br == ar) & (bk < ak))))
    wr, wk = np.where(b_wins, br, ar), np.where(b_wins, bk, ak)
    lr, lk = np.where(b_wins, ar, br), np.where(b_wins, ak, bk)
    h = np.where(ah > bh, ah, bh)
    h = np.where((lk >= 0) & (lr > h), lr, h)
    return wr, wk, h


def none_like(n):
    return np.zeros(n), np.full(n, -1, dtype=np.int32), np.full(n, -INF)


def fold_in_order(r, k, h, order):
    """acc = none; acc = better2(acc, lane) for the lanes in `order`"""
    acc = none_like(r.shape[0])
    for i in order:
        acc = better2(acc, (r[:, i], k[:, i], h[:, i]))
    return acc


def fold_tree(r, k, h):
    """the butterfly's grouping: halves against halves"""
    cur = (r, k, h)
    while cur[0].shape[1] > 1:
        n = cur[0].shape[1] // 2
        cur = better2(tuple(x[:, :n] for x in cur), tuple(x[:, n:] for x in cur))
    return tuple(x[:, 0] for x in cur)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def _empty(n, width):
    return np.zeros((n, width)), np.full((n, width), -1, dtype=np.int32), np.full((n, width), -INF)


def named_cases(width):
    """the cases every form must get right, one per row; (r, k, h, names)"""
    rows = []

    def case(name, lanes):
        """lanes: {lane: (r, k, h)}; every other lane is a none with h = -inf"""
        rows.append((name, lanes))

    last, mid = width - 1, width // 2
    case("all none", {})
    for ln in sorted({0, 31, 32, 63, mid - 1, mid, last}):
        case(f"one valid lane {ln}", {ln: (1.25, 7 + ln, -INF)})
    # equal r, different k: in different rows of 16, in different halves, the low k in the high lane
    for la, lb in ((3, 20), (3, 40), (17, 60), (5, 6), (15, 16), (31, 32), (0, last), (mid - 1, mid)):
        case(f"tie {la}/{lb}, low k first", {la: (2.5, 10, -INF), lb: (2.5, 11, -INF)})
        case(f"tie {la}/{lb}, low k last", {la: (2.5, 11, -INF), lb: (2.5, 10, -INF), 9: (1.0, 99, -INF)})
    case("three-way tie", {2: (4.0, 30, -INF), 18: (4.0, 5, -INF), 50: (4.0, 17, -INF), 33: (3.0, 1, -INF)})
    # +0.0 against -0.0: equal ratios, the lower k wins and keeps its own bits
    case("+0 k low, -0 k high", {4: (0.0, 1, -INF), 37: (-0.0, 2, -INF)})
    case("-0 k low, +0 k high", {4: (0.0, 2, -INF), 37: (-0.0, 1, -INF)})
    case("-0 alone", {21: (-0.0, 3, -INF)})
    case("-0 wins over negatives", {21: (-0.0, 3, -INF), 22: (-1.0, 2, -INF), 61: (-5.0, 0, -INF)})
    case("zeros in h only", {1: (-2.0, 3, 0.0), 34: (-3.0, 4, -0.0)})
    # the pseudo-candidates of dzg_first_pivot_entry: valid, r = -inf
    case("-inf alone", {40: (-INF, 12, -INF)})
    case("two -inf", {40: (-INF, 12, -INF), 8: (-INF, 13, -INF)})
    case("-inf beside finite", {40: (-INF, 2, -INF), 41: (-7.0, 9, -INF), 3: (-9.0, 1, -INF)})
    case("-inf beside a none with h=+inf", {40: (-INF, 2, -INF), 12: (0.0, -1, INF)})
    case("+inf wins", {10: (INF, 5, -INF), 11: (1e300, 4, -INF)})
    case("two +inf", {10: (INF, 5, -INF), 55: (INF, 4, -INF)})
    case("h=+inf on a none lane", {0: (1.0, 1, -INF), 63: (0.0, -1, INF)})
    case("h=+inf on a none lane, nobody valid", {47: (0.0, -1, INF)})
    case("h=+inf on a valid lane", {0: (1.0, 1, -INF), 62: (0.5, 2, INF)})
    case("h=+inf on the winner", {0: (1.0, 1, INF), 62: (0.5, 2, -INF)})
    case("finite h above every r", {6: (1.0, 1, -INF), 23: (0.5, 2, 8.0), 44: (0.75, 3, 2.0)})
    case("finite h on a none above every r", {6: (1.0, 1, -INF), 23: (0.0, -1, 8.0)})
    case("every lane valid, descending", {i: (float(width - i), i, -INF) for i in range(width)})
    case("every lane valid, all equal", {i: (1.0, width - 1 - i, -INF) for i in range(width)})
    r, k, h = _empty(len(rows), width)
    for c, (_, lanes) in enumerate(rows):
        for ln, (rv, kv, hv) in lanes.items():
            r[c, ln], k[c, ln], h[c, ln] = rv, kv, hv
    return r, k, h, [n for n, _ in rows]


def random_cases(rng, n, width):
    """ratios from a small pool (ties, zeros of both signs, +-inf) and from a normal; distinct k"""
    pool = np.array([-INF, -1.5, -0.0, 0.0, 0.5, 1.0, 1.0, 2.0, 2.0, INF])
    hpool = np.array([-INF, -INF, -INF, INF, -0.0, 0.0, 0.75, 1.5, 3.0, 1e9])
    r = np.where(rng.random((n, width)) < 0.5, rng.choice(pool, size=(n, width)), rng.normal(size=(n, width)))
    k = np.argsort(rng.random((n, width)), axis=1).astype(np.int32) * 3  # a permutation per case
    h = rng.choice(hpool, size=(n, width))
    h = np.where(rng.random((n, width)) < 0.7, -INF, h)
    density = rng.choice([0.0, 0.02, 0.1, 0.5, 1.0], size=(n, 1))
    none = rng.random((n, width)) >= density
    r[none], k[none] = 0.0, -1
    return r, k, h


def all_cases(form, seed):
    width = FORMS[form]
    rng = np.random.default_rng(seed)
    nr, nk, nh, names = named_cases(width)
    rr, rk, rh = random_cases(rng, 2000, width)
    r, k, h = np.vstack([nr, rr]), np.vstack([nk, rk]), np.vstack([nh, rh])
    names = names + [f"random {i}" for i in range(rr.shape[0])]
    count = np.full(r.shape[0], width, dtype=np.int32)
    if form == 1:  # every case at every count of the list, then random counts
        reps = [(r, k, h, names, np.full(r.shape[0], c, dtype=np.int32)) for c in COUNTS]
        extra = rng.integers(1, width + 1, size=rr.shape[0]).astype(np.int32)
        reps.append((rr, rk, rh, [f"random count {i}" for i in range(rr.shape[0])], extra))
        r, k, h = (np.vstack([x[j] for x in reps]) for j in range(3))
        names = sum((x[3] for x in reps), [])
        count = np.concatenate([x[4] for x in reps])
    return (np.ascontiguousarray(r), np.ascontiguousarray(k, dtype=np.int32), np.ascontiguousarray(h), count,
            names)


def taking_part(r, k, h, count):
    """the four-slot form: candidates at index >= count do not take part"""
    out = np.arange(r.shape[1])[None, :] >= count[:, None]
    r, k, h = r.copy(), k.copy(), h.copy()
    r[out], k[out], h[out] = 0.0, -1, -INF
    return r, k, h


def _first_bad(ok, names):
    bad = np.flatnonzero(~ok)
    return None if bad.size == 0 else (int(bad[0]), names[int(bad[0])], int(bad.size))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1, 2])
def test_fold_does_not_depend_on_the_order_but_for_a_zero_h(form):
    """What the device code relies on, on the CPU alone: lanes ascending, lanes descending, a seeded
    shuffle and the butterfly's tree give the same r and k bit for bit and the same h up to the sign of
    a zero -- and that sign does differ somewhere, which is why h is compared with ==."""
    r, k, h, count, names = all_cases(form, 20260 + form)
    r, k, h = taking_part(r, k, h, count)
    width = r.shape[1]
    up = fold_in_order(r, k, h, range(width))
    others = [fold_in_order(r, k, h, range(width - 1, -1, -1)),
              fold_in_order(r, k, h, np.random.default_rng(5).permutation(width)),
              fold_tree(r, k, h)]
    sign_differs = 0
    for o in others:
        assert _first_bad(bits(o[0]) == bits(up[0]), names) is None
        assert _first_bad(o[1] == up[1], names) is None
        assert _first_bad(o[2] == up[2], names) is None
        diff = bits(o[2]) != bits(up[2])
        assert np.all((o[2][diff] == 0.0) & (up[2][diff] == 0.0))
        sign_differs += int(diff.sum())
    assert sign_differs > 0
    # the closed form itself, spelled out: max r of the valid lanes, lowest k among them, and h the
    # largest of every h and every other valid r
    valid = k >= 0
    big = np.where(valid, r, -INF).max(axis=1)
    top = valid & (r == big[:, None])
    kk = np.where(top, k, np.iinfo(np.int32).max).min(axis=1)
    win = top & (k == kk[:, None])
    anyv = valid.any(axis=1)
    assert np.array_equal(np.where(anyv, kk, -1), up[1])
    assert np.all(win.sum(axis=1) == anyv)
    own = r[np.arange(r.shape[0]), win.argmax(axis=1)]  # (the winner lane's own bits)
    assert np.array_equal(bits(np.where(anyv, own, 0.0)), bits(up[0]))
    hh = np.maximum(h, np.where(valid & ~win, r, -INF)).max(axis=1)
    assert np.array_equal(hh, up[2])


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 1, 2])
def test_device_reduction_is_the_fold(form):
    from dantzig_amd import _ffi

    r, k, h, count, names = all_cases(form, 20260 + form)
    n = r.shape[0]
    assert n >= 2000 and (form != 1 or set(COUNTS) <= set(count.tolist()))
    out_r, out_k, out_h = np.full(n, np.nan), np.full(n, -7, dtype=np.int32), np.full(n, np.nan)
    rc = _ffi.lib().dzg_debug_cand_reduce(C.c_int32(0), C.c_int32(form), C.c_int64(n), _ffi.ptr(r), _ffi.ptr(k),
                                          _ffi.ptr(h), _ffi.ptr(count), _ffi.ptr(out_r), _ffi.ptr(out_k),
                                          _ffi.ptr(out_h))
    _ffi.check(rc, "dzg_debug_cand_reduce")
    pr, pk, ph = taking_part(r, k, h, count)
    want = fold_in_order(pr, pk, ph, range(pr.shape[1]))
    bad = _first_bad(bits(out_r) == bits(want[0]), names)
    assert bad is None, ("r", bad, out_r[bad[0]], want[0][bad[0]])
    bad = _first_bad(out_k == want[1], names)
    assert bad is None, ("k", bad, out_k[bad[0]], want[1][bad[0]])
    bad = _first_bad(out_h == want[2], names)
    assert bad is None, ("h", bad, out_h[bad[0]], want[2][bad[0]])
