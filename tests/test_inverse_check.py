"""The reference check of the basis inverse (tests/inverse_check.py) on synthetic inverses built
with numpy: it accepts B^-1 in explicit and in product form (Binv0 - U W^T), for dense and CSC
matrices, and rejects each of the ways an inverse goes subtly wrong."""
import numpy as np
import pytest

from tests import inverse_check as ic

M, NS, K = 90, 180, 45


def _lp(seed=1):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (M, NS)) * (rng.uniform(size=(M, NS)) < 0.3)
    a[rng.integers(0, M, NS), np.arange(NS)] = 1.0        # no empty column
    cols = rng.choice(NS, K, replace=False)
    pos = rng.choice(M, K, replace=False)
    basis = np.empty(M, dtype=np.int64)
    basis[pos] = cols
    basis[np.setdiff1d(np.arange(M), pos)] = NS + rng.choice(M, M - K, replace=False)
    return a, basis


def _pivots(a, basis, count, seed=2):
    """`count` structural pivots in product form: Binv0 = B0^-1, u_t = (dx - e_p) / dx_p,
    w_t = row p of the current inverse; returns Binv0, U, W, the bases and the explicit inverses."""
    rng = np.random.default_rng(seed)
    basis = basis.copy()
    b0 = ic.basis_matrix(a, basis, NS)
    binv0 = np.linalg.inv(b0)
    cur = binv0.copy()
    us, ws, bases, invs = [], [], [basis.copy()], [binv0]
    for _ in range(count):
        q = int(rng.choice(np.setdiff1d(np.arange(NS), basis)))
        dx = cur @ a[:, q]
        p = int(np.argmax(np.abs(dx)))
        u = dx.copy()
        u[p] -= 1.0
        u /= dx[p]
        w = cur[p].copy()
        cur = cur - np.outer(u, w)
        basis[p] = q
        us.append(u)
        ws.append(w)
        bases.append(basis.copy())
        invs.append(np.linalg.inv(ic.basis_matrix(a, basis, NS)))
    return binv0, np.array(us), np.array(ws), bases, invs


def _worst(binv, a, basis, rows=None):
    rows = np.arange(M) if rows is None else np.asarray(rows)
    return float(ic.residual(binv[rows], rows, a, basis, NS).max())


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).nmant >= 63


def test_accepts_the_inverse_dense_and_csc():
    a, basis = _lp()
    binv = np.linalg.inv(ic.basis_matrix(a, basis, NS))
    assert _worst(binv, a, basis) <= ic.C_MAX
    csc_ptr = np.concatenate([[0], np.cumsum((a != 0).sum(axis=0))])
    rows = np.concatenate([np.flatnonzero(a[:, j]) for j in range(NS)])
    vals = np.concatenate([a[np.flatnonzero(a[:, j]), j] for j in range(NS)])
    csc = ic.Csc(M, csc_ptr, rows, vals)
    assert np.array_equal(ic.basis_matrix(csc, basis, NS), ic.basis_matrix(a, basis, NS))
    assert _worst(binv, csc, basis) == _worst(binv, a, basis)


def test_accepts_the_product_form():
    a, basis = _lp()
    binv0, u, w, bases, _ = _pivots(a, basis, 12)
    assert _worst(binv0 - u.T @ w, a, bases[-1]) <= ic.C_MAX


def test_rejects_two_rows_swapped():
    a, basis = _lp()
    binv = np.linalg.inv(ic.basis_matrix(a, basis, NS))
    i, j = int(np.flatnonzero(basis < NS)[0]), int(np.flatnonzero(basis >= NS)[0])
    bad = binv.copy()
    bad[[i, j]] = bad[[j, i]]
    assert _worst(bad, a, basis) > ic.C_MAX
    assert _worst(bad, a, basis, rows=[i]) > ic.C_MAX


@pytest.mark.parametrize("row", [0, 17, M - 1])
def test_rejects_one_entry_off_by_1e_9(row):
    a, basis = _lp()
    binv0, u, w, bases, _ = _pivots(a, basis, 5)
    binv = binv0 - u.T @ w
    bad = binv.copy()
    r = int(np.argmax(np.abs(bad[row])))
    bad[row, r] *= 1.0 + 1e-9
    assert _worst(binv, a, bases[-1], rows=[row]) <= ic.C_MAX
    assert _worst(bad, a, bases[-1], rows=[row]) > ic.C_MAX


def test_rejects_binv0_without_its_etas():
    a, basis = _lp()
    binv0, u, w, bases, _ = _pivots(a, basis, 3)
    assert _worst(binv0, a, bases[-1]) > ic.C_MAX
    # ... also on the rows a sample takes: the positions of the last pivots
    recent = [int(p) for p in np.flatnonzero(bases[-1] != bases[0])]
    assert _worst(binv0, a, bases[-1], rows=recent) > ic.C_MAX


def test_rejects_the_inverse_of_the_basis_one_pivot_earlier():
    a, basis = _lp()
    _, _, _, bases, invs = _pivots(a, basis, 4)
    assert _worst(invs[-1], a, bases[-1]) <= ic.C_MAX
    assert _worst(invs[-2], a, bases[-1]) > ic.C_MAX


def test_row_sample_takes_the_rows_that_matter():
    a, basis = _lp()
    rows = ic.sample_rows(M, basis, NS, recent=[5, 77], n=8, seed=3)
    assert {5, 77, 0, M - 1} <= set(rows.tolist())
    assert (basis[rows] < NS).any() and (basis[rows] >= NS).any()
    assert np.array_equal(rows, np.unique(rows))
    assert np.array_equal(ic.sample_rows(M, basis, NS, every_below=M + 1), np.arange(M))
    pivots = [(0, int(basis[3]), -1, 0.0), (0, int(basis[40]), -1, 0.0)]
    assert ic.last_pivot_positions(basis, pivots) == [3, 40]
