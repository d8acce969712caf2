"""CPU: the integer model of the sparse products (tests/spmv_model.py) against the oracle and the package's host side, and
the fixture conditions that tests/test_gpu_spmv_stages.py and tests/test_gpu_qap_front.py rely on."""

import random

import numpy as np
import pytest

import spmv_model as S
from oracle import pyref
from zksnake_amd import _native as N
from zksnake_amd import spmv
from zksnake_amd.array import SparseArray

FIELDS = ("BN254", "BLS12_381")


@pytest.fixture(scope="module", params=FIELDS)
def skewed(request):
    cv = pyref.curve_by_name(request.param)
    return cv, S.skewed_circuit(cv.r)


def _sparse(trip, n_row, n_col, r):
    return SparseArray.from_triplets(*(list(t) for t in zip(*trip)), n_row, n_col, r)


def test_constants_are_the_packages():
    assert (S.LONG_ROW, S.ITEM) == (spmv.LONG_ROW, spmv.ITEM)
    assert S.THREADS * S.ITEM == 1 << 20
    rnd = random.Random(2)
    vals = [0, 1, (1 << 64) - 1, 1 << 64, (1 << 256) - 1] + [rnd.randrange(1 << 256) for _ in range(20)]
    assert (S.to_limbs(vals) == N.ints_to_limbs(vals, 4)).all() and S.from_limbs(S.to_limbs(vals)) == vals


@pytest.mark.parametrize("name", FIELDS)
def test_dot_csr_equals_the_oracle_and_sparse_array(name):
    r = pyref.curve_by_name(name).r
    lengths = [0, 1, 5, 0, 70, 2, 0]
    n_col = 9
    row_ptr, cols, vals, w = S.matrix(lengths, n_col, r, 4)
    assert np.diff(row_ptr.astype(np.int64)).tolist() == lengths and len(vals) == len(cols) == sum(lengths)
    assert {0, n_col - 1} <= set(cols.tolist()) and {0, 1, r - 1} <= set(w) and {1, r - 1} <= set(vals)
    assert len(set(cols[6:76].tolist())) < 70             # the long row repeats columns
    rows = np.repeat(np.arange(len(lengths)), lengths).tolist()
    trip = list(zip(rows, cols.tolist(), vals))
    got = S.dot_csr(row_ptr, cols, vals, w, r)
    assert got == pyref.sparse_dot(trip, len(lengths), w, r) == _sparse(trip, len(lengths), n_col, r).dot(w)
    assert got[0] == got[3] == got[6] == 0


@pytest.mark.parametrize("long_row,item", [(64, 4096), (4, 3), (1, 1)])
def test_cut_equals_the_packages_cutter(long_row, item):
    lengths = [0, long_row, long_row + 1]
    for k in (1, 256, 257):
        lengths += [k * item - 1, k * item, k * item + 1]
    lengths += [0, 2]
    row_ptr = S.row_ptr_of(lengths)
    rows, ptr, items = S.cut(row_ptr, long_row, item)
    prows, pptr, pitems = spmv.long_row_items(row_ptr, long_row, item)
    assert rows.tolist() == prows.tolist() and ptr.tolist() == pptr.tolist() and items.tolist() == pitems.tolist()
    assert (rows.dtype, ptr.dtype, items.dtype) == (prows.dtype, pptr.dtype, pitems.dtype) and items.shape == pitems.shape
    # the contract itself: exactly the rows above the limit, each tiled without gap or overlap by non-empty items of <= item
    assert rows.tolist() == [i for i, n in enumerate(lengths) if n > long_row]
    for j, i in enumerate(rows.tolist()):
        mine = items[ptr[j]:ptr[j + 1]].astype(np.int64)
        assert mine[0, 0] == row_ptr[i] and mine[-1, 1] == row_ptr[i + 1] and (mine[1:, 0] == mine[:-1, 1]).all()
        assert ((mine[:, 1] - mine[:, 0]) <= item).all() and (mine[:, 1] > mine[:, 0]).all()
        assert len(mine) == -(-lengths[i] // item)
    assert int(ptr[-1]) == len(items)


def test_cut_of_the_partial_stride_case():
    """the row lengths of test_gpu_spmv_stages.py's item-count case"""
    lengths = [3 * 513, 2, 3 * 256, 3 * 257 - 1, 0, 5]
    for cutter in (S.cut, spmv.long_row_items):
        rows, ptr, items = cutter(S.row_ptr_of(lengths), 4, 3)
        assert rows.tolist() == [0, 2, 3, 5] and np.diff(ptr.astype(np.int64)).tolist() == [513, 256, 257, 2] and len(items) == 1028
        assert (items[:, 1] - items[:, 0]).tolist().count(2) == 2          # the last items of rows 3 and 5 are short


def test_csr_and_csc_of_shuffled_duplicate_carrying_matrices(skewed):
    cv, (A, B, C, n_row, n_col, n_pub, w) = skewed
    r = cv.r
    x = [random.Random(8).randrange(r) for _ in range(n_row)]
    x[0], x[1] = 0, r - 1
    in_row_order = sorted(A, key=lambda t: t[0])
    assert in_row_order != A and [t[0] for t in in_row_order] == sorted(t[0] for t in A)
    for trip in (A, B, C, in_row_order):
        m = _sparse(trip, n_row, n_col, r)
        row_ptr, cols, vals = m.to_csr()
        assert row_ptr.dtype == cols.dtype == np.uint32 and vals.dtype == np.uint64 and vals.shape == (len(trip), 4)
        # stable: inside a row the entries keep the order they were given in
        for i in range(n_row):
            mine = [(c, v) for rr, c, v in trip if rr == i]
            k0, k1 = int(row_ptr[i]), int(row_ptr[i + 1])
            assert cols[k0:k1].tolist() == [c for c, _ in mine] and S.from_limbs(vals[k0:k1]) == [v for _, v in mine]
        assert S.dot_csr(row_ptr, cols, S.from_limbs(vals), w, r) == m.dot(w) == pyref.sparse_dot(trip, n_row, w, r)
        col_ptr, rows, tvals = m.to_csc()
        assert col_ptr.shape == (n_col + 1,) and int(col_ptr[-1]) == len(trip)
        assert S.dot_csr(col_ptr, rows, S.from_limbs(tvals), x, r) == S.column_sums(trip, n_col, x, r)


def test_skewed_circuit_is_what_the_gpu_tests_assume(skewed):
    cv, (A, B, C, n_row, n_col, n_pub, w) = skewed
    r = cv.r
    assert (n_row, n_col, n_pub, len(w)) == (11, 311, 3, 311) and S.SKEWED_PADDED == 16
    assert w[0] == 1 and w[S.ZERO_WIRE] == 0 and w[S.MINUS_ONE_WIRE] == r - 1 and all(0 <= v < r for v in w)
    count = lambda trip, key, size: np.bincount([t[key] for t in trip], minlength=size).tolist()  # noqa: E731
    assert count(A, 0, n_row) == [0, 1, 64, 65, 4096, 4097, 8193, 2, 255, 256, 257] == S.SKEWED_LENGTHS
    assert count(B, 0, n_row) == [65, 4096, 4097, 8193, 2, 255, 256, 257, 0, 1, 64]
    assert sorted(C) == [(j, 300 + j, r - 1) for j in range(11)]
    for trip in (A, B):
        assert [t[0] for t in trip] != sorted(t[0] for t in trip)                       # not in row order
        per_wire = count(trip, 1, n_col)
        assert any(0 < n <= S.LONG_ROW for n in per_wire) and any(n > S.LONG_ROW for n in per_wire)   # both kernels of the transpose
        assert len({(t[0], t[1]) for t in trip}) < len(trip) // 2                         # duplicate (row, col) pairs
        assert max(t[1] for t in trip) < S.N_FREE
    assert count(C, 1, n_col)[:300] == [0] * 300                                          # empty transposed rows


def test_skewed_circuit_satisfies_the_oracle_and_every_output_wire_matters(skewed):
    cv, (A, B, C, n_row, n_col, n_pub, w) = skewed
    u, v, _, h = pyref.qap_evaluate_witness(A, B, C, S.SKEWED_PADDED, w, cv)
    assert len(u) == len(v) == 16 and len(h) == 15 and all(h)
    for j in range(n_row):
        bad = list(w)
        bad[S.N_FREE + j] = (bad[S.N_FREE + j] + 1) % cv.r
        with pytest.raises(ValueError, match="did not divided by Z to zero"):
            pyref.qap_evaluate_witness(A, B, C, S.SKEWED_PADDED, bad, cv)


@pytest.mark.parametrize("name", FIELDS)
def test_periodic_row_closed_form(name):
    r = pyref.curve_by_name(name).r
    for n in (1, 34, 35, 36, 1000):
        row_ptr, cols, vals, w, expected = S.periodic_row(n, r)
        assert row_ptr.tolist() == [0, n] and cols.shape == (n,) and vals.shape == (n, 4) and len(w) == 7
        assert cols.tolist() == [k % 7 for k in range(n)]
        ints = S.from_limbs(vals)
        assert all(ints[k] == ints[k % 5] for k in range(n))
        assert S.dot_csr(row_ptr, cols, ints, w, r) == [expected]
