"""GPU: the three sparse-product kernels of csrc/spmv.hip (spmv_kernel, spmv_items_kernel, spmv_rows_kernel) through their C
entry points, against the integer model (tests/spmv_model.py), by ==.

Every case pre-fills the output and the partial sums with garbage that is no field element (top bits set: above both moduli),
keeps one guard row behind each documented size and downloads the inputs again afterwards.  A row that a call must not touch
has to keep its garbage bit for bit, so "expected" is always a whole array: model values where a row is written, garbage
elsewhere, the guard included."""

import numpy as np
import pytest

import spmv_model as S
from oracle import pyref
from zksnake_amd import _native as N
from zksnake_amd.device import DeviceBuffer
from zksnake_amd.spmv import ITEM, LONG_ROW, DeviceCsr

pytestmark = pytest.mark.gpu

FIELDS = (("BN254", 0), ("BLS12_381", 1))
BY_FIELD = pytest.mark.parametrize("name,cid", FIELDS, ids=[f[0] for f in FIELDS])


def garbage(n, seed):
    """(n, 4) limbs, every row at least 15 * 2^252: no element of either scalar field, so a written row always differs"""
    g = np.random.default_rng(seed).integers(1, 2**64, size=(n, 4), dtype=np.uint64)
    g[:, 3] |= np.uint64(0xF << 60)
    return g


class Stage:
    """one matrix and vector in device memory, an output of n_rows + 1 garbage rows, and the bookkeeping of what must not change"""

    def __init__(self, gpu, cid, row_ptr, cols, vals, w, seed=1):
        self.gpu, self.cid = gpu, cid
        self.n_rows = len(row_ptr) - 1
        self.host = [np.ascontiguousarray(row_ptr, dtype=np.uint32), np.ascontiguousarray(cols, dtype=np.uint32),
                     vals if isinstance(vals, np.ndarray) else S.to_limbs(vals), w if isinstance(w, np.ndarray) else S.to_limbs(w)]
        self.dev = [DeviceBuffer.from_numpy(a) for a in self.host]
        self.garbage = garbage(self.n_rows + 1, seed)
        self.out = DeviceBuffer.from_numpy(self.garbage)

    def lane(self, skip_longer_than):
        rp, cl, vl, w = self.dev
        N.check(self.gpu.zk_spmv_dev(self.cid, self.n_rows, rp.ptr, cl.ptr, vl.ptr, w.ptr, self.out.ptr, skip_longer_than, None))

    def long(self, cutting, seed=2):
        long_rows, item_ptr, items = cutting
        n_items = len(items)
        host = [long_rows, item_ptr, items]
        dev = [DeviceBuffer.from_numpy(a) for a in host]
        stale = garbage(n_items + 1, seed)
        partials = DeviceBuffer.from_numpy(stale)
        rp, cl, vl, w = self.dev
        N.check(self.gpu.zk_spmv_long_dev(self.cid, len(long_rows), dev[0].ptr, dev[1].ptr, n_items, dev[2].ptr, cl.ptr, vl.ptr, w.ptr,
                                          partials.ptr, self.out.ptr, None))
        got = partials.download((n_items + 1, 4))
        assert (got[n_items] == stale[n_items]).all(), "the guard behind the partial sums was written"
        assert not (got[:n_items] == stale[:n_items]).all(axis=1).any(), "an item left no partial sum"
        for d, h in zip(dev, host):
            assert (d.download(h.shape, h.dtype) == h).all(), "an item array was changed"

    def check(self, written, expected):
        """rows `written` hold the model's values, every other row and the guard their garbage; the inputs are as uploaded"""
        want = self.garbage.copy()
        want[list(written)] = S.to_limbs([expected[i] for i in written])
        got = self.out.download((self.n_rows + 1, 4))
        wrong = np.nonzero((got != want).any(axis=1))[0].tolist()
        assert not wrong, f"rows {wrong[:8]} (of {self.n_rows} and a guard) differ"
        for d, h in zip(self.dev, self.host):
            assert (d.download(h.shape, h.dtype) == h).all(), "an input array was changed"


def one_item_each(row_ptr, rows):
    """every row in `rows` listed as a long row with its whole entry range as one work item"""
    items = np.array([(row_ptr[i], row_ptr[i + 1]) for i in rows], dtype=np.uint32).reshape(-1, 2)
    return np.array(rows, dtype=np.uint32), np.arange(len(rows) + 1, dtype=np.uint32), items


# ---- lane kernel: grid and row edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 255, 256, 257, 1000])
@BY_FIELD
def test_lane_kernel_at_grid_and_row_edges(gpu, name, cid, n_rows):
    r = pyref.curve_by_name(name).r
    lengths = [LONG_ROW if i % 97 == 0 else i % 4 for i in range(n_rows)]
    row_ptr, cols, vals, w = S.matrix(lengths, 23, r, n_rows)
    st = Stage(gpu, cid, row_ptr, cols, vals, w, seed=n_rows)
    st.lane(0)
    expected = S.dot_csr(row_ptr, cols, vals, w, r)
    assert all(expected[i] == 0 for i in range(n_rows) if lengths[i] == 0)     # empty rows: four zero limbs
    st.check(range(n_rows), expected)


# ---- skip_longer_than is a parameter ----------------------------------------------------------------------------------------
@BY_FIELD
def test_skip_longer_than_is_a_parameter(gpu, name, cid):
    r = pyref.curve_by_name(name).r
    lengths = [0, 1, 2, 3, LONG_ROW, LONG_ROW + 1, 300]
    row_ptr, cols, vals, w = S.matrix(lengths, 40, r, 6)
    expected = S.dot_csr(row_ptr, cols, vals, w, r)
    every = range(len(lengths))

    st = Stage(gpu, cid, row_ptr, cols, vals, w, seed=10)
    st.lane(0)                                               # 0 = never skip: the 300-entry row on one lane too
    st.check(every, expected)

    st = Stage(gpu, cid, row_ptr, cols, vals, w, seed=11)
    st.lane(2)
    st.check([i for i in every if lengths[i] <= 2], expected)

    st = Stage(gpu, cid, row_ptr, cols, vals, w, seed=12)
    st.lane(LONG_ROW)
    st.check([i for i in every if lengths[i] <= LONG_ROW], expected)
    cutting = S.cut(row_ptr, LONG_ROW, ITEM)
    assert cutting[0].tolist() == [5, 6] and len(cutting[2]) == 2
    st.long(cutting)                                         # writes exactly the two skipped rows
    st.check(every, expected)


# ---- spmv_items_kernel: item lengths around the 256-thread stride -----------------------------------------------------------
ITEM_LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, ITEM - 1, ITEM]


@BY_FIELD
def test_item_lengths_around_the_thread_stride(gpu, name, cid):
    r = pyref.curve_by_name(name).r
    lengths = [1] + ITEM_LENGTHS + [3]                       # a one-entry row first: no item starts on a multiple of 256
    row_ptr, cols, vals, w = S.matrix(lengths, 50, r, 21)
    listed = list(range(1, 1 + len(ITEM_LENGTHS)))
    assert all(int(row_ptr[i]) % S.THREADS for i in listed)
    st = Stage(gpu, cid, row_ptr, cols, vals, w, seed=20)
    st.long(one_item_each(row_ptr, listed))
    st.check(listed, S.dot_csr(row_ptr, cols, vals, w, r))   # the first and the last row are not listed and keep their garbage


# ---- spmv_rows_kernel: item counts around the 256-thread stride -------------------------------------------------------------
@BY_FIELD
def test_item_counts_around_the_partial_stride(gpu, name, cid):
    r = pyref.curve_by_name(name).r
    lengths = [3 * 513, 2, 3 * 256, 3 * 257 - 1, 0, 5]
    row_ptr, cols, vals, w = S.matrix(lengths, 31, r, 31)
    cutting = S.cut(row_ptr, 4, 3)
    assert cutting[0].tolist() == [0, 2, 3, 5] and np.diff(cutting[1].astype(np.int64)).tolist() == [513, 256, 257, 2]
    st = Stage(gpu, cid, row_ptr, cols, vals, w, seed=30)
    st.long(cutting)
    st.check([0, 2, 3, 5], S.dot_csr(row_ptr, cols, vals, w, r))


@BY_FIELD
def test_all_r_minus_1_over_513_items(gpu, name, cid):
    """the most any partial sum and any row sum accumulates: every product is (r - 1)^2 = 1"""
    r = pyref.curve_by_name(name).r
    n = 513 * 3
    row_ptr = S.row_ptr_of([n])
    cols = (np.arange(n) % 7).astype(np.uint32)
    cutting = S.cut(row_ptr, 4, 3)
    assert len(cutting[2]) == 513
    st = Stage(gpu, cid, row_ptr, cols, [r - 1] * n, [r - 1] * 7, seed=40)
    st.long(cutting)
    st.check([0], [n % r])


# ---- the production cut at its first strided size ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_items", [(256 * ITEM, 256), (257 * ITEM + 1, 258)], ids=["2^20", "257_items_and_one_entry"])
def test_production_cut_at_its_first_strided_size(gpu, n, n_items):
    """DeviceCsr on one periodic row: 2^20 entries are 256 items, the shape Groth16.setup reaches for an input wire of a
    2^20-row circuit and the last one whose row sum does not stride; one more item and an entry is the first that does"""
    r = pyref.BN254.r
    row_ptr, cols, vals, w, expected = S.periodic_row(n, r)
    csr = DeviceCsr(0, row_ptr, cols, vals)
    assert (csr.n_rows, csr.n_long, csr.n_items) == (1, 1, n_items)
    stale = garbage(2, 50)
    out, dw = DeviceBuffer.from_numpy(stale), DeviceBuffer.from_numpy(S.to_limbs(w))
    csr.apply(dw.ptr, out.ptr)
    got = out.download((2, 4))
    assert S.from_limbs(got[:1]) == [expected] and (got[1] == stale[1]).all()
    assert (csr.cols.download(cols.shape, np.uint32) == cols).all() and (csr.vals.download(vals.shape) == vals).all()
    assert (dw.download((7, 4)) == S.to_limbs(w)).all() and csr.row_ptr.download((2,), np.uint32).tolist() == [0, n]
    long_rows, item_ptr, items = S.cut(row_ptr)
    assert csr.long_rows.download((1,), np.uint32).tolist() == long_rows.tolist() == [0]
    assert csr.item_ptr.download((2,), np.uint32).tolist() == item_ptr.tolist() == [0, n_items]
    assert (csr.items.download((n_items, 2), np.uint32) == items).all()


# ---- matrix values given as limbs at or above the modulus -------------------------------------------------------------------
@BY_FIELD
def test_limb_values_at_or_above_the_modulus(gpu, name, cid):
    """SparseArray._value_limbs passes a 2-D limb array through unchecked.  The kernels multiply such a value as it is: the
    Montgomery product takes normalised inputs with (a / p)(b / p) <= R / p >= 70, and a value below 2^256 < 5.4 p times a
    canonical w stays far inside, so the product is (v mod r) w R^-1 below 2p like any other"""
    import random
    r = pyref.curve_by_name(name).r
    rnd = random.Random(60)
    raw = [(1 << 256) - 1, r, r + 1, 2 * r, ((1 << 256) // r) * r + 9, (1 << 255) + 12345] + [rnd.randrange(r, 1 << 256) for _ in range(3)]
    assert all(r <= v < 1 << 256 for v in raw) and len(raw) == 9
    row_ptr = S.row_ptr_of([3, 6])
    cols = np.array([0, 4, 4, 1, 2, 3, 4, 0, 2], dtype=np.uint32)
    w = [rnd.randrange(r), r - 1, 1, rnd.randrange(r), rnd.randrange(r)]
    cutting = S.cut(row_ptr, 4, 3)
    assert cutting[0].tolist() == [1] and len(cutting[2]) == 2
    expected = S.dot_csr(row_ptr, cols, [v % r for v in raw], w, r)
    assert expected == S.dot_csr(row_ptr, cols, raw, w, r)
    st = Stage(gpu, cid, row_ptr, cols, raw, w, seed=61)
    st.lane(4)
    st.check([0], expected)
    st.long(cutting)
    st.check([0, 1], expected)
