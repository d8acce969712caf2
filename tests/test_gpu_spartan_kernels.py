"""GPU: zk_r1cs_products_dev and zk_r1cs_bind_dev (csrc/spartan.hip) against the integer model (tests/spartan_model.py), on both
curves, at the shapes where the code takes another path: the smallest tables, empty sub-segments, repeats, the ends of the field,
the LONG_ROW and ITEM boundaries, long and short sub-segments in one segment, more long segments than the capped grid has
workgroups, more segments than it has threads, and a busy stream.  Outputs start poisoned: every element must be written.
Every comparison is == on integers."""

import ctypes
import random

import numpy as np
import pytest

import spartan_model as S
from zksnake_amd import _native as N
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from zksnake_amd.frvec import DevVec, FrOps
from zksnake_amd.spartan import protocol as SP
from zksnake_amd.spmv import ITEM, LONG_ROW

pytestmark = pytest.mark.gpu

FIELDS = (("BN254", BN254_SCALAR_FIELD), ("BLS12_381", BLS12_381_SCALAR_FIELD))
IDS = [f[0] for f in FIELDS]
GRID = 1 << 18          # FR_MAX_BLOCKS workgroups of 256 threads (csrc/fr_sum.hip.h): segment 2^18 is a thread's second one
MAX_BLOCKS = 1024


def raw(vals):
    return np.ascontiguousarray(N.ints_to_limbs(list(vals), 4))


def poisoned(gpu, n):
    vec = DevVec(n, zero=False)
    N.check(gpu.zk_dev_memset(vec.ptr(), 0xA5, 32 * n))
    return vec


def ints(vec):
    return N.limbs_to_ints(vec.download())


def device_csr(ops, log_seg, ptr, idx, val):
    return SP.DeviceR1csCsr(ops.cid, log_seg, np.array(ptr, dtype=np.uint32), np.array(idx, dtype=np.uint32),
                            raw(val) if val else np.zeros((0, 4), dtype=np.uint64))


def run_both(gpu, ops, csr, log_x, d_x, coeff, stream=None):
    """both entry points on poisoned outputs: (az, bz, cz, out) as device vectors"""
    n_seg = 1 << csr.log_seg
    outs = [poisoned(gpu, n_seg) for _ in range(4)]
    if stream is not None:
        N.check(gpu.zk_dev_synchronize())                # the stream does not wait for the default stream's fills
        N.check(gpu.zk_debug_spin_dev(stream, 2000))     # the calls queue up behind work already on their stream
    csr.products(log_x, d_x.ptr(), outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), stream)
    csr.bind(log_x, d_x.ptr(), raw(coeff), outs[3].ptr(), stream)
    if stream is not None:
        N.check(gpu.zk_stream_synchronize(stream))
    return outs


def check(gpu, p, log_seg, mats, x, coeff, stream=None, n_long=None, n_items=None):
    ops = FrOps(p)
    ptr, idx, val = S.merged_csr(1 << log_seg, mats)
    csr = device_csr(ops, log_seg, ptr, idx, val)
    try:
        if n_long is not None:
            assert (csr.n_long, csr.n_items) == (n_long, n_items)
        d_x = ops.d_from(raw(x))
        az, bz, cz, out = run_both(gpu, ops, csr, len(x).bit_length() - 1, d_x, coeff, stream)
        assert (ints(az), ints(bz), ints(cz)) == S.products(ptr, idx, val, x, p)
        assert ints(out) == S.bind(ptr, idx, val, x, coeff, p)
    finally:
        csr.free()


def rand_mats(rnd, p, n_seg, n_x, lengths):
    """lengths: {(segment, matrix): entries}; random idx and full-width values"""
    mats = [[], [], []]
    for (seg, m), count in lengths.items():
        mats[m] += [(seg, rnd.randrange(n_x), rnd.randrange(p)) for _ in range(count)]
    return mats


def rand_x(rnd, p, n):
    return [rnd.randrange(p) for _ in range(n)]


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_smallest_tables(gpu, name, p):
    rnd = random.Random(1)
    coeff = rand_x(rnd, p, 3)
    # log_seg = 0: one segment; log_x = 0: one element of x
    check(gpu, p, 0, [[(0, 0, 5)], [(0, 0, p - 2)], [(0, 0, 7), (0, 0, 1)]], [rnd.randrange(p)], coeff, n_long=0, n_items=0)
    check(gpu, p, 0, rand_mats(rnd, p, 1, 4, {(0, 0): 3, (0, 2): 2}), rand_x(rnd, p, 4), coeff)
    check(gpu, p, 1, rand_mats(rnd, p, 2, 2, {(0, 0): 1, (1, 1): 2, (1, 2): 1, (0, 2): 3}), rand_x(rnd, p, 2), coeff)
    check(gpu, p, 3, rand_mats(rnd, p, 8, 16, {(s, m): rnd.randrange(5) for s in range(7) for m in range(3)}), rand_x(rnd, p, 16), coeff)


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_empty_matrices_and_repeats(gpu, name, p):
    rnd = random.Random(2)
    coeff, x = rand_x(rnd, p, 3), rand_x(rnd, p, 8)
    check(gpu, p, 2, [[], [], []], x, coeff)                                              # all sub-segments empty: zeros
    check(gpu, p, 0, [[], [], []], x[:1], coeff)
    for empty in range(3):
        mats = rand_mats(rnd, p, 4, 8, {(s, m): 1 + rnd.randrange(3) for s in range(4) for m in range(3) if m != empty})
        check(gpu, p, 2, mats, x, coeff)
    # a repeated (segment, idx) adds -- also to zero
    check(gpu, p, 1, [[(1, 3, 5), (1, 3, 6), (1, 3, p - 11)], [(0, 2, 9), (0, 2, 9)], [(1, 0, 1), (1, 1, 1), (1, 0, 1)]], x, coeff)


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_field_edges(gpu, name, p):
    top = p - 1
    mats = [[(s, i, top) for s in range(4) for i in range(3)], [(1, 7, top)], [(s, s, top) for s in range(4)] * 2]
    for coeff in ((0, 0, 0), (top, top, top), (0, top, 1), (top, 0, p), (2 ** 256 - 1, p + 1, 2 * p - 1)):   # reduced on entry
        check(gpu, p, 2, mats, [top] * 8, coeff)
    # a long sub-segment of r - 1 times r - 1: the block sums at the top of the range
    check(gpu, p, 1, [[(0, i % 8, top) for i in range(ITEM + 1)], [], [(1, 0, top)] * (LONG_ROW + 1)], [top] * 8, (top, top, top),
          n_long=2, n_items=3)


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_long_row_boundary_and_work_items(gpu, name, p):
    rnd = random.Random(3)
    coeff, x = rand_x(rnd, p, 3), rand_x(rnd, p, 64)
    check(gpu, p, 2, rand_mats(rnd, p, 4, 64, {(1, 1): LONG_ROW, (2, 0): 3}), x, coeff, n_long=0, n_items=0)       # 64 stays short
    check(gpu, p, 2, rand_mats(rnd, p, 4, 64, {(1, 1): LONG_ROW + 1, (2, 0): 3}), x, coeff, n_long=1, n_items=1)   # 65 goes long
    check(gpu, p, 2, rand_mats(rnd, p, 4, 64, {(3, 2): ITEM, (0, 0): LONG_ROW}), x, coeff, n_long=1, n_items=1)    # 4096: one item
    check(gpu, p, 2, rand_mats(rnd, p, 4, 64, {(3, 2): ITEM + 1, (0, 0): 1}), x, coeff, n_long=1, n_items=2)       # 4097: two
    # two long sub-segments in the SAME segment, for A and C, beside a short B; a neighbour that is long in B only; short ones around
    lengths = {(1, 0): 2 * ITEM + 7, (1, 1): 5, (1, 2): LONG_ROW + 1, (2, 1): 300, (2, 0): LONG_ROW, (0, 0): 2, (3, 2): 1}
    check(gpu, p, 2, rand_mats(rnd, p, 4, 64, lengths), x, coeff, n_long=2, n_items=5)
    # the first and the last segment long, and every sub-segment of one segment long
    lengths = {(0, 0): 70, (7, 2): 70, (4, 0): 100, (4, 1): ITEM + 100, (4, 2): 65, (5, 1): 64}
    check(gpu, p, 3, rand_mats(rnd, p, 8, 64, lengths), x, coeff, n_long=3, n_items=6)


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_more_long_segments_than_workgroups(gpu, name, p):
    """1030 long segments of one item each: the item kernel and the long-segment kernel both stride past their 1024 workgroups"""
    rnd = random.Random(4)
    n_long = MAX_BLOCKS + 6
    lengths = {(s, s % 3): LONG_ROW + 1 + (s % 2) for s in range(n_long)}
    lengths.update({(s, (s + 1) % 3): 2 for s in range(0, n_long, 7)})
    check(gpu, p, 11, rand_mats(rnd, p, 2048, 32, lengths), rand_x(rnd, p, 32), rand_x(rnd, p, 3), n_long=n_long, n_items=n_long)


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_past_the_grid(gpu, name, p):
    """2^18 + 257 segments with one entry each in 2^19: the threads of the first workgroup and one more take a second segment, the
    padding segments are written as zero.  With one entry per segment the model's sums are single products."""
    rnd = random.Random(5)
    ops = FrOps(p)
    n, log_seg, log_x = GRID + 257, 19, 10
    x, coeff = rand_x(rnd, p, 1 << log_x), rand_x(rnd, p, 3)
    idx = [rnd.randrange(1 << log_x) for _ in range(n)]
    val = [rnd.randrange(p) for _ in range(n)]
    mat = [i % 3 if i < GRID else (i + 1) % 3 for i in range(n)]
    ptr = np.zeros(3 * (1 << log_seg) + 1, dtype=np.uint32)
    filled = np.zeros(3 * (1 << log_seg), dtype=np.int64)
    filled[3 * np.arange(n) + np.array(mat)] = 1
    np.cumsum(filled, out=ptr[1:])
    csr = device_csr(ops, log_seg, ptr, idx, val)
    try:
        assert csr.n_long == 0
        outs = run_both(gpu, ops, csr, log_x, ops.d_from(raw(x)), coeff)
        got = [ints(v) for v in outs]
        pad = [0] * ((1 << log_seg) - n)
        for m in range(3):
            assert got[m] == [v * x[i] % p if k == m else 0 for v, i, k in zip(val, idx, mat)] + pad, "ABC"[m]
        assert got[3] == [coeff[k] * v * x[i] % p for v, i, k in zip(val, idx, mat)] + pad
    finally:
        csr.free()


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_past_the_grid_geometric(gpu, name, p):
    """x[j] = c g^j and val[k] = d u^k built on the device, segment i < 2^18 + 257 holds entry i in matrix i mod 3 with idx = i: the
    outputs are the closed forms c d (g u)^i, pinned at the edges of the grid and summed as geometric series"""
    rnd = random.Random(6)
    ops = FrOps(p)
    n, log_seg = GRID + 257, 19
    c, g, d, u = (rnd.randrange(1 << 250, p) for _ in range(4))
    coeff = rand_x(rnd, p, 3)

    def geo(first, ratio, count):
        vec = ops.d_powers(ratio, count)
        N.check(gpu.zk_vec_axpby_dev(ops.cid, count, N.u64p(raw([first])), vec.ptr(), None, None, None, vec.ptr(), None))
        return vec

    d_x, d_val = geo(c, g, 1 << log_seg), geo(d, u, n)
    filled = np.zeros(3 * (1 << log_seg), dtype=np.int64)
    filled[3 * np.arange(n) + np.arange(n) % 3] = 1   # sub-segment 3 i + i mod 3
    ptr = np.zeros(3 * (1 << log_seg) + 1, dtype=np.uint32)
    np.cumsum(filled, out=ptr[1:])
    idx = np.arange(n, dtype=np.uint32)
    csr = SP.DeviceR1csCsr(ops.cid, log_seg, ptr, idx, d_val.download())
    try:
        assert csr.n_long == 0 and int(ptr[-1]) == n and [int(ptr[3 * 5 + k]) for k in range(4)] == [5, 5, 5, 6]
        outs = run_both(gpu, ops, csr, log_seg, d_x, coeff)
        q = g * u % p
        pins = sorted({0, 1, 2, 3, 255, 256, 257, GRID - 1, GRID, GRID + 1, GRID + 255, GRID + 256, n - 1, n, n + 1, (1 << log_seg) - 1}
                      | {rnd.randrange(n) for _ in range(48)})
        for i in pins:
            want = [0, 0, 0]
            if i < n:
                want[i % 3] = c * d * pow(q, i, p) % p
            for m in range(3):
                assert ops.int_at(outs[m].download(1, i), 0) == want[m], f"{'ABC'[m]}[{i}]"
            assert ops.int_at(outs[3].download(1, i), 0) == sum(coeff[m] * want[m] for m in range(3)) % p, f"out[{i}]"
        # the sums: matrix m holds c d q^i over the i < n with i = m mod 3
        q3 = pow(q, 3, p)
        total = []
        for m in range(3):
            count = (n - m + 2) // 3
            series = c * d * pow(q, m, p) * (pow(q3, count, p) - 1) * pow(q3 - 1, -1, p) % p
            total.append(series)
            out = np.zeros(4, dtype=np.uint64)
            N.check(gpu.zk_mle_sum_dev(ops.cid, 1 << log_seg, outs[m].ptr(), N.u64p(out), None))
            assert int.from_bytes(out.tobytes(), "little") == series, "ABC"[m]
        out = np.zeros(4, dtype=np.uint64)
        N.check(gpu.zk_mle_sum_dev(ops.cid, 1 << log_seg, outs[3].ptr(), N.u64p(out), None))
        assert int.from_bytes(out.tobytes(), "little") == sum(k * t for k, t in zip(coeff, total)) % p
    finally:
        csr.free()


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_busy_stream(gpu, name, p):
    """both entry points only enqueue: on a non-default stream that is still busy they queue up behind its work, long segments and all"""
    rnd = random.Random(7)
    stream = ctypes.c_void_p()
    N.check(gpu.zk_stream_create(0, ctypes.byref(stream)))
    try:
        lengths = {(1, 0): ITEM + 9, (1, 1): 4, (1, 2): LONG_ROW + 2, (2, 1): 3, (0, 0): 2, (3, 2): 1}
        check(gpu, p, 2, rand_mats(rnd, p, 4, 64, lengths), rand_x(rnd, p, 64), rand_x(rnd, p, 3), stream=stream, n_long=1, n_items=3)
        check(gpu, p, 9, rand_mats(rnd, p, 512, 64, {(s, m): rnd.randrange(4) for s in range(500) for m in range(3)}), rand_x(rnd, p, 64),
              rand_x(rnd, p, 3), stream=stream)
    finally:
        N.check(gpu.zk_stream_destroy(stream))
