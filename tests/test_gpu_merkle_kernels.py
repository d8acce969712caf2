"""GPU: the kernels of csrc/merkle.hip through the C ABI against the hashlib model (tests/merkle_model.py), compared with == on
bytes.  Outputs are pre-filled with 0xA5 and followed by a guard region that must still hold 0xA5 afterwards.

Sizes past one workgroup and past the capped grid (GRID = 2^18 threads, 1024 workgroups of 256): the row hasher at GRID + 5 rows
and the tree at 2 GRID + 3 leaves (the first sizes at which a thread takes a second row, a second parent), the paths at
2^18 + 4 entries, and the item hasher at 600 items (three workgroups, the first case past one) and at GRID + 5 items, whose
lengths cycle through aligned and unaligned starts inside every wave and whose five second items are 129 to 300 bytes long,
once hashed in full and once with the last two offsets beyond data_bytes, so that the clamp acts in a second item."""

import random

import numpy as np
import pytest

import merkle_model as M
import stream_state_child as S
from zksnake_amd import _native as N
from zksnake_amd.device import DeviceBuffer

pytestmark = pytest.mark.gpu

D = M.DIGEST
POISON = 0xA5
GUARD = 512
GRID = 1 << 18   # threads of the capped grid: 1024 workgroups of 256


class Out:
    """a device buffer of `nbytes` bytes of 0xA5 and a guard of 0xA5 behind them"""

    def __init__(self, gpu, nbytes):
        self.nbytes = nbytes
        self.buf = DeviceBuffer(nbytes + GUARD)
        N.check(gpu.zk_dev_memset(self.buf.ptr, POISON, nbytes + GUARD))

    @property
    def ptr(self):
        return self.buf.ptr

    def bytes(self):
        """the payload, after checking the guard"""
        raw = self.buf.download((self.nbytes + GUARD,), np.uint8)
        assert (raw[self.nbytes:] == POISON).all(), "bytes behind the output were written"
        return raw[:self.nbytes].tobytes()


def rand_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


def chunks(raw, size):
    return [raw[i:i + size] for i in range(0, len(raw), size)]


def rows_data(n, row_bytes, seed):
    data = rand_bytes(n * row_bytes, seed).reshape(n, row_bytes)
    if n >= 2:
        data[0], data[n - 1] = 0x00, 0xFF
    return data


def run_rows(gpu, data, shift=0):
    """digests of the rows of `data`, uploaded `shift` bytes past the start of an allocation"""
    n, row_bytes = data.shape
    src = DeviceBuffer(data.nbytes + shift + 16)
    if data.nbytes:
        src.upload(data, shift)
    out = Out(gpu, n * D)
    N.check(gpu.zk_blake2b_rows_dev(n, src.ptr + shift, row_bytes, out.ptr, None))
    return out.bytes()


ROW_BYTES = (0, 1, 7, 8, 31, 32, 63, 64, 96, 127, 128, 129, 255, 256, 257, 300)


@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_rows(gpu, row_bytes):
    """one lane, past one wave, past one workgroup; 64-bit loads where the row length allows them, and the same rows from a base
    one byte past an allocation's start, which forces byte loads"""
    for n in (1, 3, 65, 257):
        data = rows_data(n, row_bytes, 1000 * row_bytes + n)
        want = b"".join(M.H(row.tobytes()) for row in data)
        assert run_rows(gpu, data) == want, f"n = {n}"
        if n == 65:
            assert run_rows(gpu, data, shift=1) == want, "byte path"


def test_rows_null_source_with_no_bytes(gpu):
    out = Out(gpu, 3 * D)
    N.check(gpu.zk_blake2b_rows_dev(3, None, 0, out.ptr, None))
    assert out.bytes() == M.H(b"") * 3


def run_items(gpu, data, offsets, data_bytes):
    n = len(offsets) - 1
    src, off = DeviceBuffer.from_numpy(data), DeviceBuffer.from_numpy(np.array(offsets, dtype=np.uint64))
    out = Out(gpu, n * D)
    N.check(gpu.zk_blake2b_items_dev(n, src.ptr, data_bytes, off.ptr, out.ptr, None))
    return out.bytes()


def test_items_of_mixed_lengths_in_one_wave(gpu):
    lens = [0, 1, 127, 128, 129, 256, 257, 1000, 64, 0] * 7
    offsets = [0]
    for x in lens:
        offsets.append(offsets[-1] + x)
    data = rand_bytes(offsets[-1], 7)
    raw = data.tobytes()
    want = b"".join(M.H(raw[a:b]) for a, b in zip(offsets, offsets[1:]))
    assert len(lens) == 70 and run_items(gpu, data, offsets, len(raw)) == want


def test_items_offsets_past_the_data_are_clamped(gpu):
    """off[n] and an inner offset lie beyond data_bytes, inside an allocation that really is that large: the digests are those of
    the clamped ranges (without the clamp they would be other digests, of memory that exists)"""
    real, data_bytes = 3000, 2000
    data = rand_bytes(real, 8)
    offsets = [0, 500, 2500, 2600, real]
    raw = data.tobytes()
    want = b"".join(M.H(raw[min(a, min(b, data_bytes)):min(b, data_bytes)]) for a, b in zip(offsets, offsets[1:]))
    assert want == M.H(raw[:500]) + M.H(raw[500:2000]) + M.H(b"") * 2
    assert want != b"".join(M.H(raw[a:b]) for a, b in zip(offsets, offsets[1:]))
    assert run_items(gpu, data, offsets, data_bytes) == want


ITEM_PATTERN = (0, 1, 7, 8, 9, 16, 33, 64, 0, 24)   # 162 bytes a cycle: the starts drift through every residue mod 8
ITEM_TAIL = (129, 256, 3, 200, 300)                 # items GRID .. GRID + 4, the second items of threads 0 .. 4


@pytest.fixture(scope="module")
def many_items():
    """(data, offsets, digests) of GRID + 5 items: hashlib over every item in full, computed once"""
    lens = [ITEM_PATTERN[i % len(ITEM_PATTERN)] for i in range(GRID)] + list(ITEM_TAIL)
    offsets = np.concatenate([[0], np.cumsum(lens)]).tolist()
    data = rand_bytes(offsets[-1], 19)
    raw = data.tobytes()
    starts = {offsets[i] % 8 for i in range(64)}
    assert 0 in starts and len(starts) > 4, "aligned and unaligned starts inside one wave"
    assert offsets[GRID] % 8 and offsets[GRID + 1] % 8 and offsets[GRID + 3] % 8 == 0 and offsets[GRID + 4] % 8 == 0
    return data, offsets, [M.H(raw[a:b]) for a, b in zip(offsets, offsets[1:])]


def test_items_past_one_workgroup(gpu, many_items):
    """600 items: three workgroups, the last one partly idle"""
    data, offsets, digests = many_items
    assert run_items(gpu, data[:offsets[600]], offsets[:601], offsets[600]) == b"".join(digests[:600])


def test_items_past_one_grid(gpu, many_items):
    """GRID + 5 items of about 4 MB: threads 0 .. 4 take a second item, of 129 and 256 bytes from starts that are no multiple of
    8 and of 200 and 300 bytes from starts that are.  With data_bytes at the end of the allocation every item is hashed in full;
    with data_bytes 77 bytes into item GRID + 3 the last two offsets lie beyond it, inside the same allocation, and the clamp
    acts in two second items: item GRID + 3 is its first 77 bytes and item GRID + 4 is empty."""
    data, offsets, digests = many_items
    n = GRID + 5
    assert len(digests) == n and 4_000_000 < len(data) == offsets[n] < 4_500_000
    got = run_items(gpu, data, offsets, offsets[n])
    wrong = [i for i in range(n) if got[i * D:(i + 1) * D] != digests[i]]
    assert not wrong, f"{len(wrong)} of {n} digests differ, the first is item {wrong[0]} (GRID = {GRID})"
    data_bytes = offsets[GRID + 3] + 77
    assert offsets[n - 2] < data_bytes < offsets[n - 1] < offsets[n]
    raw = data.tobytes()
    clamped = digests[:GRID + 3] + [M.H(raw[offsets[GRID + 3]:data_bytes]), M.H(b"")]
    assert clamped[-2:] != digests[-2:]
    got = run_items(gpu, data, offsets, data_bytes)
    wrong = [i for i in range(n) if got[i * D:(i + 1) * D] != clamped[i]]
    assert not wrong, f"clamped: {len(wrong)} of {n} digests differ, the first is item {wrong[0]} (GRID = {GRID})"


def test_rows_past_one_grid(gpu):
    n = GRID + 5   # the first size at which a thread takes a second row
    data = rows_data(n, 32, 9)
    assert run_rows(gpu, data) == b"".join(M.H(row) for row in chunks(data.tobytes(), 32))


def run_build(gpu, n, leaves):
    """the whole tree over the n 64-byte nodes in `leaves` (bytes)"""
    nodes = M.layout(n)[2]
    tree = Out(gpu, nodes * D)
    tree.buf.upload(np.frombuffer(leaves, dtype=np.uint8))
    N.check(gpu.zk_merkle_build_dev(n, tree.ptr, None))
    return tree


BUILD_SIZES = tuple(range(1, 10)) + (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)


@pytest.mark.parametrize("n", BUILD_SIZES)
def test_build(gpu, n):
    """around every admissible threshold of the one-workgroup tail; odd levels at the bottom, in the middle and below the root"""
    leaves = rand_bytes(n * D, 100 + n).tobytes()
    got = run_build(gpu, n, leaves).bytes()
    assert got[:n * D] == leaves, "level 0 was written"
    assert got == M.tree_bytes(M.levels(chunks(leaves, D)))


N_BIG = 2 * GRID + 3   # level 1 has 2^18 + 2 parents: the first size at which a thread takes a second parent


@pytest.fixture(scope="module")
def big(gpu):
    """(items, model levels, the device tree) of 2^19 + 3 leaves of 32 bytes, hashed and built on the device"""
    data = rows_data(N_BIG, 32, 11)
    lv = M.levels([M.H(row) for row in chunks(data.tobytes(), 32)])
    src = DeviceBuffer.from_numpy(data)
    tree = Out(gpu, M.layout(N_BIG)[2] * D)
    N.check(gpu.zk_blake2b_rows_dev(N_BIG, src.ptr, 32, tree.ptr, None))
    N.check(gpu.zk_merkle_build_dev(N_BIG, tree.ptr, None))
    return data, lv, tree


def test_build_past_one_grid(big):
    _, lv, tree = big
    assert tree.bytes() == M.tree_bytes(lv)


def run_paths(gpu, n, tree_ptr, indices):
    depth = M.layout(n)[0]
    idx = DeviceBuffer.from_numpy(np.array(indices, dtype=np.uint64))
    out = Out(gpu, len(indices) * depth * D)
    N.check(gpu.zk_merkle_paths_dev(n, tree_ptr, len(indices), idx.ptr, out.ptr, None))
    return out.bytes()


def want_paths(lv, indices):
    return b"".join(b"".join(M.path(lv, i)) for i in indices)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 13, 257])
def test_paths_at_every_index(gpu, n):
    leaves = rand_bytes(n * D, 200 + n).tobytes()
    lv = M.levels(chunks(leaves, D))
    tree = run_build(gpu, n, leaves)
    indices = list(range(n)) + [0, n - 1, n - 1, n // 2]
    assert run_paths(gpu, n, tree.ptr, indices) == want_paths(lv, indices)


@pytest.mark.parametrize("n", [5, 9])
def test_paths_of_indices_past_the_leaves(gpu, n):
    """an index at or past n opens the last leaf: the clamp of the kernel, which the Python layer never reaches"""
    leaves = rand_bytes(n * D, 300 + n).tobytes()
    lv = M.levels(chunks(leaves, D))
    tree = run_build(gpu, n, leaves)
    indices = list(range(n)) + [n, n + 7, 2**63]
    assert run_paths(gpu, n, tree.ptr, indices) == want_paths(lv, [min(i, n - 1) for i in indices])


def test_paths_in_a_large_tree(gpu, big):
    _, lv, tree = big
    n = N_BIG
    rnd = random.Random(12)
    indices = [0, 1, n - 1, n - 2, GRID, GRID - 1, GRID + 1] + [rnd.randrange(n) for _ in range(100)]
    assert run_paths(gpu, n, tree.ptr, indices) == want_paths(lv, indices)


def test_paths_past_one_grid(gpu):
    n, k = 13, (1 << 16) + 1   # k * depth = 2^18 + 4 entries
    leaves = rand_bytes(n * D, 13).tobytes()
    lv = M.levels(chunks(leaves, D))
    tree = run_build(gpu, n, leaves)
    rnd = random.Random(14)
    indices = [rnd.randrange(n) for _ in range(k)]
    indices[0], indices[-1] = n - 1, n - 1
    table = [b"".join(M.path(lv, i)) for i in range(n)]
    assert M.layout(n)[0] * k > GRID
    assert run_paths(gpu, n, tree.ptr, indices) == b"".join(table[i] for i in indices)


def test_paths_of_no_queries(gpu):
    tree = run_build(gpu, 5, rand_bytes(5 * D, 15).tobytes())
    out = Out(gpu, D)
    assert gpu.zk_merkle_paths_dev(5, tree.ptr, 0, out.ptr, out.ptr, None) == N.ZK_OK
    assert gpu.zk_merkle_paths_dev(5, tree.ptr, 0, None, None, None) == N.ZK_OK
    assert out.bytes() == bytes([POISON]) * D


def test_chain_on_a_parked_stream(gpu):
    """rows -> build -> paths on a created stream behind zk_debug_spin_dev, the rows and the indices arriving behind the spin: the
    results equal those of the same chain on the default stream, and differ from what the stale device content would give"""
    n, k = 2500, 40   # two launches of the level kernel, then the tail
    depth, _, nodes = M.layout(n)
    real, stale = rows_data(n, 32, 16), rows_data(n, 32, 17)
    rnd = random.Random(18)
    idx_real = np.array([rnd.randrange(n) for _ in range(k)], dtype=np.uint64)
    idx_stale = np.array([(int(i) + 7) % n for i in idx_real], dtype=np.uint64)

    def chain(rows_ptr, idx_ptr, st, tree, paths):
        N.check(gpu.zk_blake2b_rows_dev(n, rows_ptr, 32, tree.ptr, st))
        N.check(gpu.zk_merkle_build_dev(n, tree.ptr, st))
        N.check(gpu.zk_merkle_paths_dev(n, tree.ptr, k, idx_ptr, paths.ptr, st))
        return tree, paths

    d_rows, d_idx = DeviceBuffer.from_numpy(real), DeviceBuffer.from_numpy(idx_real)
    plain = tuple(o.bytes() for o in chain(d_rows.ptr, d_idx.ptr, None, Out(gpu, nodes * D), Out(gpu, k * depth * D)))
    rows, idx = S.Staged(stale, real), S.Staged(idx_stale, idx_real)
    tree, paths = Out(gpu, nodes * D), Out(gpu, k * depth * D)   # allocated and filled before the stream is parked
    outs = S.behind_spin(gpu, [rows, idx], lambda st: chain(rows.ptr, idx.ptr, st, tree, paths))
    parked = tuple(o.bytes() for o in outs)

    def model(data, indices):
        lv = M.levels([M.H(row) for row in chunks(data.tobytes(), 32)])
        return M.tree_bytes(lv), want_paths(lv, [int(i) for i in indices])

    on_real, on_stale = model(real, idx_real), model(stale, idx_stale)
    assert plain == on_real
    S.settle(parked[0], on_real[0], on_stale[0])
    S.settle(parked[1], on_real[1], on_stale[1])
    assert parked == plain
