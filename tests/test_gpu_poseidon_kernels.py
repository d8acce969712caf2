"""GPU: the kernels of csrc/poseidon.hip through the C ABI against the integer model (tests/poseidon_model.py), compared with ==
on limbs, on both curves.  Outputs are pre-filled with 0xA5 and followed by a guard region that must still hold 0xA5 afterwards.

Sizes: one lane, the edges of a wave (63, 64, 65), past one workgroup (257), and GRID + 3 items (GRID = 2^18 threads, 1024
workgroups of 256), the first size at which a thread takes a second item.  At that size input i is input i mod 257, so the model
runs 257 times and numpy spreads its values; the large tree has leaves of period 17 and the model hashes every distinct pair of
a level once."""

import functools
import random

import numpy as np
import pytest

import poseidon_model as M
import tree_model as T
from zksnake_amd import _native as N
from zksnake_amd.device import DeviceBuffer

pytestmark = pytest.mark.gpu

CURVES = ("BN254", "BLS12_381")
POISON = 0xA5
GUARD = 512
GRID = 1 << 18   # threads of the capped grid: 1024 workgroups of 256
PERIOD = 257


class Out:
    """a device buffer of `elems` elements of 0xA5 bytes and a guard of 0xA5 behind them"""

    def __init__(self, gpu, elems):
        self.elems = elems
        self.buf = DeviceBuffer(32 * elems + GUARD)
        N.check(gpu.zk_dev_memset(self.buf.ptr, POISON, 32 * elems + GUARD))

    @property
    def ptr(self):
        return self.buf.ptr

    def limbs(self):
        """the payload as (elems, 4) uint64, after checking the guard"""
        raw = self.buf.download((32 * self.elems + GUARD,), np.uint8)
        assert (raw[32 * self.elems:] == POISON).all(), "bytes behind the output were written"
        return raw[:32 * self.elems].view(np.uint64).reshape(self.elems, 4)


def limbs(values):
    return N.ints_to_limbs(list(values), 4)


@functools.lru_cache(maxsize=None)
def elements(curve, count, seed):
    """`count` seeded random elements"""
    rng = random.Random(f"{curve}/{seed}")
    return [rng.randrange(M.R[curve]) for _ in range(count)]


def rows(curve, n, width, seed):
    """n rows of `width` elements: row 0 all zero, row 1 all r - 1 (where there are that many), the rest seeded random"""
    r = M.R[curve]
    flat = list(elements(curve, PERIOD * 9, seed)[:n * width])
    flat[:width] = [0] * width
    if n > 1:
        flat[width:2 * width] = [r - 1] * width
    return [tuple(flat[i * width:(i + 1) * width]) for i in range(n)]


@functools.lru_cache(maxsize=None)
def model_perm(curve, state):
    return tuple(M.perm(curve, list(state)))


@functools.lru_cache(maxsize=None)
def model_hash(curve, row):
    return M.hash(curve, list(row))


@functools.lru_cache(maxsize=None)
def model_sponge(curve, row):
    return M.sponge(curve, list(row))


def upload(flat):
    return DeviceBuffer.from_numpy(limbs(flat))


# ---- permutation --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", M.WIDTHS)
@pytest.mark.parametrize("curve", CURVES)
def test_perm(gpu, curve, t):
    """out of place with the input left as it was, and in place, at every size"""
    cid = N.curve_id(curve)
    for n in (1, 63, 64, 65, 257):
        states = rows(curve, n, t, "perm")
        flat = [x for s in states for x in s]
        want = limbs([x for s in states for x in model_perm(curve, s)])
        src, out = upload(flat), Out(gpu, n * t)
        N.check(gpu.zk_poseidon_perm_dev(cid, t, n, src.ptr, out.ptr, None))
        assert (out.limbs() == want).all(), f"n = {n}"
        assert (src.download((n * t, 4)) == limbs(flat)).all(), f"n = {n}: the input changed"
        inplace = Out(gpu, n * t)
        inplace.buf.upload(limbs(flat))
        N.check(gpu.zk_poseidon_perm_dev(cid, t, n, inplace.ptr, inplace.ptr, None))
        assert (inplace.limbs() == want).all(), f"n = {n}, in place"


@pytest.mark.parametrize("k", (2, 3, 4))
@pytest.mark.parametrize("curve", CURVES)
def test_hash(gpu, curve, k):
    cid, n = N.curve_id(curve), 257
    data = rows(curve, n, k, "hash")
    src, out = upload([x for row in data for x in row]), Out(gpu, n)
    N.check(gpu.zk_poseidon_hash_dev(cid, k, n, src.ptr, out.ptr, None))
    assert (out.limbs() == limbs(model_hash(curve, row) for row in data)).all()


def test_hash_of_1_2_3_is_the_fixture_value(gpu):
    src, out = upload([1, 2, 3]), Out(gpu, 1)
    N.check(gpu.zk_poseidon_hash_dev(0, 3, 1, src.ptr, out.ptr, None))
    assert N.limbs_to_ints(out.limbs()) == [0x0E7732D89E6939C0FF03D5E58DAB6302F3230E269DC5B968F725DF34AB36D732]


@pytest.mark.parametrize("length", (1, 2, 3, 4, 5, 8, 9))
@pytest.mark.parametrize("curve", CURVES)
def test_sponge_rows(gpu, curve, length):
    """odd lengths end in a block of one element, which adds nothing to state[2]"""
    cid, n = N.curve_id(curve), 65
    data = rows(curve, n, length, "sponge")
    src, out = upload([x for row in data for x in row]), Out(gpu, n)
    N.check(gpu.zk_poseidon_sponge_rows_dev(cid, n, src.ptr, length, out.ptr, None))
    assert (out.limbs() == limbs(model_sponge(curve, row) for row in data)).all()


# ---- past the capped grid -------------------------------------------------------------------------------------------------

def periodic(base_rows, n):
    """(n * width, 4) limbs: row i is base_rows[i mod PERIOD]"""
    width = len(base_rows[0])
    base = limbs(x for row in base_rows for x in row).reshape(PERIOD, width, 4)
    return np.ascontiguousarray(base[np.arange(n) % PERIOD]).reshape(n * width, 4)


@pytest.mark.parametrize("curve", CURVES)
def test_perm_takes_a_second_item(gpu, curve):
    cid, n, t = N.curve_id(curve), GRID + 3, 3
    base = rows(curve, PERIOD, t, "perm")
    src, out = DeviceBuffer.from_numpy(periodic(base, n)), Out(gpu, n * t)
    N.check(gpu.zk_poseidon_perm_dev(cid, t, n, src.ptr, out.ptr, None))
    assert (out.limbs() == periodic([model_perm(curve, s) for s in base], n)).all()


@pytest.mark.parametrize("curve", CURVES)
def test_hash_takes_a_second_item(gpu, curve):
    cid, n, k = N.curve_id(curve), GRID + 3, 2
    base = rows(curve, PERIOD, k, "hash")
    src, out = DeviceBuffer.from_numpy(periodic(base, n)), Out(gpu, n)
    N.check(gpu.zk_poseidon_hash_dev(cid, k, n, src.ptr, out.ptr, None))
    assert (out.limbs() == periodic([(model_hash(curve, row),) for row in base], n)).all()


@pytest.mark.parametrize("curve", CURVES)
def test_sponge_takes_a_second_item(gpu, curve):
    cid, n, length = N.curve_id(curve), GRID + 3, 3
    base = rows(curve, PERIOD, length, "sponge")
    src, out = DeviceBuffer.from_numpy(periodic(base, n)), Out(gpu, n)
    N.check(gpu.zk_poseidon_sponge_rows_dev(cid, n, src.ptr, length, out.ptr, None))
    assert (out.limbs() == periodic([(model_sponge(curve, row),) for row in base], n)).all()


# ---- trees ----------------------------------------------------------------------------------------------------------------

def model_levels(curve, leaves):
    """M.levels with every distinct (left, right) of the tree hashed once"""
    return T.levels(leaves, functools.lru_cache(maxsize=None)(lambda left, right: M.hash(curve, [left, right])))


def build(gpu, curve, leaves):
    """(the tree's nodes as limbs, the model's levels) over level 0 = leaves"""
    n = len(leaves)
    lv = model_levels(curve, leaves)
    nodes = sum(len(level) for level in lv)
    tree = Out(gpu, nodes)
    tree.buf.upload(limbs(leaves))
    N.check(gpu.zk_poseidon_merkle_build_dev(N.curve_id(curve), n, tree.ptr, None))
    return tree, lv


@pytest.mark.parametrize("n", (1, 2, 3, 5, 8, 9, 257, 1000))
@pytest.mark.parametrize("curve", CURVES)
def test_merkle_build(gpu, curve, n):
    """every level against the model: odd widths hash their last node with itself, one leaf is its own root"""
    leaves = [row[0] for row in rows(curve, n, 1, "tree")]
    tree, lv = build(gpu, curve, leaves)
    assert M.levels(curve, leaves[:9]) == model_levels(curve, leaves[:9])
    got, at = tree.limbs(), 0
    for l, level in enumerate(lv):
        assert (got[at:at + len(level)] == limbs(level)).all(), f"level {l}"
        at += len(level)
    assert at == len(got)


@pytest.mark.parametrize("n", (GRID + 3, 2 * GRID + 3))
@pytest.mark.parametrize("curve", CURVES)
def test_merkle_build_past_the_grid(gpu, curve, n):
    """GRID + 3 leaves, and 2 GRID + 3, where level 1 has GRID + 2 parents and a thread takes a second one.  Leaves of period 17,
    every level against the model"""
    base = [row[0] for row in rows(curve, 17, 1, "tree")]
    leaves = [base[i % 17] for i in range(n)]
    tree, lv = build(gpu, curve, leaves)
    assert len(lv[1]) == (n + 1) // 2 and len(lv[-1]) == 1
    got, at = tree.limbs(), 0
    for l, level in enumerate(lv):
        assert (got[at:at + len(level)] == limbs(level)).all(), f"level {l}"
        at += len(level)
    assert at == len(got)


@pytest.mark.parametrize("n", (5, 9))
@pytest.mark.parametrize("curve", CURVES)
def test_merkle_paths(gpu, curve, n):
    """every index, an index past the leaves (it opens the last leaf) and k = 0"""
    leaves = [row[0] for row in rows(curve, n, 1, "tree")]
    tree, lv = build(gpu, curve, leaves)
    depth = len(lv) - 1
    indices = list(range(n)) + [n, n + 7, 2**63]
    d_idx = DeviceBuffer.from_numpy(np.array(indices, dtype=np.uint64))
    out = Out(gpu, len(indices) * depth)
    N.check(gpu.zk_poseidon_merkle_paths_dev(n, tree.ptr, len(indices), d_idx.ptr, out.ptr, None))
    want = [x for i in indices for x in M.path(lv, min(i, n - 1))]
    assert (out.limbs() == limbs(want)).all()
    for q, i in enumerate(indices[:n]):
        assert M.verify(curve, M.root(lv), want[q * depth:(q + 1) * depth], i, leaves[i])
    untouched = Out(gpu, depth)
    N.check(gpu.zk_poseidon_merkle_paths_dev(n, tree.ptr, 0, d_idx.ptr, untouched.ptr, None))
    assert (untouched.limbs().view(np.uint8) == POISON).all()


def numbered_tree(n):
    """(levels of node numbers, the tree as (nodes, 4) limbs): limb c of node j holds 4 j + c, so every word of the tree is its
    own value and a gathered node names where it came from"""
    lv, width = [], n
    while True:
        first = lv[-1][-1] + 1 if lv else 0
        lv.append(list(range(first, first + width)))
        if width == 1:
            break
        width = (width + 1) // 2
    nodes = lv[-1][0] + 1
    return lv, np.arange(4 * nodes, dtype=np.uint64).reshape(nodes, 4)


def run_numbered_paths(gpu, n, indices):
    """(k, depth, 4) limbs gathered from the numbered tree, and the same from the model's paths"""
    lv, nodes = numbered_tree(n)
    depth, k = len(lv) - 1, len(indices)
    tree = DeviceBuffer.from_numpy(nodes)
    d_idx = DeviceBuffer.from_numpy(np.array(indices, dtype=np.uint64))
    out = Out(gpu, k * depth)
    N.check(gpu.zk_poseidon_merkle_paths_dev(n, tree.ptr, k, d_idx.ptr, out.ptr, None))
    table = np.array([T.path(lv, i) for i in range(n)], dtype=np.int64).reshape(n, depth)
    return out.limbs().reshape(k, depth, 4), nodes[table[np.array(indices, dtype=np.int64)]]


@pytest.mark.parametrize("n", (1, 2, 3, 5, 8, 13, 257))
def test_merkle_paths_at_every_index(gpu, n):
    """the gather alone, on a tree that was uploaded and not hashed: every index and some again, depth 0 to 9, odd widths at the
    bottom, in the middle and below the root, past one workgroup"""
    got, want = run_numbered_paths(gpu, n, list(range(n)) + [0, n - 1, n - 1, n // 2])
    assert got.shape == want.shape and (got == want).all()


def test_merkle_paths_past_one_grid(gpu):
    n, k = 13, (1 << 16) + 1   # k * depth = 2^18 + 4 entries: threads 0 .. 3 take a second one
    rnd = random.Random(21)
    indices = [rnd.randrange(n) for _ in range(k)]
    indices[0], indices[-1] = n - 1, n - 1
    got, want = run_numbered_paths(gpu, n, indices)
    assert got.shape == want.shape == (k, 4, 4) and k * 4 > GRID and (got == want).all()


def test_one_leaf_has_empty_paths(gpu):
    tree, lv = build(gpu, "BN254", [12345])
    d_idx = DeviceBuffer.from_numpy(np.zeros(4, dtype=np.uint64))
    untouched = Out(gpu, 4)
    N.check(gpu.zk_poseidon_merkle_paths_dev(1, tree.ptr, 4, d_idx.ptr, untouched.ptr, None))
    assert (untouched.limbs().view(np.uint8) == POISON).all() and N.limbs_to_ints(tree.limbs()) == [12345]
