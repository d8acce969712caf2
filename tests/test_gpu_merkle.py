"""GPU: zksnake_amd.commitment.vector.Merkle / MerkleTree against the hashlib model (tests/merkle_model.py) and the vectors recorded
from the reference (tests/golden/merkle_vectors.json); every comparison is == on bytes."""

import ctypes
import json
import os
import random

import numpy as np
import pytest

import merkle_model as M
from zksnake_amd import _native as N
from zksnake_amd.commitment.vector import Merkle, MerkleTree
from zksnake_amd.constant import BN254_SCALAR_FIELD
from zksnake_amd.frvec import DevVec

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 16, 17)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "merkle_vectors.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def scheme(gpu):
    s = Merkle()
    s.setup()
    return s


def field_elements(n, seed):
    rnd = random.Random(seed)
    vals = [rnd.randrange(BN254_SCALAR_FIELD) for _ in range(n)]
    vals[0], vals[-1] = 0, BN254_SCALAR_FIELD - 1
    return vals


def test_three_input_kinds_give_the_same_tree(scheme):
    """a list of bytes, an array of rows and a DevVec over the same 32-byte leaves; a DevVec's leaf is int.to_bytes(32, "little")"""
    n = 77
    vals = field_elements(n, 1)
    items = [v.to_bytes(32, "little") for v in vals]
    limbs = N.ints_to_limbs(vals, 4)
    vec = DevVec(n)
    vec.upload(limbs)
    lv = M.levels(M.leaf_digests(items))
    trees = [scheme.tree(items), scheme.tree(np.frombuffer(b"".join(items), dtype=np.uint8).reshape(n, 32)), scheme.tree(vec)]
    for tree in trees:
        assert (tree.n, tree.depth, tree.root) == (n, 7, M.root(lv))
        assert tree.level(0).tobytes() == b"".join(lv[0]) and tree.level(tree.depth).tobytes() == tree.root
        for l in range(tree.depth + 1):
            assert tree.level(l).shape == (len(lv[l]), 64) and tree.level(l).tobytes() == b"".join(lv[l])
        tree.release()
    assert (vec.download() == limbs).all(), "the DevVec was written"
    assert scheme.commit(vec) == scheme.commit(items) == M.root(lv)


@pytest.mark.parametrize("n", SIZES)
def test_roots_equal_the_reference_and_every_opening_verifies(scheme, golden, n):
    items = [M.golden_leaf(i) for i in range(n)]   # lengths 0..4: the items kernel (n = 1: the rows kernel on empty rows)
    lv = M.levels(M.leaf_digests(items))
    rec = golden["trees"][str(n)]
    assert scheme.commit(items).hex() == rec["root"]
    tree = scheme.tree(items)
    assert tree.root.hex() == rec["root"] and tree.depth == len(lv) - 1
    for i in range(n):
        proof = tree.open(i)
        assert proof == M.path(lv, i) and len(proof) == tree.depth
        if rec["openings"][i]["verifies"]:
            assert [p.hex() for p in proof] == rec["openings"][i]["proof"]
        assert scheme.verify(tree.root, proof, i, items[i])
        assert not scheme.verify(tree.root, proof, i, items[i] + b"!")
        for l in range(len(proof)):
            bad = list(proof)
            bad[l] = bytes([bad[l][0] ^ 1]) + bad[l][1:]
            assert not scheme.verify(tree.root, bad, i, items[i])
        if n > 1 and proof[0] != lv[0][i]:
            assert not scheme.verify(tree.root, proof, i ^ 1, items[i])
    many = tree.open_many(list(range(n)) + [n - 1, 0])
    assert many.shape == (n + 2, tree.depth, 64) and many.dtype == np.uint8
    assert [[row.tobytes() for row in q] for q in many] == [tree.open(i) for i in list(range(n)) + [n - 1, 0]]
    assert tree.open_many([]).shape == (0, tree.depth, 64)
    tree.release()


def test_open_wrapper_and_index_rules(scheme):
    items = [M.golden_leaf(i) for i in range(5)]
    lv = M.levels(M.leaf_digests(items))
    assert scheme.open(items, 4) == M.path(lv, 4)          # the path on which the last node is its own sibling at two levels
    assert scheme.verify(scheme.commit(items), scheme.open(items, 4), 4, items[4])
    for index in (5, -1):
        with pytest.raises(IndexError):
            scheme.open(items, index)
    assert scheme.open(iter(items), 0) == M.path(lv, 0)    # any iterable of bytes-like items
    assert scheme.commit([bytearray(x) for x in items]) == scheme.commit([memoryview(x) for x in items]) == M.root(lv)


def test_a_long_list_of_mixed_lengths(scheme):
    rnd = random.Random(2)
    lens = [0, 1, 31, 32, 33, 127, 128, 129, 200]
    items = [rnd.randbytes(lens[rnd.randrange(len(lens))]) for _ in range(1 << 16)]
    lv = M.levels(M.leaf_digests(items))
    tree = scheme.tree(items)
    assert tree.root == M.root(lv) and tree.depth == 16
    assert tree.level(0).tobytes() == b"".join(lv[0])
    indices = [0, 1, (1 << 16) - 1, 12345, 40000]
    assert tree.open_many(indices).tobytes() == b"".join(b"".join(M.path(lv, i)) for i in indices)
    tree.release()


def test_equal_length_rows_that_are_not_a_multiple_of_eight(scheme):
    items = [bytes([i & 0xFF]) * 13 for i in range(300)]
    assert scheme.commit(items) == M.root(M.levels(M.leaf_digests(items)))
    arr = np.frombuffer(b"".join(items), dtype=np.uint8).reshape(300, 13)
    assert scheme.commit(arr) == scheme.commit(items)


def test_release_returns_the_memory(scheme, gpu):
    """the tree's allocation goes back to the library: the next allocation of that size gets the same block, and a released tree
    refuses to be read"""
    items = [bytes([i]) * 8 for i in range(100)]
    tree = scheme.tree(items)
    assert isinstance(tree, MerkleTree)
    ptr, nbytes = tree._buf.ptr, tree._buf.nbytes
    assert nbytes == tree.nodes * 64
    tree.release()
    assert tree._buf is None
    got = []   # the allocator keeps freed blocks by size: the tree's block is among the next few of its size
    try:
        for _ in range(8):
            again = ctypes.c_void_p()
            N.check(gpu.zk_dev_alloc(nbytes, ctypes.byref(again)))
            got.append(again.value)
            if again.value == ptr:
                break
        assert ptr in got, "the released block was not handed out again"
    finally:
        for p in got:
            N.check(gpu.zk_dev_free(p))
    for call in (lambda: tree.open(0), lambda: tree.open_many([1, 2]), lambda: tree.level(0)):
        with pytest.raises(RuntimeError):
            call()
    assert tree.root == M.root(M.levels(M.leaf_digests(items)))   # the root is host bytes and stays
    tree.release()   # twice is harmless
