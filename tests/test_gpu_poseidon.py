"""GPU: zksnake_amd.hash.Poseidon and zksnake_amd.commitment.vector.PoseidonMerkle end to end, checked with the host verifier
and the integer model (tests/poseidon_model.py)."""

import random

import numpy as np
import pytest

import poseidon_model as M
from zksnake_amd import _native as N
from zksnake_amd.commitment.vector import PoseidonMerkle, PoseidonMerkleTree
from zksnake_amd.frvec import DevVec
from zksnake_amd.hash import Poseidon

pytestmark = pytest.mark.gpu

CURVES = ("BN254", "BLS12_381")
FIXTURE_1_2_3 = 0x0E7732D89E6939C0FF03D5E58DAB6302F3230E269DC5B968F725DF34AB36D732


def ints(vec):
    return N.limbs_to_ints(vec.download())


def test_hash_many_of_1_2_3_is_the_fixture_value(gpu):
    assert ints(Poseidon("BN254").hash_many([[1, 2, 3]])) == [FIXTURE_1_2_3]


@pytest.mark.parametrize("curve", CURVES)
def test_the_three_input_forms_agree_with_the_host(gpu, curve):
    """a list of rows, an (n, k, 4) limb array and a DevVec with a row length, for permute_many, hash_many and sponge_many"""
    h, rng = Poseidon(curve), random.Random(curve)
    rows = [[rng.randrange(h.p) for _ in range(3)] for _ in range(7)]
    arr = N.ints_to_limbs([x for row in rows for x in row], 4).reshape(7, 3, 4)
    vec = DevVec(21, zero=False)
    vec.upload(arr.reshape(21, 4))
    for call, k, want in ((h.permute_many, 3, [x for row in rows for x in h.permute(row)]),
                          (h.hash_many, 3, [h.hash(row) for row in rows]),
                          (h.sponge_many, 3, [h.sponge(row) for row in rows])):
        assert ints(call(rows)) == ints(call(arr)) == ints(call(vec, k)) == want
    assert ints(h.sponge_many(vec, 1)) == [M.sponge(curve, [x]) for row in rows for x in row]
    assert ints(h.sponge_many(vec, 7)) == [M.sponge(curve, [x for row in rows for x in row][7 * i:7 * i + 7]) for i in range(3)]


@pytest.mark.parametrize("n", (1, 3, 5, 1000))
@pytest.mark.parametrize("curve", CURVES)
def test_round_trip(gpu, curve, n):
    """commit, open every index (a sample of them at n = 1000) from one tree, verify on the host; tampering is rejected"""
    scheme, rng = PoseidonMerkle(curve), random.Random(f"{curve}/{n}")
    scheme.setup()
    vector = [[rng.randrange(scheme.order), rng.randrange(scheme.order), i] for i in range(n)]
    root = scheme.commit(vector)
    tree = scheme.tree(vector)
    try:
        assert isinstance(tree, PoseidonMerkleTree) and tree.root == root and tree.n == n and tree.depth == (n - 1).bit_length()
        assert tree.nodes == sum(len(tree.level(l)) for l in range(tree.depth + 1))
        assert N.limbs_to_ints(tree.level(tree.depth)) == [root]
        assert N.limbs_to_ints(tree.level(0)[:3]) == [M.sponge(curve, row) for row in vector[:3]]
        indices = list(range(n)) if n <= 5 else [0, 1, 2, 499, 500, 997, 998, 999]
        paths = tree.open_many(indices)
        assert paths.shape == (len(indices), tree.depth, 4) and paths.dtype == np.uint64
        for q, i in enumerate(indices):
            proof = tree.open(i)
            assert proof == N.limbs_to_ints(paths[q]) if tree.depth else proof == []
            assert len(proof) == tree.depth and scheme.verify(root, proof, i, vector[i])
            assert not scheme.verify(root, proof, i, vector[i][:2] + [vector[i][2] + 1])
            assert not scheme.verify(root + 1, proof, i, vector[i])
            if tree.depth and proof[0] != scheme.hasher.sponge(vector[i]):   # a leaf that is its own sibling sits on either side
                assert not scheme.verify(root, proof, i ^ 1, vector[i])
            if tree.depth:
                assert not scheme.verify(root, [proof[0] ^ 1] + proof[1:], i, vector[i])
    finally:
        tree.release()
    assert scheme.open(vector, n - 1) == proof
    if n == 5:
        lv = M.levels(curve, [M.sponge(curve, row) for row in vector])
        assert root == M.root(lv) and proof == M.path(lv, 4)


@pytest.mark.parametrize("curve", CURVES)
def test_the_four_vector_forms_give_one_root(gpu, curve):
    scheme, rng = PoseidonMerkle(curve), random.Random(curve)
    values = [rng.randrange(scheme.order) for _ in range(9)]
    arr = N.ints_to_limbs(values, 4)
    vec = DevVec(9, zero=False)
    vec.upload(arr)
    want = M.root(M.levels(curve, [M.sponge(curve, [x]) for x in values]))
    assert scheme.commit(values) == scheme.commit([[x] for x in values]) == scheme.commit(arr.reshape(9, 1, 4)) == scheme.commit(vec) == want
    assert N.limbs_to_ints(vec.download()) == values   # hashed in place, not modified
    proof = scheme.open(vec, 8)
    assert scheme.verify(want, proof, 8, values[8]) and scheme.verify(want, proof, 8, [values[8]])


def test_a_released_tree_raises(gpu):
    tree = PoseidonMerkle().tree([1, 2, 3])
    assert tree.open(2) and tree.root
    tree.release()
    tree.release()   # twice is fine
    with pytest.raises(RuntimeError):
        tree.open(0)
    with pytest.raises(RuntimeError):
        tree.open_many([0, 1])
    with pytest.raises(RuntimeError):
        tree.level(0)
    with pytest.raises(IndexError):
        tree.open(3)   # the index is still checked first
