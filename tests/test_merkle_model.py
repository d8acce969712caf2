"""CPU: tests/merkle_model.py against the vectors recorded from the reference's Merkle (tests/golden/merkle_vectors.json, written by
tests/golden/gen_merkle_golden.py), against RFC 7693, and against the library's layout arithmetic (zk_merkle_layout: no GPU)."""

import ctypes
import json
import os

import numpy as np
import pytest

import merkle_model as M
from zksnake_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 16, 17)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "merkle_vectors.json")) as f:
        return json.load(f)


def model_levels(n):
    return M.levels(M.leaf_digests([M.golden_leaf(i) for i in range(n)]))


def test_golden_file_covers_the_sizes(golden):
    assert golden["alg"] == "blake2b" and sorted(map(int, golden["trees"])) == sorted(SIZES)
    for n in SIZES:
        assert len(golden["trees"][str(n)]["openings"]) == n
    assert os.path.getsize(os.path.join(HERE, "golden", "merkle_vectors.json")) < 100_000


@pytest.mark.parametrize("n", SIZES)
def test_model_roots_and_proofs_equal_the_reference(golden, n):
    """every root; every proof where the reference's own proof verifies -- which is every index when n is a power of two -- and
    where it does not, the reference's proof is the model's without the levels at which the node had no sibling"""
    rec, lv = golden["trees"][str(n)], model_levels(n)
    assert M.root(lv).hex() == rec["root"]
    for i, opening in enumerate(rec["openings"]):
        mine = [p.hex() for p in M.path(lv, i)]
        if opening["verifies"]:
            assert mine == opening["proof"], f"index {i}"
        else:
            assert len(opening["proof"]) < len(mine) and all(p in mine for p in opening["proof"]), f"index {i}"
    if n & (n - 1) == 0:
        assert all(o["verifies"] for o in rec["openings"])


def test_the_reference_rejects_its_own_proofs_where_a_sibling_is_missing(golden):
    """the finding DESIGN.md 4.12 states, as recorded: these proofs fail in the reference itself"""
    failing = {(n, i) for n in SIZES for i, o in enumerate(golden["trees"][str(n)]["openings"]) if not o["verifies"]}
    for case in ((3, 2), (5, 4), (6, 4), (6, 5), (7, 6), (9, 8), (13, 12), (17, 16)):
        assert case in failing
    assert not any(n & (n - 1) == 0 for n, _ in failing)


@pytest.mark.parametrize("n", SIZES + (31, 33, 100))
def test_model_proofs_verify_at_every_index(n):
    lv = model_levels(n)
    depth, offsets, nodes = M.layout(n)
    assert len(lv) == depth + 1 and [len(x) for x in lv] == [b - a for a, b in zip(offsets, offsets[1:] + [nodes])]
    assert len(M.tree_bytes(lv)) == nodes * M.DIGEST and M.tree_bytes(lv)[-M.DIGEST:] == M.root(lv)
    for i in range(n):
        proof = M.path(lv, i)
        assert len(proof) == depth
        assert M.verify(M.root(lv), proof, i, M.golden_leaf(i))
        assert not M.verify(M.root(lv), proof, i, M.golden_leaf(i) + b"x")
        if n > 1:
            assert not M.verify(M.root(lv), proof, i ^ 1, M.golden_leaf(i)) or proof[0] == lv[0][i]


def test_rfc7693_abc():
    want = ("ba80a53f981c4d0d6a2797b69f12f6e94c212f14685ac4b74b12bb6fdbffa2d1"
            "7d87c5392aab792dc252d5de4533cc9518d38aa8dbf1925ab92386edd4009923")
    assert M.H(b"abc").hex() == want


def layout_of(lib, n):
    depth, nodes = ctypes.c_int(-1), ctypes.c_uint64(0)
    offsets = np.full(N.MERKLE_MAX_LOG + 1, 2**64 - 1, dtype=np.uint64)
    status = lib.zk_merkle_layout(n, ctypes.byref(depth), N.u64p(offsets), ctypes.byref(nodes))
    return status, depth.value, [int(x) for x in offsets], nodes.value


@pytest.mark.parametrize("n", list(range(1, 71)) + [1 << 26])
def test_library_layout_equals_the_model(lib, n):
    status, depth, offsets, nodes = layout_of(lib, n)
    want_depth, want_offsets, want_nodes = M.layout(n)
    assert status == N.ZK_OK and (depth, nodes) == (want_depth, want_nodes)
    assert offsets[:depth + 1] == want_offsets and all(x == 2**64 - 1 for x in offsets[depth + 1:])
    assert depth == (n - 1).bit_length()


@pytest.mark.parametrize("n", [0, (1 << 26) + 1])
def test_library_layout_refuses(lib, n):
    status, depth, offsets, nodes = layout_of(lib, n)
    assert status == N.ZK_ERR_ARG and depth == -1 and nodes == 0 and offsets[0] == 2**64 - 1
