"""CPU: the host side of csrc/merkle.hip under sanitizers, the new symbols' bindings, and the argument rules of
zksnake_amd.commitment.vector that need no GPU."""

import os
import re

import numpy as np
import pytest

from helpers import run_host_program
from zksnake_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("zk_blake2b_rows_dev", "zk_blake2b_items_dev", "zk_merkle_layout", "zk_merkle_build_dev", "zk_merkle_paths_dev")


def test_merkle_host_side_refuses_bad_arguments_under_sanitizers(tmp_path):
    """tests/native/merkle_args_check.cpp, built by the recipe in its header (helpers.run_host_program, as tests/test_pcs_host.py
    builds pcs_args_check): a host-only compile, an EMPTY offload bundle for the __hip_fatbin_<hash> symbol the object refers to, link,
    run.  The sanitizer runtimes are linked into the program; nothing is loaded into Python.  The program sees no device on any
    machine, so the calls that pass the checks fail in the launch with ZK_ERR_HIP, which is what it expects."""
    res = run_host_program("merkle_args_check", tmp_path)
    assert res.returncode == 0 and "merkle_args_check: all ok" in res.stdout, res.stdout + res.stderr


def test_symbols_are_bound(lib):
    for name in SYMBOLS:
        assert name in N.SIGNATURES and hasattr(lib, name)
    with open(os.path.join(ROOT, "include", "zkmi.h")) as f:
        header = f.read()
    assert f"#define ZK_MERKLE_DIGEST {N.MERKLE_DIGEST}\n" in header
    assert re.search(rf"#define ZK_MERKLE_MAX_LOG {N.MERKLE_MAX_LOG}\s", header)
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header)


def test_only_blake2b():
    from zksnake_amd.commitment.vector import Merkle, VectorCommitmentScheme
    for alg in ("sha256", "blake2s", "", None):
        with pytest.raises(ValueError):
            Merkle(alg)
    scheme = Merkle()
    assert isinstance(scheme, VectorCommitmentScheme) and scheme.alg == "blake2b" and Merkle("blake2b").setup() is None
    with pytest.raises(NotImplementedError):
        VectorCommitmentScheme().commit([b"x"])


def test_vectors_are_refused_before_any_device_call(monkeypatch):
    """an empty vector, an item that is not bytes-like and an array of the wrong kind never reach the GPU: ensure_gpu is made to
    fail the test if it is called"""
    from zksnake_amd.commitment.vector import Merkle

    def no_gpu(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(N, "ensure_gpu", no_gpu)
    scheme = Merkle()
    for empty in ([], (), iter(()), np.zeros((0, 32), dtype=np.uint8)):
        with pytest.raises(IndexError):
            scheme.commit(empty)
    with pytest.raises(IndexError):
        scheme.open([], 0)
    for bad in ([b"a", "b"], [b"a", 5], [None], ["text"]):
        with pytest.raises(TypeError):
            scheme.commit(bad)
    for bad in (np.zeros((4, 32), dtype=np.uint64), np.zeros(32, dtype=np.uint8), np.zeros((4, 64), dtype=np.uint8)[:, :32]):
        with pytest.raises(TypeError):
            scheme.commit(bad)


def test_index_rules_on_a_tree_of_known_size():
    """the index is checked against n before the tree's memory is asked for"""
    from zksnake_amd.commitment.vector import MerkleTree
    tree = MerkleTree(5, None)   # no device memory behind it
    assert (tree.n, tree.depth, tree.nodes, tree.root) == (5, 3, 11, None)
    for index in (5, -1, 1 << 40):
        with pytest.raises(IndexError):
            tree.open(index)
        with pytest.raises(IndexError):
            tree.open_many([0, index])
    with pytest.raises(TypeError):
        tree.open(1.5)
    with pytest.raises(RuntimeError):
        tree.open(4)        # in range: only now does the missing memory matter
    with pytest.raises(RuntimeError):
        tree.level(0)
    with pytest.raises(IndexError):
        tree.level(4)
    with pytest.raises(IndexError):
        MerkleTree(0, None)
    with pytest.raises(ValueError):
        MerkleTree((1 << 26) + 1, None)


def test_verify_is_the_reference_loop_on_the_host():
    """verify needs no GPU: a path of the hashlib model is accepted, and a changed element, sibling or index is not"""
    import merkle_model as M
    from zksnake_amd.commitment.vector import Merkle
    items = [M.golden_leaf(i) for i in range(5)]
    lv = M.levels(M.leaf_digests(items))
    scheme = Merkle()
    for i in range(5):
        proof = M.path(lv, i)
        assert scheme.verify(M.root(lv), proof, i, items[i])
        assert not scheme.verify(M.root(lv), proof, i, items[i] + b"\0")
        assert not scheme.verify(M.root(lv), [proof[0], proof[2], proof[1]], i, items[i])
    assert not scheme.verify(M.root(lv), M.path(lv, 1), 2, items[1])
