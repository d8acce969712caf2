"""CPU: the host side of csrc/poseidon.hip -- its parameter generator against the model's, its argument rules under sanitizers,
the new symbols' bindings -- and what zksnake_amd.hash / PoseidonMerkle do without a GPU."""

import ctypes
import os
import random
import re

import numpy as np
import pytest

import poseidon_model as M
from helpers import run_host_program
from zksnake_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("zk_poseidon_params", "zk_poseidon_perm_dev", "zk_poseidon_hash_dev", "zk_poseidon_sponge_rows_dev",
           "zk_poseidon_merkle_build_dev", "zk_poseidon_merkle_paths_dev")
CURVES = ("BN254", "BLS12_381")


@pytest.mark.parametrize("t", M.WIDTHS)
@pytest.mark.parametrize("curve", CURVES)
def test_library_parameters_equal_the_models(lib, curve, t):
    """two independent Grain generators, C++ and Python, agree by =="""
    r, rf, rp, rc, mds = M.params(curve, t)
    got_rf, got_rp = ctypes.c_int(-1), ctypes.c_int(-1)
    out = np.full(((rf + rp) * t + t * t + 1, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    N.check(lib.zk_poseidon_params(N.curve_id(curve), t, ctypes.byref(got_rf), ctypes.byref(got_rp), N.u64p(out)))
    assert (got_rf.value, got_rp.value) == (rf, rp)
    assert N.limbs_to_ints(out[:-1]) == [c for row in rc for c in row] + [m for row in mds for m in row]
    assert (out[-1] == 0xA5A5A5A5A5A5A5A5).all(), "written past the last matrix entry"
    N.check(lib.zk_poseidon_params(N.curve_id(curve), t, None, None, None))
    for bad_curve, bad_t in ((2, t), (-1, t), (N.curve_id(curve), 2), (N.curve_id(curve), 6)):
        assert lib.zk_poseidon_params(bad_curve, bad_t, None, None, None) == N.ZK_ERR_ARG


def test_symbols_are_bound(lib):
    for name in SYMBOLS:
        assert name in N.SIGNATURES and hasattr(lib, name)
    with open(os.path.join(ROOT, "include", "zkmi.h")) as f:
        header = f.read()
    assert f"#define ZK_POSEIDON_MAX_LOG {N.POSEIDON_MAX_LOG}\n" in header
    assert "#define ZK_POSEIDON_MAX_ROW (1u << 20)\n" in header and N.POSEIDON_MAX_ROW == 1 << 20
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header)


def test_poseidon_host_side_refuses_bad_arguments_under_sanitizers(tmp_path):
    """tests/native/poseidon_args_check.cpp, built by helpers.run_host_program: a host-only compile, an empty offload bundle, link,
    run.  The sanitizer runtimes are linked into the program; nothing is loaded into Python.  The program sees no device on any
    machine, so the calls that pass the checks end in ZK_ERR_HIP, which is what it expects; it also runs the permutation the
    kernels run, on the host, against the two published values."""
    res = run_host_program("poseidon_args_check", tmp_path)
    assert res.returncode == 0 and "poseidon_args_check: all ok" in res.stdout, res.stdout + res.stderr


@pytest.mark.parametrize("curve", CURVES)
def test_host_poseidon_equals_the_model(curve):
    from zksnake_amd.hash import Poseidon
    h, rng = Poseidon(curve), random.Random(curve)
    r = M.R[curve]
    assert h.p == r
    for t in M.WIDTHS:
        rf, rp, rc, mds = h.params(t)
        assert (r, rf, rp, rc, mds) == M.params(curve, t)
        for state in ([0] * t, [r - 1] * t, [rng.randrange(r) for _ in range(t)]):
            assert h.permute(state) == M.perm(curve, state)
            assert h.hash(state[1:]) == M.hash(curve, state[1:])
    for length in (1, 2, 3, 4, 5, 8, 9):
        row = [rng.randrange(r) for _ in range(length)]
        assert h.sponge(row) == M.sponge(curve, row)
    assert h.sponge([r - 1]) == M.sponge(curve, [r - 1])
    if curve == "BN254":
        assert h.hash([1, 2, 3]) == 0x0E7732D89E6939C0FF03D5E58DAB6302F3230E269DC5B968F725DF34AB36D732


def test_verify_on_the_host():
    """verify needs no GPU: the model's paths for n = 5 are accepted at every index, and a changed leaf, sibling or index is not"""
    from zksnake_amd.commitment.vector import PoseidonMerkle, VectorCommitmentScheme
    for curve in CURVES:
        scheme = PoseidonMerkle(curve)
        assert isinstance(scheme, VectorCommitmentScheme) and scheme.setup() is None and scheme.order == M.R[curve]
        rows = [[i, 10 + i, 20 + i] for i in range(5)]
        lv = M.levels(curve, [M.sponge(curve, row) for row in rows])
        for i in range(5):
            proof = M.path(lv, i)
            assert scheme.verify(M.root(lv), proof, i, rows[i])
            assert not scheme.verify(M.root(lv), proof, i, rows[i][:2] + [rows[i][2] + 1])
            assert not scheme.verify(M.root(lv), proof, i, rows[i] + [0])
            assert not scheme.verify(M.root(lv), [proof[0], proof[2], proof[1]], i, rows[i])
            assert not scheme.verify(M.root(lv), [proof[0], (proof[1] + 1) % scheme.order, proof[2]], i, rows[i])
            assert not scheme.verify(M.root(lv), [proof[0], proof[1], proof[2] + scheme.order], i, rows[i])   # not an alias mod r
        assert not scheme.verify(M.root(lv), M.path(lv, 1), 2, rows[1])
        # a leaf of one element is that element or a row of it
        lv1 = M.levels(curve, [M.sponge(curve, [x]) for x in (7, 8, 9)])
        assert scheme.verify(M.root(lv1), M.path(lv1, 2), 2, 9) and scheme.verify(M.root(lv1), M.path(lv1, 2), 2, [9])
        assert scheme.verify(M.sponge(curve, [7]), [], 0, 7)   # one leaf is its own root


def no_gpu(*a, **k):
    raise AssertionError("a device call was made")


def test_bad_inputs_are_refused_before_any_device_call(monkeypatch):
    """range, length and shape errors of the GPU calls never reach the GPU: ensure_gpu is made to fail the test if it is called"""
    from zksnake_amd.hash import Poseidon
    monkeypatch.setattr(N, "ensure_gpu", no_gpu)
    h = Poseidon()
    r = h.p
    for call in (h.permute_many, h.hash_many, h.sponge_many):
        for bad in ([[1, 2, r]], [[1, 2, -1]], [[1, 2, 3], [1, 2, 1 << 256]]):
            with pytest.raises(ValueError):
                call(bad)
        with pytest.raises(ValueError):
            call([[1, 2, 3], [1, 2]])                     # rows of different lengths
        with pytest.raises(ValueError):
            call([])
        with pytest.raises(ValueError):
            call(np.zeros((2, 3), dtype=np.uint64))       # not (n, k, 4)
        with pytest.raises(ValueError):
            call(np.zeros((0, 3, 4), dtype=np.uint64))
        over = N.ints_to_limbs([1, 2, r], 4).reshape(1, 3, 4)
        with pytest.raises(ValueError):
            call(over)
    over[0, 2] = N.ints_to_limbs([r - 1], 4)[0]
    assert h.rows_in(over, None, range(2, 5), "x")[:2] == (1, 3)   # r - 1 is in range
    for bad in ([[1]], [[1, 2, 3, 4, 5]], np.zeros((1, 5, 4), dtype=np.uint64)):
        with pytest.raises(ValueError):
            h.hash_many(bad)
    for bad in ([[1, 2]], [[1] * 6]):
        with pytest.raises(ValueError):
            h.permute_many(bad)
    with pytest.raises(ValueError):
        h.hash_many([[1, 2, 3]], 2)
    # the host calls have the same range rule
    for bad in ([1, r], [0, -1]):
        with pytest.raises(ValueError):
            h.hash(bad)
        with pytest.raises(ValueError):
            h.sponge(bad)
        with pytest.raises(ValueError):
            h.permute([0] + bad)
    for bad in ([1], [1, 2, 3, 4, 5]):
        with pytest.raises(ValueError):
            h.hash(bad)
    with pytest.raises(ValueError):
        h.sponge([])
    with pytest.raises(ValueError):
        h.permute([1, 2])
    with pytest.raises(ValueError):
        h.params(6)
    with pytest.raises(KeyError):
        Poseidon("secp256k1")


def test_vectors_are_refused_before_any_device_call(monkeypatch):
    from zksnake_amd.commitment.vector import Merkle, PoseidonMerkle
    monkeypatch.setattr(N, "ensure_gpu", no_gpu)
    scheme = PoseidonMerkle()
    r = scheme.order
    for empty in ([], (), iter(()), np.zeros((0, 2, 4), dtype=np.uint64)):
        with pytest.raises(IndexError):
            scheme.commit(empty)
    with pytest.raises(IndexError):
        scheme.open([], 0)
    for index in (3, -1, 1 << 40):
        with pytest.raises(IndexError):
            scheme.open([1, 2, 3], index)
    for bad in ([1, r], [[1, 2], [3, r]], [-1], [[1, 2], [3]], [1, [2]], np.zeros((3, 4), dtype=np.uint64),
                N.ints_to_limbs([r], 4).reshape(1, 1, 4)):
        with pytest.raises(ValueError):
            scheme.commit(bad)
    with pytest.raises(ValueError):
        Merkle("poseidon")      # the BLAKE2b scheme is not touched


def test_index_rules_on_a_tree_of_known_size():
    """the index is checked against n before the tree's memory is asked for"""
    from zksnake_amd.commitment.vector import PoseidonMerkleTree
    tree = PoseidonMerkleTree(5, None)   # no device memory behind it
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
        PoseidonMerkleTree(0, None)
    with pytest.raises(ValueError):
        PoseidonMerkleTree((1 << 26) + 1, None)
