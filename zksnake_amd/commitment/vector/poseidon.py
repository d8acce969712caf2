"""Merkle vector commitment over Poseidon: a tree a circuit can open, built on the GPU.

A leaf is a row of L >= 1 field elements and its digest is `Poseidon.sponge(row)` (the length sits in the capacity element, so a
leaf digest is never a node); a node is `Poseidon.hash(left, right)`, circomlib's Poseidon(2).  The shape is `Merkle`'s: a node
without a right sibling is hashed with itself, depth = ceil(log2 n), one leaf is its own root, and a proof has `depth` entries,
the node itself where it has no sibling.  Nodes are canonical Fr elements, 32 bytes.  Leaf digests, every level and the opening
paths come from csrc/poseidon.hip (one permutation per lane); `verify` is 1 + ceil(L / 2) + depth permutations in Python integers
and needs no GPU.

A `vector` is one of
  * a `DevVec`: leaf i is the one-element row [element i];
  * a sequence of ints: the same;
  * a sequence of equal-length rows of ints;
  * an (n, L, 4) uint64 limb array, one leaf per row.
An integer outside [0, r) and rows of different lengths are a ValueError, an empty vector and an index outside range(n) an
IndexError, all before any device call.  The commitment is the root as an int, a proof a list of `depth` ints.
"""

import operator

import numpy as np

from ... import _native as N
from ...device import DeviceBuffer
from ...frvec import DevVec
from ...hash import Poseidon
from .base import VectorCommitmentScheme
from .merkle import _layout

NODE = 32
MAX_LEAVES = 1 << N.POSEIDON_MAX_LOG


def _leaf_count(n):
    if n == 0:
        raise IndexError("a Merkle tree needs at least one leaf")
    if n > MAX_LEAVES:
        raise ValueError(f"a Poseidon Merkle tree has at most 2^{N.POSEIDON_MAX_LOG} leaves")
    return n


class PoseidonMerkleTree:
    """a tree over n leaves, resident in device memory (level 0 first, 32 bytes per node) until release()"""

    def __init__(self, n, buf):
        self.n = _leaf_count(n)
        self.depth, self._offsets, self.nodes = _layout(n)
        self._buf = buf   # the tree's one owner
        self.root = None if buf is None else N.limbs_to_ints(buf.download((1, 4), np.uint64, (self.nodes - 1) * NODE))[0]

    def _device(self):
        if self._buf is None or self._buf.ptr is None:
            raise RuntimeError("the tree has been released")
        return self._buf

    def _indices(self, indices):
        idx = [operator.index(i) for i in indices]
        for i in idx:
            if not 0 <= i < self.n:
                raise IndexError(f"index {i} is outside a vector of {self.n} elements")
        return np.array(idx, dtype=np.uint64)

    def open_many(self, indices):
        """(k, depth, 4) uint64: row q is the proof of indices[q] as limbs, leaf level first"""
        idx = self._indices(indices)
        tree, k = self._device(), idx.shape[0]
        if k == 0 or self.depth == 0:
            return np.zeros((k, self.depth, 4), dtype=np.uint64)
        d_idx = DeviceBuffer.from_numpy(idx)
        d_paths = DeviceBuffer(k * self.depth * NODE)
        try:
            N.check(N.load().zk_poseidon_merkle_paths_dev(self.n, tree.ptr, k, d_idx.ptr, d_paths.ptr, None))
            return d_paths.download((k, self.depth, 4), np.uint64)
        finally:
            d_idx.free()
            d_paths.free()

    def open(self, index):
        path = self.open_many([index])[0]
        return N.limbs_to_ints(path) if len(path) else []

    def level(self, l):
        """the nodes of level l (0: the leaf digests, depth: the root) as (n_l, 4) uint64 limbs"""
        if not 0 <= l <= self.depth:
            raise IndexError(f"level {l} of a tree of depth {self.depth}")
        end = self._offsets[l + 1] if l < self.depth else self.nodes
        return self._device().download((end - self._offsets[l], 4), np.uint64, self._offsets[l] * NODE)

    def release(self):
        if self._buf is not None:
            self._buf.free()
            self._buf = None


class PoseidonMerkle(VectorCommitmentScheme):

    def __init__(self, curve="BN254"):
        super().__init__()
        self.hasher = Poseidon(curve)
        self.curve = curve
        self.order = self.hasher.p

    def setup(self):
        pass

    def _leaves(self, vector):
        """(n, L, source) of a vector, checked on the host; no device call"""
        if isinstance(vector, DevVec):
            _leaf_count(vector.n)
            return self.hasher.rows_in(vector, 1, range(1, 2), "PoseidonMerkle")
        if isinstance(vector, np.ndarray):
            if vector.ndim == 3:
                _leaf_count(vector.shape[0])
            return self.hasher.rows_in(vector, None, range(1, N.POSEIDON_MAX_ROW + 1), "PoseidonMerkle")
        items = vector if isinstance(vector, (list, tuple)) else list(vector)
        _leaf_count(len(items))
        flat = [isinstance(item, (int, np.integer)) for item in items]
        if all(flat):
            items = [[item] for item in items]
        elif any(flat):
            raise ValueError("PoseidonMerkle: a vector holds ints or rows of ints, not both")
        return self.hasher.rows_in(items, None, range(1, N.POSEIDON_MAX_ROW + 1), "PoseidonMerkle")

    def tree(self, vector):
        """hash the leaves and build the tree on the GPU; the caller release()s it (or drops it)"""
        return self._build(*self._leaves(vector))

    def _build(self, n, row_elems, src):
        lib = N.ensure_gpu()
        tree = DeviceBuffer(_layout(n)[2] * NODE)
        try:
            rows = self.hasher.on_device(src)
            N.check(lib.zk_poseidon_sponge_rows_dev(self.hasher.cid, n, rows.ptr(), row_elems, tree.ptr, None))
            N.check(lib.zk_poseidon_merkle_build_dev(self.hasher.cid, n, tree.ptr, None))
            return PoseidonMerkleTree(n, tree)   # downloads the root: the kernels above have run when the rows go back
        except BaseException:
            tree.free()
            raise

    def commit(self, vector):
        tree = self.tree(vector)
        try:
            return tree.root
        finally:
            tree.release()

    def open(self, vector, index):
        leaves = self._leaves(vector)
        index = operator.index(index)
        if not 0 <= index < leaves[0]:
            raise IndexError(f"index {index} is outside a vector of {leaves[0]} elements")
        tree = self._build(*leaves)
        try:
            return tree.open(index)
        finally:
            tree.release()

    def verify(self, commitment, proof, index, element):
        """on the host: element is the leaf, an int or a row of ints"""
        row = [element] if isinstance(element, (int, np.integer)) else list(element)
        try:
            digest = self.hasher.sponge(row)
            for sibling in proof:
                digest = self.hasher.hash([sibling, digest] if index & 1 else [digest, sibling])
                index >>= 1
        except ValueError:   # an element or a sibling outside [0, r) opens nothing
            return False
        return digest == commitment
