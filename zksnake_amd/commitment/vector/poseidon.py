"""Merkle vector commitment over Poseidon: a tree a circuit can open, built on the GPU.

A leaf is a row of L >= 1 field elements and its digest is `Poseidon.sponge(row)` (the length sits in the capacity element, so a
leaf digest is never a node); a node is `Poseidon.hash(left, right)`, circomlib's Poseidon(2).  The shape is `Merkle`'s: a node
without a right sibling is hashed with itself, depth = ceil(log2 n), one leaf is its own root, and a proof has `depth` entries,
the node itself where it has no sibling (`_tree.py` holds all of that).  Nodes are canonical Fr elements, 32 bytes.  Leaf digests, every level and the opening
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
from ._tree import MAX_LEAVES, DeviceTree, TreeScheme, _layout, _leaf_count  # noqa: F401 - MAX_LEAVES is part of this module

NODE = 32


class PoseidonMerkleTree(DeviceTree):
    """a tree of 32-byte nodes: `open_many` gives (k, depth, 4) uint64 limbs and `level` (n_l, 4) limbs, the root and the entries
    of a proof are ints"""

    KIND, DTYPE, WIDTH, PATHS = "Poseidon Merkle", np.uint64, 4, "zk_poseidon_merkle_paths_dev"

    @staticmethod
    def _values(nodes):
        return N.limbs_to_ints(nodes) if len(nodes) else []


class PoseidonMerkle(TreeScheme):

    def __init__(self, curve="BN254"):
        super().__init__()
        self.hasher = Poseidon(curve)
        self.curve = curve
        self.order = self.hasher.p

    def _leaves(self, vector):
        """(n, L, source) of a vector, checked on the host; no device call"""
        if isinstance(vector, DevVec):
            _leaf_count(vector.n, PoseidonMerkleTree.KIND)
            return self.hasher.rows_in(vector, 1, range(1, 2), "PoseidonMerkle")
        if isinstance(vector, np.ndarray):
            if vector.ndim == 3:
                _leaf_count(vector.shape[0], PoseidonMerkleTree.KIND)
            return self.hasher.rows_in(vector, None, range(1, N.POSEIDON_MAX_ROW + 1), "PoseidonMerkle")
        items = vector if isinstance(vector, (list, tuple)) else list(vector)
        _leaf_count(len(items), PoseidonMerkleTree.KIND)
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

    def open(self, vector, index):
        leaves = self._leaves(vector)
        index = operator.index(index)
        if not 0 <= index < leaves[0]:
            raise IndexError(f"index {index} is outside a vector of {leaves[0]} elements")
        return self._use(self._build(*leaves), lambda tree: tree.open(index))

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
