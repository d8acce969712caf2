"""Merkle vector commitment over BLAKE2b-512 (the reference's `zksnake.commitment.vector.Merkle`), hashed on the GPU.

Leaf digests, every level of the tree and the opening paths come from csrc/merkle.hip (one digest per lane); `verify` is log n
hashes and stays on the host with hashlib, the reference's own loop.  `Merkle.tree(vector)` keeps the tree in device memory, so
that many indices are opened from one build (`MerkleTree.open_many`: one launch, one download); `commit` and `open` are thin
wrappers over it.  What does not depend on the hash -- the layout, the resident tree, those wrappers -- is `_tree.py`.

A `vector` is one of
  * a sequence of bytes-like items of any lengths (the reference's shape): joined on the host, uploaded once;
  * a C-contiguous 2-D uint8 array, one leaf per row;
  * a `DevVec`: leaf i is the 32 bytes of element i as stored, `int.to_bytes(32, "little")`, hashed in place.

Differences from the reference:
  1. Where a node has no right sibling the reference's `commit` hashes it with itself, but its `open` leaves that level out of the
     proof, so its own `verify` rejects those proofs (index 2 of 3, index 4 of 5, ...).  Here `open` puts the node's own digest in
     that place: every proof has `depth` entries and the unchanged `verify` loop accepts it.  Roots are the reference's for every
     n, proofs are the reference's wherever the reference's proof verifies (every index when n is a power of two).
  2. Only alg="blake2b" exists; anything else is a ValueError at construction (there is no CPU fallback).
  3. An empty vector raises IndexError (as the reference's `tree[-1][0]` does) before any device call, and an index outside
     range(n) raises IndexError instead of being opened as some other leaf.
"""

import hashlib

import numpy as np

from ... import _native as N
from ...device import DeviceBuffer
from ...frvec import DevVec
from ._tree import MAX_LEAVES, DeviceTree, TreeScheme, _layout, _leaf_count  # noqa: F401 - MAX_LEAVES is part of this module

DIGEST = N.MERKLE_DIGEST


class MerkleTree(DeviceTree):
    """a tree of 64-byte nodes: `open_many` gives (k, depth, 64) uint8 and `level` (n_l, 64) uint8, the root and the entries of a
    proof are bytes"""

    KIND, DTYPE, WIDTH, PATHS = "Merkle", np.uint8, DIGEST, "zk_merkle_paths_dev"

    @staticmethod
    def _values(nodes):
        return [row.tobytes() for row in nodes]

    @classmethod
    def from_device_rows(cls, n, ptr, row_bytes):
        """the tree over n leaves that already lie in device memory, row_bytes bytes each from `ptr` on (hashed in place, not
        modified, and not needed once this returns)"""
        _leaf_count(n)
        if not 0 <= row_bytes < 1 << 32:
            raise ValueError("a leaf has fewer than 2^32 bytes")
        lib = N.ensure_gpu()
        tree = DeviceBuffer(_layout(n)[2] * DIGEST)
        try:
            N.check(lib.zk_blake2b_rows_dev(n, ptr, row_bytes, tree.ptr, None))
            N.check(lib.zk_merkle_build_dev(n, tree.ptr, None))
            return cls(n, tree)   # downloads the root
        except BaseException:
            tree.free()
            raise


def _host_leaves(vector):
    """(n, bytes to upload as a uint8 array, row length or None, offsets or None) of a host vector; no device call"""
    if isinstance(vector, np.ndarray):
        if vector.ndim != 2 or vector.dtype != np.uint8 or not vector.flags.c_contiguous:
            raise TypeError("an array of leaves is C-contiguous, 2-D and uint8: one leaf per row")
        return vector.shape[0], vector.reshape(-1), vector.shape[1], None
    items = vector if isinstance(vector, (list, tuple)) else list(vector)
    if not set(map(type, items)) <= {bytes, bytearray}:   # the usual case is settled without a Python-level loop over the items
        items = list(items)
        for i, item in enumerate(items):
            if isinstance(item, memoryview):
                items[i] = item.tobytes()    # len() of a memoryview counts elements, not bytes
            elif not isinstance(item, (bytes, bytearray)):
                raise TypeError(f"a leaf is bytes-like, not {type(item).__name__}")
    n = len(items)
    lens = np.fromiter(map(len, items), dtype=np.uint64, count=n)
    data = np.frombuffer(b"".join(items), dtype=np.uint8)
    if n == 0 or (lens == lens[0]).all():
        return n, data, int(lens[0]) if n else 0, None
    offsets = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    return n, data, None, offsets


class Merkle(TreeScheme):

    def __init__(self, alg="blake2b"):
        super().__init__()
        if alg != "blake2b":
            raise ValueError(f"only alg='blake2b' has a kernel (there is no CPU fallback), not {alg!r}")
        self.alg = alg

    def _hash(self, data):
        return hashlib.blake2b(data).digest()

    def tree(self, vector):
        """hash the leaves and build the tree on the GPU; the caller release()s it (or drops it)"""
        if isinstance(vector, DevVec):
            n, data, row_bytes, offsets = _leaf_count(vector.n), None, 32, None
        else:
            n, data, row_bytes, offsets = _host_leaves(vector)
            _leaf_count(n)
        if row_bytes is not None and row_bytes >> 32:
            raise ValueError("a leaf has fewer than 2^32 bytes")
        lib = N.ensure_gpu()
        nodes = _layout(n)[2]
        tree, owned = DeviceBuffer(nodes * DIGEST), []
        try:
            if data is None:
                src = vector.ptr()
            else:
                owned.append(DeviceBuffer.from_numpy(data) if data.nbytes else None)
                src = owned[0].ptr if owned[0] else None
            if offsets is None:
                N.check(lib.zk_blake2b_rows_dev(n, src, row_bytes, tree.ptr, None))
            else:
                owned.append(DeviceBuffer.from_numpy(offsets))
                N.check(lib.zk_blake2b_items_dev(n, src, data.nbytes, owned[1].ptr, tree.ptr, None))
            N.check(lib.zk_merkle_build_dev(n, tree.ptr, None))
            return MerkleTree(n, tree)   # downloads the root: the kernels above have run when the inputs are freed
        except BaseException:
            tree.free()
            raise
        finally:
            for buf in owned:
                if buf is not None:
                    buf.free()

    def verify(self, commitment, proof, index, element):
        digest = self._hash(element)
        for sibling in proof:
            digest = self._hash(sibling + digest if index & 1 else digest + sibling)
            index >>= 1
        return digest == commitment
