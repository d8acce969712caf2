"""Merkle vector commitment over BLAKE2b-512 (the reference's `zksnake.commitment.vector.Merkle`), hashed on the GPU.

Leaf digests, every level of the tree and the opening paths come from csrc/merkle.hip (one digest per lane); `verify` is log n
hashes and stays on the host with hashlib, the reference's own loop.  `Merkle.tree(vector)` keeps the tree in device memory, so
that many indices are opened from one build (`MerkleTree.open_many`: one launch, one download); `commit` and `open` are thin
wrappers over it.

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

import ctypes
import hashlib
import operator

import numpy as np

from ... import _native as N
from ...device import DeviceBuffer
from ...frvec import DevVec
from .base import VectorCommitmentScheme

DIGEST = N.MERKLE_DIGEST
MAX_LEAVES = 1 << N.MERKLE_MAX_LOG


def _layout(n):
    """(depth, first node of every level, nodes) of a tree over n leaves: host arithmetic of the library, no GPU"""
    depth, nodes = ctypes.c_int(0), ctypes.c_uint64(0)
    offsets = np.zeros(N.MERKLE_MAX_LOG + 1, dtype=np.uint64)
    N.check(N.load().zk_merkle_layout(n, ctypes.byref(depth), N.u64p(offsets), ctypes.byref(nodes)))
    return depth.value, [int(x) for x in offsets[:depth.value + 1]], nodes.value


def _leaf_count(n):
    if n == 0:
        raise IndexError("a Merkle tree needs at least one leaf")
    if n > MAX_LEAVES:
        raise ValueError(f"a Merkle tree has at most 2^{N.MERKLE_MAX_LOG} leaves")
    return n


class MerkleTree:
    """a tree over n leaves, resident in device memory (level 0 first, 64 bytes per node) until release()"""

    def __init__(self, n, buf):
        self.n = _leaf_count(n)
        self.depth, self._offsets, self.nodes = _layout(n)
        self._buf = buf   # the tree's one owner
        self.root = None if buf is None else buf.download((DIGEST,), np.uint8, (self.nodes - 1) * DIGEST).tobytes()

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
        """(k, depth, 64) uint8: row q is the proof of indices[q], leaf level first"""
        idx = self._indices(indices)
        tree, k = self._device(), idx.shape[0]
        if k == 0 or self.depth == 0:
            return np.zeros((k, self.depth, DIGEST), dtype=np.uint8)
        d_idx = DeviceBuffer.from_numpy(idx)
        d_paths = DeviceBuffer(k * self.depth * DIGEST)
        try:
            N.check(N.load().zk_merkle_paths_dev(self.n, tree.ptr, k, d_idx.ptr, d_paths.ptr, None))
            return d_paths.download((k, self.depth, DIGEST), np.uint8)
        finally:
            d_idx.free()
            d_paths.free()

    def open(self, index):
        return [row.tobytes() for row in self.open_many([index])[0]]

    def level(self, l):
        """the nodes of level l (0: the leaf digests, depth: the root) as (n_l, 64) uint8"""
        if not 0 <= l <= self.depth:
            raise IndexError(f"level {l} of a tree of depth {self.depth}")
        end = self._offsets[l + 1] if l < self.depth else self.nodes
        return self._device().download((end - self._offsets[l], DIGEST), np.uint8, self._offsets[l] * DIGEST)

    def release(self):
        if self._buf is not None:
            self._buf.free()
            self._buf = None


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


class Merkle(VectorCommitmentScheme):

    def __init__(self, alg="blake2b"):
        super().__init__()
        if alg != "blake2b":
            raise ValueError(f"only alg='blake2b' has a kernel (there is no CPU fallback), not {alg!r}")
        self.alg = alg

    def setup(self):
        pass

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

    def commit(self, vector):
        tree = self.tree(vector)
        try:
            return tree.root
        finally:
            tree.release()

    def open(self, vector, index):
        tree = self.tree(vector)
        try:
            return tree.open(index)
        finally:
            tree.release()

    def verify(self, commitment, proof, index, element):
        digest = self._hash(element)
        for sibling in proof:
            digest = self._hash(sibling + digest if index & 1 else digest + sibling)
            index >>= 1
        return digest == commitment
