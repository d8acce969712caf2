"""What the Merkle trees of this package share whatever their hash: the layout of the levels, the tree
resident in device memory with its opening paths, and the commit / open wrappers of a scheme that builds one.  The host side of
csrc/merkle_tree.hip.h; `merkle.py` (BLAKE2b, 64-byte nodes) and `poseidon.py` (32-byte nodes) bring the hash."""

import ctypes
import operator

import numpy as np

from ... import _native as N
from ...device import DeviceBuffer
from .base import VectorCommitmentScheme

assert N.MERKLE_MAX_LOG == N.POSEIDON_MAX_LOG   # one leaf limit, as in the library
MAX_LEAVES = 1 << N.MERKLE_MAX_LOG


def _layout(n):
    """(depth, first node of every level, nodes) of a tree over n leaves: host arithmetic of the library, no GPU"""
    depth, nodes = ctypes.c_int(0), ctypes.c_uint64(0)
    offsets = np.zeros(N.MERKLE_MAX_LOG + 1, dtype=np.uint64)
    N.check(N.load().zk_merkle_layout(n, ctypes.byref(depth), N.u64p(offsets), ctypes.byref(nodes)))
    return depth.value, [int(x) for x in offsets[:depth.value + 1]], nodes.value


def _leaf_count(n, kind="Merkle"):
    if n == 0:
        raise IndexError("a Merkle tree needs at least one leaf")
    if n > MAX_LEAVES:
        raise ValueError(f"a {kind} tree has at most 2^{N.MERKLE_MAX_LOG} leaves")
    return n


class DeviceTree:
    """a tree over n leaves, resident in device memory (level 0 first) until release().  A subclass names its nodes: `KIND` for
    messages, a node as `WIDTH` numbers of `DTYPE` in the arrays handed out, the library's gather `PATHS`, and `_values`, which
    turns an (m, WIDTH) array of nodes into the list of m commitments or proof entries."""

    KIND = DTYPE = WIDTH = PATHS = None

    def __init__(self, n, buf):
        self.n = _leaf_count(n, self.KIND)
        self.depth, self._offsets, self.nodes = _layout(n)
        self._node = self.WIDTH * np.dtype(self.DTYPE).itemsize   # bytes
        self._buf = buf   # the tree's one owner
        self.root = None if buf is None else self._values(self._download(self.nodes - 1, 1))[0]

    def _download(self, first, count):
        return self._device().download((count, self.WIDTH), self.DTYPE, first * self._node)

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
        """(k, depth, WIDTH) of DTYPE: row q is the proof of indices[q], leaf level first"""
        idx = self._indices(indices)
        tree, k = self._device(), idx.shape[0]
        if k == 0 or self.depth == 0:
            return np.zeros((k, self.depth, self.WIDTH), dtype=self.DTYPE)
        d_idx = DeviceBuffer.from_numpy(idx)
        d_paths = DeviceBuffer(k * self.depth * self._node)
        try:
            N.check(getattr(N.load(), self.PATHS)(self.n, tree.ptr, k, d_idx.ptr, d_paths.ptr, None))
            return d_paths.download((k, self.depth, self.WIDTH), self.DTYPE)
        finally:
            d_idx.free()
            d_paths.free()

    def open(self, index):
        return self._values(self.open_many([index])[0])

    def level(self, l):
        """the nodes of level l (0: the leaf digests, depth: the root) as (n_l, WIDTH) of DTYPE"""
        if not 0 <= l <= self.depth:
            raise IndexError(f"level {l} of a tree of depth {self.depth}")
        end = self._offsets[l + 1] if l < self.depth else self.nodes
        return self._download(self._offsets[l], end - self._offsets[l])

    def release(self):
        if self._buf is not None:
            self._buf.free()
            self._buf = None


class TreeScheme(VectorCommitmentScheme):
    """commit and open of a scheme whose tree(vector) builds a DeviceTree: build, use, release"""

    def setup(self):
        pass

    @staticmethod
    def _use(tree, use):
        try:
            return use(tree)
        finally:
            tree.release()

    def commit(self, vector):
        return self._use(self.tree(vector), lambda tree: tree.root)

    def open(self, vector, index):
        return self._use(self.tree(vector), lambda tree: tree.open(index))
