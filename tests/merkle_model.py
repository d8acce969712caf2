"""hashlib model of csrc/merkle.hip and zksnake_amd.commitment.vector, written from the definition: BLAKE2b-512 leaf digests,
every level of the tree with a lone node hashed with itself, the layout of the concatenated levels, the root, an opening path
with the node's own digest where it has no sibling, and the reference's verify loop.  hashlib is an independent BLAKE2b, so
everything that is compared with this model is compared with == on bytes."""

import hashlib

import tree_model as T

DIGEST = 64
MAX_LOG = 26


def H(data):
    return hashlib.blake2b(bytes(data)).digest()


def leaf_digests(items):
    return [H(x) for x in items]


def levels(leaves):
    """[level 0, level 1, .., [root]] from the leaf digests"""
    return T.levels(leaves, lambda left, right: H(left + right))


def layout(n):
    """(depth, first node of every level, nodes)"""
    assert 1 <= n <= 1 << MAX_LOG
    offsets, nodes, width = [], 0, n
    while True:
        offsets.append(nodes)
        nodes += width
        if width == 1:
            return len(offsets) - 1, offsets, nodes
        width = (width + 1) // 2


def tree_bytes(lv):
    return b"".join(b"".join(level) for level in lv)


def root(lv):
    return lv[-1][0]


def path(lv, index):
    """depth entries: the sibling at every level below the root, the node itself where there is none"""
    return T.path(lv, index)


def verify(commitment, proof, index, element):
    cur = H(element)
    for sib in proof:
        cur = H(cur + sib) if index % 2 == 0 else H(sib + cur)
        index //= 2
    return cur == commitment


def golden_leaf(i):
    """the leaves of tests/golden/merkle_vectors.json: byte i, i mod 5 times"""
    return bytes([i & 0xFF]) * (i % 5)
