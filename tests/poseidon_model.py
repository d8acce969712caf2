"""Poseidon over Fr in Python integers: the test model of csrc/poseidon.hip and zksnake_amd.hash.

Its own Grain LFSR generates the round constants, so that the library's C++ generator and this one are two independent
implementations that have to agree by ==.  Nothing here imports the library.
"""

import functools

import tree_model as T

R = {
    "BN254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "BLS12_381": 52435875175126190479447740508185965837690552500527637822603658699938581184513,
}
R_F = 8
R_P = {3: 57, 4: 56, 5: 60}
WIDTHS = (3, 4, 5)


def grain_stream(r, t, rf, rp):
    """draw(): the next n-bit integer of the paper's Grain LFSR in self-shrinking mode, n = the bit length of r, big-endian"""
    n = r.bit_length()
    bits = []
    for value, width in ((1, 2), (0, 4), (n, 12), (t, 12), (rf, 10), (rp, 10), ((1 << 30) - 1, 30)):
        bits += [(value >> (width - 1 - i)) & 1 for i in range(width)]
    assert len(bits) == 80

    def step():
        new = bits[62] ^ bits[51] ^ bits[38] ^ bits[23] ^ bits[13] ^ bits[0]
        bits.pop(0)
        bits.append(new)
        return new

    for _ in range(160):
        step()

    def emitted():
        while True:
            first, second = step(), step()
            if first:
                return second

    def draw():
        c = 0
        for _ in range(n):
            c = (c << 1) | emitted()
        return c

    return draw


@functools.lru_cache(maxsize=None)
def generate(curve, t):
    """(round constants in round order, x_0..x_(t-1), y_0..y_(t-1)): (R_F + R_P) t draws, each redrawn while >= r, then 2 t
    draws reduced mod r -- all 2 t again while two of them are equal or some x_i + y_j is zero"""
    r, rf, rp = R[curve], R_F, R_P[t]
    draw = grain_stream(r, t, rf, rp)
    flat = []
    while len(flat) < (rf + rp) * t:
        c = draw()
        if c < r:
            flat.append(c)
    while True:
        xy = [draw() % r for _ in range(2 * t)]
        xs, ys = xy[:t], xy[t:]
        if len(set(xy)) == 2 * t and all((x + y) % r for x in xs for y in ys):
            return flat, xs, ys


@functools.lru_cache(maxsize=None)
def params(curve, t):
    """(r, R_F, R_P, round constants [round][i], matrix [i][j] = 1 / (x_i + y_j))"""
    r, rf, rp = R[curve], R_F, R_P[t]
    flat, xs, ys = generate(curve, t)
    rc = [flat[k * t:(k + 1) * t] for k in range(rf + rp)]
    mds = [[pow(x + y, -1, r) for y in ys] for x in xs]
    return r, rf, rp, rc, mds


def perm(curve, state):
    t = len(state)
    r, rf, rp, rc, mds = params(curve, t)
    s = [x % r for x in state]
    for k in range(rf + rp):
        s = [(x + c) % r for x, c in zip(s, rc[k])]
        if k < rf // 2 or k >= rf // 2 + rp:
            s = [pow(x, 5, r) for x in s]
        else:
            s[0] = pow(s[0], 5, r)
        s = [sum(m * x for m, x in zip(row, s)) % r for row in mds]
    return s


def hash(curve, inputs):  # noqa: A001 - the name the design gives it
    assert 2 <= len(inputs) <= 4
    return perm(curve, [0] + list(inputs))[0]


def sponge(curve, row):
    r = R[curve]
    assert len(row) >= 1
    s = [len(row) % r, 0, 0]
    for i in range(0, len(row), 2):
        s[1] = (s[1] + row[i]) % r
        if i + 1 < len(row):
            s[2] = (s[2] + row[i + 1]) % r
        s = perm(curve, s)
    return s[1]


def levels(curve, leaves):
    """every level of the tree over the leaf digests, level 0 first; a node without a right sibling is hashed with itself"""
    return T.levels(leaves, lambda left, right: hash(curve, [left, right]))


def path(lv, index):
    """the siblings of leaf `index`, leaf level first; the node itself where it has no sibling"""
    return T.path(lv, index)


def root(lv):
    return lv[-1][0]


def verify(curve, commitment, proof, index, digest):
    for sibling in proof:
        digest = hash(curve, [sibling, digest] if index & 1 else [digest, sibling])
        index >>= 1
    return digest == commitment
