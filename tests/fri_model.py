"""Integer model of the FRI polynomial commitment (zksnake_amd/commitment/polynomial/fri.py, csrc/fri.hip), written from the
protocol's definition: hashlib for BLAKE2b, a recursive transform, Python ints, and `oracle.pyref` only for r, the field's
multiplicative generator and the roots of unity.  Nothing of the package is used.

  n = 2^k coefficients at most, blowup B = 2^b, N = n B, `final` = 2^f coefficients sent in the clear, L = k - f folds.
  Layer l lives on the coset s_l <w_l> of M_l = N >> l points, s_0 = fr_gen, w_0 = root_of_unity(N), both squared per layer.
  A layer f of M = 2h values is kept in PAIR ORDER, g[2j] = f[j], g[2j+1] = f[j+h] (f at x_j and at -x_j); leaf j of its tree
  is le32(f[j]) || le32(f[j+h]).  fold: f'[j] = (f[j] + f[j+h]) / 2 + alpha (f[j] - f[j+h]) / (2 s_l w_l^j), j < h.

A proof is a dict {"roots": [64 bytes per committed layer 1 .. L-1], "final": [2^f ints], "queries": [(per polynomial
[(leaf, path)], per committed layer [(leaf, path)])]}; `proof_bytes` is its serialisation (layout in its docstring)."""

import hashlib

from oracle import pyref

TAG = b"zksnake-amd-fri-v1"
MAGIC = b"FRI1"
CURVES = {"BN254": (0, pyref.BN254), "BLS12_381": (1, pyref.BLS12_381)}


# ---- hashing, trees, transcript ---------------------------------------------------------------------------------------------
def H(data):
    return hashlib.blake2b(bytes(data)).digest()


def tree_levels(leaves):
    """[leaf digests, .., [root]]; the leaf counts of this protocol are powers of two, so no node lacks a sibling"""
    out = [[H(x) for x in leaves]]
    while len(out[-1]) > 1:
        cur = out[-1]
        out.append([H(cur[i] + cur[i + 1]) for i in range(0, len(cur), 2)])
    return out


def tree_path(levels, index):
    out = []
    for level in levels[:-1]:
        out.append(level[index ^ 1])
        index >>= 1
    return out


def path_ok(root, path, index, leaf):
    """the reference's verify loop"""
    cur = H(leaf)
    for sib in path:
        cur = H(sib + cur) if index & 1 else H(cur + sib)
        index >>= 1
    return cur == root


class Transcript:
    """FiatShamirTranscript(label=b"", alg="blake2b") restated: a running hash, a challenge is the digest and seeds the next hasher"""

    def __init__(self, r):
        self.r = r
        self.h = hashlib.blake2b(b"")

    def append(self, data):
        self.h.update(data)

    def scalar_in(self, x):
        self.h.update(int(x).to_bytes(32, "big"))

    def challenge(self):
        out = self.h.digest()
        self.h = hashlib.blake2b(out)
        return int.from_bytes(out, "big") % self.r


# ---- parameters -------------------------------------------------------------------------------------------------------------
class Params:
    def __init__(self, curve, k, b, f, queries):
        assert b >= 1 and k + b <= 26 and 0 <= f < k and 1 <= queries <= 1 << 16
        self.cid, cv = CURVES[curve]
        self.curve, self.r, self.g = curve, cv.r, cv.fr_gen
        self.k, self.b, self.f, self.queries = k, b, f, queries
        self.n, self.N, self.L = 1 << k, 1 << (k + b), k - f
        self.w0 = cv.root_of_unity(self.N)

    def header(self):
        return TAG + bytes([self.cid, self.k, self.b, self.f]) + self.queries.to_bytes(4, "big")

    def shift(self, l):
        return pow(self.g, 1 << l, self.r)

    def omega(self, l):
        return pow(self.w0, 1 << l, self.r)

    def size(self, l):
        return self.N >> l


# ---- polynomials ------------------------------------------------------------------------------------------------------------
def poly_eval(c, x, r):
    acc = 0
    for a in reversed(c):
        acc = (acc * x + a) % r
    return acc


def div_linear(c, z, r):
    """(quotient, remainder) of c by X - z: Horner's rule"""
    q, acc = [0] * max(len(c) - 1, 0), 0
    for i in range(len(c) - 1, -1, -1):
        acc = (acc * z + c[i]) % r
        if i:
            q[i - 1] = acc
    return q, acc


def fft(a, w, r):
    """[sum_i a_i w^(i j)] for j < len(a), recursively"""
    m = len(a)
    if m == 1:
        return list(a)
    ev, od = fft(a[0::2], w * w % r, r), fft(a[1::2], w * w % r, r)
    out, t = [0] * m, 1
    for j in range(m // 2):
        out[j], out[j + m // 2] = (ev[j] + t * od[j]) % r, (ev[j] - t * od[j]) % r
        t = t * w % r
    return out


def pair_order(f):
    h = len(f) // 2
    if h == 0:
        return list(f)
    out = [0] * len(f)
    out[0::2], out[1::2] = f[:h], f[h:]
    return out


def natural_order(g):
    return list(g) if len(g) < 2 else list(g[0::2]) + list(g[1::2])


def lde(P, coeffs, size=None):
    """p on the coset of layer 0 in pair order: coefficients c_i g^i, the transform of size N, the permutation"""
    size = size or P.N
    assert len(coeffs) <= size
    scaled, t = [0] * size, 1
    for i, c in enumerate(coeffs):
        scaled[i] = c % P.r * t % P.r
        t = t * P.g % P.r
    return pair_order(fft(scaled, pow(P.w0, P.N // size, P.r), P.r))


def fold(P, l, layer, alpha):
    """pair order of layer l -> pair order of layer l + 1"""
    return fold_on(P.r, P.shift(l), P.omega(l), layer, alpha)


def fold_on(r, s, w, layer, alpha):
    """the fold of a pair-order layer on the coset s <w>, w of order len(layer)"""
    h = len(layer) // 2
    half = pow(2, -1, r)
    out, x = [0] * h, s
    for j in range(h):
        a, b = layer[2 * j], layer[2 * j + 1]
        out[j] = ((a + b) * half + alpha * (a - b) % r * pow(2 * x, -1, r)) % r
        x = x * w % r
    return pair_order(out)


def leaves_of(layer):
    """64 bytes per pair; a layer in pair order is its leaves one after the other"""
    return [layer[2 * j].to_bytes(32, "little") + layer[2 * j + 1].to_bytes(32, "little") for j in range(len(layer) // 2)]


def commit(P, coeffs):
    """(root, tree levels, leaves, pair-order evaluations)"""
    if len(coeffs) > P.n:
        raise ValueError("too many coefficients")
    ev = lde(P, coeffs)
    leaves = leaves_of(ev)
    levels = tree_levels(leaves)
    return levels[-1][0], levels, leaves, ev


def in_domain(P, z):
    return pow(z, P.N, P.r) == pow(P.g, P.N, P.r)


# ---- prover -----------------------------------------------------------------------------------------------------------------
def prove(P, polys, pairs, transcript=None, cheat_value=None):
    """polys: lists of coefficients; pairs: [(index of a polynomial, z)] in opening order.  Returns (proof, values).
    cheat_value = {position in pairs: v'}: those values are claimed instead of the true ones and layer 0 is built in evaluation
    space, sum_k lambda^k (p_i(x) - v_k) / (x - z_k) at every point of the coset (no polynomial of low degree agrees with it);
    the last layer's interpolant is then cut to `final` coefficients without the degree check."""
    r = P.r
    t = transcript or Transcript(r)
    trees = [commit(P, p) for p in polys]
    t.append(P.header())
    for tree in trees:
        t.append(tree[0])
    values = []
    for pos, (i, z) in enumerate(pairs):
        if in_domain(P, z):
            raise ValueError("an opening point lies in the evaluation domain")
        v = poly_eval(polys[i], z, r)
        if cheat_value and pos in cheat_value:
            v = cheat_value[pos] % r
        values.append(v)
        t.scalar_in(z % r)
        t.scalar_in(v)
    lam = t.challenge()
    if cheat_value:
        layer = []
        for idx in range(P.N // 2):
            x = P.g * pow(P.w0, idx, r) % r
            for sign, half in ((x, 0), (r - x, 1)):
                acc = 0
                for pos, (i, z) in enumerate(pairs):
                    acc += pow(lam, pos, r) * (trees[i][3][2 * idx + half] - values[pos]) * pow(sign - z, -1, r)
                layer.append(acc % r)
    else:
        q = [0] * P.n
        for pos, (i, z) in enumerate(pairs):
            quo, _ = div_linear([c % r for c in polys[i]], z % r, r)
            for d, c in enumerate(quo):
                q[d] = (q[d] + pow(lam, pos, r) * c) % r
        layer = lde(P, q)
    roots, layers = [], []
    for l in range(P.L):
        alpha = t.challenge()
        layer = fold(P, l, layer, alpha)
        if l + 1 < P.L:
            leaves = leaves_of(layer)
            levels = tree_levels(leaves)
            roots.append(levels[-1][0])
            layers.append((levels, leaves))
            t.append(levels[-1][0])
    # the last layer back to coefficients: inverse transform over <w_L>, unscale by s_L^-i
    nat = natural_order(layer)
    m = len(nat)
    coeffs = [c * pow(m, -1, r) % r for c in fft(nat, pow(P.omega(P.L), -1, r), r)]
    s_inv = pow(P.shift(P.L), -1, r)
    coeffs = [c * pow(s_inv, i, r) % r for i, c in enumerate(coeffs)]
    final = coeffs[:1 << P.f]
    if any(coeffs[1 << P.f:]) and not cheat_value:
        raise RuntimeError("the last layer is not of low degree")
    for c in final:
        t.scalar_in(c)
    queries = []
    for _ in range(P.queries):
        idx = t.challenge() % (P.N // 2)
        from_polys = [(tree[2][idx], tree_path(tree[1], idx)) for tree in trees]
        from_layers = []
        for l, (levels, leaves) in enumerate(layers, start=1):
            j = idx % (P.size(l) // 2)
            from_layers.append((leaves[j], tree_path(levels, j)))
        queries.append((from_polys, from_layers))
    return {"roots": roots, "final": final, "queries": queries}, values


# ---- verifier ---------------------------------------------------------------------------------------------------------------
def verify(P, commitments, pairs, values, proof, transcript=None):
    """commitments: the polynomials' roots; pairs as in prove; values: the claimed p_i(z).  False for anything that does not
    check, a proof of the wrong shape included; never raises on a malformed proof."""
    try:
        return _verify(P, commitments, pairs, values, proof, transcript)
    except (TypeError, ValueError, IndexError, KeyError, AttributeError, OverflowError, ZeroDivisionError):
        return False


def _verify(P, commitments, pairs, values, proof, transcript):
    r = P.r
    roots, final, queries = proof["roots"], proof["final"], proof["queries"]
    if len(roots) != P.L - 1 or len(final) != 1 << P.f or len(queries) != P.queries or len(values) != len(pairs):
        return False
    if any(type(x) is not int or not 0 <= x < r for x in final) or any(len(x) != 64 for x in roots):
        return False
    t = transcript or Transcript(r)
    t.append(P.header())
    for root in commitments:
        if len(root) != 64:
            return False
        t.append(bytes(root))
    for (i, z), v in zip(pairs, values):
        if not 0 <= i < len(commitments) or in_domain(P, z):
            return False
        t.scalar_in(z % r)
        t.scalar_in(v % r)
    lam = t.challenge()
    alphas = []
    for l in range(P.L):
        alphas.append(t.challenge())
        if l + 1 < P.L:
            t.append(bytes(roots[l]))
    for c in final:
        t.scalar_in(c)
    half = pow(2, -1, r)
    for from_polys, from_layers in queries:
        idx = t.challenge() % (P.N // 2)
        if len(from_polys) != len(commitments) or len(from_layers) != P.L - 1:
            return False
        depth = P.k + P.b - 1
        for root, (leaf, path) in zip(commitments, from_polys):
            if len(leaf) != 64 or len(path) != depth or any(len(s) != 64 for s in path) or not path_ok(bytes(root), path, idx, leaf):
                return False
        # layer 0 at x and -x from the openings of the polynomials
        x = P.g * pow(P.w0, idx, r) % r
        lo = hi = 0
        for pos, ((i, z), v) in enumerate(zip(pairs, values)):
            leaf = from_polys[i][0]
            p_lo, p_hi = int.from_bytes(leaf[:32], "little"), int.from_bytes(leaf[32:], "little")
            if p_lo >= r or p_hi >= r:
                return False
            lo += pow(lam, pos, r) * (p_lo - v) * pow(x - z, -1, r)
            hi += pow(lam, pos, r) * (p_hi - v) * pow(-x - z, -1, r)
        lo, hi, pos = lo % r, hi % r, idx
        for l in range(P.L):
            m = P.size(l)
            j = pos % (m // 2)
            if l:
                leaf, path = from_layers[l - 1]
                if len(leaf) != 64 or len(path) != P.k + P.b - l - 1 or any(len(s) != 64 for s in path):
                    return False
                if not path_ok(bytes(roots[l - 1]), path, j, leaf):
                    return False
                lo, hi = int.from_bytes(leaf[:32], "little"), int.from_bytes(leaf[32:], "little")
                if lo >= r or hi >= r or (lo if pos < m // 2 else hi) != value:
                    return False
            xj = P.shift(l) * pow(P.omega(l), j, r) % r
            value = ((lo + hi) * half + alphas[l] * (lo - hi) % r * pow(2 * xj, -1, r)) % r
            pos = j
        if value != poly_eval(final, P.shift(P.L) * pow(P.omega(P.L), pos, r) % r, r):
            return False
    return True


# ---- serialisation ----------------------------------------------------------------------------------------------------------
def proof_bytes(proof):
    """b"FRI1" | u32 roots | u32 final | u32 queries | u32 polynomials per query | u32 layers per query (all big-endian; the last
    two are 0 when there is no query) | the roots, 64 bytes each | the final coefficients, 32 bytes big-endian each | per query,
    per polynomial and then per layer: the 64-byte leaf, one byte = entries of the path, the path's 64-byte entries."""
    roots, final, queries = proof["roots"], proof["final"], proof["queries"]
    n_polys = len(queries[0][0]) if queries else 0
    n_layers = len(queries[0][1]) if queries else 0
    out = [MAGIC] + [x.to_bytes(4, "big") for x in (len(roots), len(final), len(queries), n_polys, n_layers)]
    out += [bytes(x) for x in roots] + [c.to_bytes(32, "big") for c in final]
    for from_polys, from_layers in queries:
        assert len(from_polys) == n_polys and len(from_layers) == n_layers
        for leaf, path in list(from_polys) + list(from_layers):
            out += [bytes(leaf), bytes([len(path)])] + [bytes(s) for s in path]
    return b"".join(out)


def golden_poly(r, count, seed):
    """the polynomials of tests/golden/fri_vectors.json: coefficients from a BLAKE2b counter stream"""
    return [int.from_bytes(H(b"fri-golden" + bytes([seed]) + i.to_bytes(4, "big")), "big") % r for i in range(count)]
