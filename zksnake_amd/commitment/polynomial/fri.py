"""
FRI: a hash-based polynomial commitment (transparent: no trusted setup, no curve, no MSM) over the NTT and the BLAKE2b Merkle
kernels.  The reference has no FRI, so there is nothing to interchange proofs with; the protocol below is this project's own
and tests/fri_model.py is its integer model.

`FRI(max_degree, curve="BN254", blowup=4, queries=64, final=16)`, all four numbers powers of two: n = max_degree = 2^k is the
most coefficients a polynomial may have, B = 2^b = blowup, N = n B <= 2^26 the size of the evaluation domain, `final` = 2^f < n
the coefficients sent in the clear after L = k - f folds.

  Domain.     Layer l lives on the coset s_l <w_l> of M_l = N >> l points: s_0 = g, the field's multiplicative generator (5 on
              BN254, 7 on BLS12-381), w_0 = the library's root of unity of order N, s_(l+1) = s_l^2, w_(l+1) = w_l^2.
  Pair order. A layer f of M = 2h values is stored and hashed as g[2j] = f[j], g[2j+1] = f[j+h]: f(x_j) and f(-x_j).  Leaf j of
              its Merkle tree is le32(f[j]) || le32(f[j+h]); a commitment is the tree's 64-byte root; one path opens both values.
  Fold.       f'[j] = (f[j] + f[j+h]) / 2 + alpha (f[j] - f[j+h]) / (2 s_l w_l^j) for j < h, in pair order of the h values.

multi_open (open is this with one pair), pairs (i_k, z_k) in `opening_points` order, every field element appended to the
transcript as 32 bytes big-endian:
  1. append b"zksnake-amd-fri-v1" || bytes([curve id, k, b, f]) || queries on 4 bytes big-endian;
  2. append every polynomial's root; 3. per pair append z_k, then v_k = p_i(z_k) (a z_k inside the domain is a ValueError);
  4. draw lambda; 5. q = sum_k lambda^k (p_i - v_k) / (X - z_k) in coefficients (linear divisions, one linear combination);
  6. layer 0 = the extension of q -- NOT committed: the verifier derives it from the openings of the p_i;
  7. L times: draw alpha_l, fold, and for all but the last layer build its tree and append the root;
  8. the last layer goes back to `final` coefficients (the rest must be zero), which are appended;
  9. per query draw idx = challenge mod N/2 (duplicates kept) and open leaf idx of every polynomial's tree and leaf
     idx mod M_l/2 of every committed layer l = 1 .. L-1.
`verify` / `multi_verify` replay this on the host with hashlib and Python ints and need no GPU.

Conjectured soundness is about queries * b bits (64 * 2 = 128 at the defaults), roughly half of that is proven.  There is no
grinding and no zero-knowledge blinding; commitments are not homomorphic (`zero_commitment` raises), so the halo2 multipoint
argument of base.py is not used: the quotients are batched with lambda instead.

`FRI.oracle(polynomial)` keeps the coefficients, the pair-order evaluations and the tree in device memory (`FriOracle`), so a
polynomial is extended and hashed once however often it is opened: `open` and `multi_open` take an oracle in place of a
polynomial, and `commit` is a thin wrapper over it.

FriProof.to_bytes: b"FRI1" | u32 roots | u32 final | u32 queries | u32 polynomials per query | u32 layers per query (big-endian;
the last two are 0 without a query) | the roots, 64 bytes each | the final coefficients, 32 bytes big-endian each | per query,
per polynomial and then per layer: the 64-byte leaf, one byte = entries of the path, the path's 64-byte entries.
"""

import hashlib
import operator

import numpy as np

from ... import _native as N
from ...device import DeviceBuffer
from ...frvec import DevVec, FrOps
from ...transcript import FiatShamirTranscript
from ..vector.merkle import DIGEST, MerkleTree
from .base import _ORDER, MultiOpeningQuery, PolynomialCommitmentScheme

TAG = b"zksnake-amd-fri-v1"
MAGIC = b"FRI1"
COSET_SHIFT = {N.CURVE_BN254: 5, N.CURVE_BLS12_381: 7}   # multiplicative generators of the scalar fields
MAX_QUERIES = 1 << 16
LEAF = 64   # two field elements


def _log2(value, what):
    value = operator.index(value)
    if value < 1 or value & (value - 1):
        raise ValueError(f"{what} is a power of two, not {value}")
    return value.bit_length() - 1


def _be32(x):
    return int(x).to_bytes(32, "big")


class FriProof:
    """roots: the committed layers' roots (layers 1 .. L-1); final: the last layer's coefficients; queries: per query
    (per polynomial [(leaf, path)], per committed layer [(leaf, path)]), a leaf 64 bytes, a path a list of 64-byte nodes"""

    def __init__(self, roots, final, queries):
        self.roots, self.final, self.queries = roots, final, queries

    def _canon(self):
        return ([bytes(x) for x in self.roots], [int(x) for x in self.final],
                [[[(bytes(leaf), [bytes(s) for s in path]) for leaf, path in part] for part in query] for query in self.queries])

    def __eq__(self, other):
        if not isinstance(other, FriProof):
            return NotImplemented
        try:
            return self._canon() == other._canon()
        except (TypeError, ValueError):
            return False

    __hash__ = None

    def to_bytes(self):
        roots, final, queries = self._canon()
        n_polys = len(queries[0][0]) if queries else 0
        n_layers = len(queries[0][1]) if queries else 0
        out = [MAGIC] + [x.to_bytes(4, "big") for x in (len(roots), len(final), len(queries), n_polys, n_layers)]
        out += roots + [_be32(c) for c in final]
        for query in queries:
            if len(query) != 2 or len(query[0]) != n_polys or len(query[1]) != n_layers:
                raise ValueError("every query opens the same polynomials and layers")
            for leaf, path in query[0] + query[1]:
                if len(leaf) != LEAF or len(path) > 255 or any(len(s) != DIGEST for s in path):
                    raise ValueError("a leaf is 64 bytes and a path at most 255 nodes of 64 bytes")
                out += [leaf, bytes([len(path)])] + path
        return b"".join(out)

    @classmethod
    def from_bytes(cls, data):
        data = bytes(data)
        if len(data) < 24 or data[:4] != MAGIC:
            raise ValueError("not a FRI proof")
        n_roots, n_final, n_queries, n_polys, n_layers = (int.from_bytes(data[4 + 4 * i:8 + 4 * i], "big") for i in range(5))
        if 24 + DIGEST * n_roots + 32 * n_final + n_queries * (n_polys + n_layers) * (LEAF + 1) > len(data):
            raise ValueError("the proof is shorter than its header says")
        at = 24

        def take(count):
            nonlocal at
            if at + count > len(data):
                raise ValueError("the proof is shorter than its header says")
            at += count
            return data[at - count:at]

        roots = [take(DIGEST) for _ in range(n_roots)]
        final = [int.from_bytes(take(32), "big") for _ in range(n_final)]
        queries = []
        for _ in range(n_queries):
            parts = []
            for count in (n_polys, n_layers):
                part = []
                for _ in range(count):
                    leaf = take(LEAF)
                    part.append((leaf, [take(DIGEST) for _ in range(take(1)[0])]))
                parts.append(part)
            queries.append(tuple(parts))
        if at != len(data):
            raise ValueError("bytes after the proof")
        return cls(roots, final, queries)


class FriOracle:
    """a committed polynomial, resident in device memory until release(): its coefficients (`coeffs`, a DevVec, not modified), its
    N evaluations on the coset in pair order (`evals`) and the Merkle tree over their N/2 leaves (`tree`); `root` is the commitment"""

    def __init__(self, key, coeffs, evals, tree):
        self._key, self.coeffs, self.evals, self.tree = key, coeffs, evals, tree
        self.root = tree.root

    def release(self):
        if self.tree is not None:
            self.tree.release()
        self.tree = self.evals = self.coeffs = None


def _tree_over(evals, leaves):
    """the tree over a pair-order layer: its leaves are the layer's memory, 64 bytes each"""
    return MerkleTree.from_device_rows(leaves, evals.ptr(), LEAF)


def _rows(ptr, n_rows, d_idx, k):
    """rows d_idx[q] of the n_rows 64-byte rows at ptr as (k, 64) uint8: one launch, one download"""
    out = DeviceBuffer(k * LEAF)
    try:
        N.check(N.load().zk_fri_rows_dev(n_rows, LEAF, ptr, k, d_idx.ptr, out.ptr, None))
        return out.download((k, LEAF), np.uint8)
    finally:
        out.free()


class FRI(PolynomialCommitmentScheme):
    """FRI(max_degree, curve, blowup=4, queries=64, final=16); see the module docstring.  `setup()` has nothing to do."""

    def __init__(self, max_degree, group="BN254", blowup=4, queries=64, final=16):
        super().__init__(max_degree, group)
        self.name = "FRI"
        self.k, self.b, self.f = _log2(max_degree, "max_degree"), _log2(blowup, "blowup"), _log2(final, "final")
        self.queries = operator.index(queries)
        if self.b < 1:
            raise ValueError("blowup is at least 2")
        if self.k + self.b > N.FRI_MAX_LOG:
            raise ValueError(f"max_degree * blowup is at most 2^{N.FRI_MAX_LOG}")
        if self.f >= self.k:
            raise ValueError("final is below max_degree: there is at least one fold")
        if not 1 <= self.queries <= MAX_QUERIES:
            raise ValueError(f"1 <= queries <= {MAX_QUERIES}")
        try:
            self.cid = N.curve_id(group)
        except KeyError:
            raise ValueError(f"unknown curve {group!r}") from None
        self.order = _ORDER[self.cid]
        self._ops = FrOps(self.order)
        self.n, self.size, self.folds = 1 << self.k, 1 << (self.k + self.b), self.k - self.f
        self.shift = COSET_SHIFT[self.cid]
        self._w0 = None
        self._key = (self.cid, self.k, self.b)

    # -- parameters: host arithmetic only --
    def setup(self):
        self.is_setup = True

    def zero_commitment(self):
        raise NotImplementedError("hash commitments are not homomorphic")

    def _omega0(self):
        if self._w0 is None:
            out = np.zeros(4, dtype=np.uint64)
            N.check(N.load().zk_fr_root_of_unity(self.cid, self.size, N.u64p(out)))   # host arithmetic of the library, no GPU
            self._w0 = int.from_bytes(out.tobytes(), "little")
        return self._w0

    def _header(self):
        return TAG + bytes([self.cid, self.k, self.b, self.f]) + self.queries.to_bytes(4, "big")

    def _in_domain(self, z):
        return pow(z, self.size, self.order) == pow(self.shift, self.size, self.order)

    def _point(self, z):
        z = operator.index(z) % self.order
        if self._in_domain(z):
            raise ValueError("an opening point lies in the evaluation domain")
        return z

    def _fold_value(self, l, j, lo, hi, alpha):
        """the fold of the pair (lo, hi) at position j of layer l"""
        r = self.order
        x = pow(self.shift, 1 << l, r) * pow(self._omega0(), j << l, r) % r
        return ((lo + hi) * pow(2, -1, r) + alpha * (lo - hi) % r * pow(2 * x, -1, r)) % r

    # -- prover --
    def oracle(self, polynomial):
        """extend and hash the polynomial on the GPU; the caller release()s the oracle (or drops it).  An oracle of a scheme
        with the same curve, max_degree and blowup is returned as it is."""
        if isinstance(polynomial, FriOracle):
            if polynomial._key != self._key or polynomial.tree is None:
                raise ValueError("the oracle is released or belongs to a scheme of another shape")
            return polynomial
        if isinstance(polynomial, (list, tuple, DevVec)):     # refused before any device call
            count = polynomial.n if isinstance(polynomial, DevVec) else len(polynomial)
            if count > self.n:
                raise ValueError(f"the polynomial has {count} coefficients, the scheme takes at most {self.n}")
        N.ensure_gpu()
        coeffs = self._vec(polynomial, self.n)
        evals = self._extend(coeffs, coeffs.n)
        return FriOracle(self._key, coeffs, evals, _tree_over(evals, self.size // 2))

    def _extend(self, coeffs, count):
        work, evals = DevVec(self.size, zero=False), DevVec(self.size, zero=False)
        N.check(N.load().zk_fri_lde_dev(self.cid, self.k, self.b, count, coeffs.ptr() if count else None, N.u64p(self._ops.one(self.shift)),
                                        work.ptr(), evals.ptr(), None))
        return evals

    def commit(self, polynomial):
        oracle = self.oracle(polynomial)
        try:
            return oracle.root
        finally:
            if oracle is not polynomial:
                oracle.release()

    def open(self, polynomial, point, transcript=None):
        """(proof, p(point))"""
        z = self._point(point)
        oracle = self.oracle(polynomial)
        try:
            proof, values = self._prove([oracle], [(0, z)], transcript)
            return proof, values[0]
        finally:
            if oracle is not polynomial:
                oracle.release()

    def multi_open(self, points_query: MultiOpeningQuery, transcript: FiatShamirTranscript = None):
        """(proof, the verifier's query).  The polynomials of the query may be oracles; the evaluations are written back into it."""
        query = points_query
        asked = [(point, i) for point, idx in query.opening_points.items() for i in idx]
        pairs = [(i, self._point(point)) for point, i in asked]
        N.ensure_gpu()
        oracles = []
        try:
            for i, polynomial in enumerate(query.polynomials):
                oracles.append(self.oracle(polynomial if isinstance(polynomial, FriOracle) else query.vector(i, self._ops)))
            proof, values = self._prove(oracles, pairs, transcript)
            verifier_query = MultiOpeningQuery()
            for (point, i), value in zip(asked, values):
                query.evaluations[point][i] = value
                verifier_query.verifier_query(oracles[i].root, point, value)
            return proof, verifier_query
        finally:
            for oracle, polynomial in zip(oracles, query.polynomials):
                if oracle is not polynomial:
                    oracle.release()

    def _prove(self, oracles, pairs, transcript):
        ops, r, lib = self._ops, self.order, N.load()
        t = transcript or FiatShamirTranscript(field=r)
        t.append(self._header())
        for oracle in oracles:
            t.append(oracle.root)
        values, quotients = [], []
        for i, z in pairs:
            coeffs = oracles[i].coeffs
            quotient = DevVec(max(coeffs.n - 1, 1), zero=False)
            values.append(ops.d_div_linear(coeffs.n, coeffs.ptr(), z, quotient.ptr()) if coeffs.n else 0)
            quotients.append((coeffs.n - 1, quotient))
            t.append(_be32(z))
            t.append(_be32(values[-1]))
        lam = t.get_challenge_scalar()
        q = DevVec(self.n)
        ops.d_lincomb(q, [(count, pow(lam, pos, r), vec.ptr()) for pos, (count, vec) in enumerate(quotients) if count > 0])
        layer = self._extend(q, self.n)   # layer 0: not committed
        del quotients, q

        roots, layers = [], []          # of layers 1 .. L-1: (evaluations, tree)
        try:
            for l in range(self.folds):
                alpha = t.get_challenge_scalar()
                s, w = pow(self.shift, 1 << l, r), pow(self._omega0(), 1 << l, r)
                m = self.size >> l
                folded = DevVec(m // 2, zero=False)
                N.check(lib.zk_fri_fold_dev(self.cid, self.k + self.b - l, layer.ptr(), N.u64p(ops.one(alpha * pow(2 * s, -1, r))),
                                            N.u64p(ops.one(pow(w, -1, r))), folded.ptr(), None))
                layer = folded
                if l + 1 < self.folds:
                    layers.append((layer, _tree_over(layer, m // 4)))
                    roots.append(layers[-1][1].root)
                    t.append(roots[-1])
            final = self._final_coefficients(layer)
            for c in final:
                t.append(_be32(c))

            half = self.size // 2
            idx = [t.get_challenge_scalar() % half for _ in range(self.queries)]
            k = len(idx)
            opened = []    # per tree: (leaves (k, 64), paths (k, depth, 64))
            sources = [(o.evals, o.tree, half) for o in oracles] + [(ev, tree, tree.n) for ev, tree in layers]
            for evals, tree, leaves in sources:
                at = np.array([i % leaves for i in idx], dtype=np.uint64)
                d_idx = DeviceBuffer.from_numpy(at)
                try:
                    opened.append((_rows(evals.ptr(), leaves, d_idx, k), tree.open_many(at)))
                finally:
                    d_idx.free()
        finally:
            for _, tree in layers:
                tree.release()
        queries = []
        for q_at in range(k):
            parts = [(rows[q_at].tobytes(), [node.tobytes() for node in paths[q_at]]) for rows, paths in opened]
            queries.append((parts[:len(oracles)], parts[len(oracles):]))
        return FriProof(roots, final, queries), values

    def _final_coefficients(self, layer):
        """the last layer (pair order, on s_L <w_L>) as `final` coefficients: inverse transform, unscale by s_L^-i"""
        ops, r = self._ops, self.order
        pairs = layer.download()
        natural = np.concatenate([pairs[0::2], pairs[1::2]])
        coeffs = ops.ints(ops.ntt(natural, natural.shape[0], inverse=True))
        s_inv, t = pow(self.shift, -(1 << self.folds), r), 1
        for i in range(len(coeffs)):
            coeffs[i] = coeffs[i] * t % r
            t = t * s_inv % r
        if any(coeffs[1 << self.f:]):
            raise RuntimeError("the last FRI layer is not of low degree")
        return coeffs[:1 << self.f]

    # -- verifier: host only --
    def verify(self, commitment, proof, point, evaluation, transcript=None):
        return self._verify([commitment], [(0, point)], [evaluation], proof, transcript)

    def multi_verify(self, points_query: MultiOpeningQuery, proof, transcript: FiatShamirTranscript = None):
        query = points_query
        try:
            asked = [(point, i) for point, idx in query.opening_points.items() for i in idx]
            values = [query.evaluations[point][i] for point, i in asked]
            return self._verify(query.commitments, [(i, point) for point, i in asked], values, proof, transcript)
        except (TypeError, KeyError, IndexError, AttributeError):
            return False

    def _verify(self, commitments, pairs, values, proof, transcript):
        try:
            return self._verify_checked(commitments, pairs, values, proof, transcript)
        except (TypeError, ValueError, IndexError, KeyError, AttributeError, OverflowError, ZeroDivisionError):
            return False     # a proof (or a query) of the wrong shape

    def _path_ok(self, root, path, index, leaf, depth):
        if len(leaf) != LEAF or len(path) != depth or any(len(s) != DIGEST for s in path):
            return False
        digest = hashlib.blake2b(leaf).digest()
        for sibling in path:      # the reference's verify loop (vector/merkle.py)
            digest = hashlib.blake2b(sibling + digest if index & 1 else digest + sibling).digest()
            index >>= 1
        return digest == root

    def _verify_checked(self, commitments, pairs, values, proof, transcript):
        r, L = self.order, self.folds
        roots, final, queries = [bytes(x) for x in proof.roots], list(proof.final), list(proof.queries)
        commitments = [bytes(x) for x in commitments]
        if len(roots) != L - 1 or len(final) != 1 << self.f or len(queries) != self.queries or len(values) != len(pairs):
            return False
        if any(type(c) is not int or not 0 <= c < r for c in final) or any(len(x) != DIGEST for x in roots + commitments):
            return False
        pairs = [(operator.index(i), operator.index(z) % r) for i, z in pairs]
        values = [operator.index(v) % r for v in values]
        if any(not 0 <= i < len(commitments) or self._in_domain(z) for i, z in pairs):
            return False
        t = transcript or FiatShamirTranscript(field=r)
        t.append(self._header())
        for root in commitments:
            t.append(root)
        for (_, z), v in zip(pairs, values):
            t.append(_be32(z))
            t.append(_be32(v))
        lam = t.get_challenge_scalar()
        alphas = []
        for l in range(L):
            alphas.append(t.get_challenge_scalar())
            if l + 1 < L:
                t.append(roots[l])
        for c in final:
            t.append(_be32(c))
        half, depth0, w0 = self.size // 2, self.k + self.b - 1, self._omega0()
        weights = [pow(lam, pos, r) for pos in range(len(pairs))]
        for query in queries:
            idx = t.get_challenge_scalar() % half
            from_polys, from_layers = query
            if len(from_polys) != len(commitments) or len(from_layers) != L - 1:
                return False
            opened = []
            for root, (leaf, path) in zip(commitments, from_polys):
                leaf, path = bytes(leaf), [bytes(s) for s in path]
                if not self._path_ok(root, path, idx, leaf, depth0):
                    return False
                opened.append((int.from_bytes(leaf[:32], "little"), int.from_bytes(leaf[32:], "little")))
                if max(opened[-1]) >= r:
                    return False
            # layer 0 at x and at -x from the openings of the polynomials
            x, lo, hi = self.shift * pow(w0, idx, r) % r, 0, 0
            for weight, (i, z), v in zip(weights, pairs, values):
                lo += weight * (opened[i][0] - v) * pow(x - z, -1, r)
                hi += weight * (opened[i][1] - v) * pow(-x - z, -1, r)
            lo, hi, pos = lo % r, hi % r, idx
            for l in range(L):
                m = self.size >> l
                j = pos % (m // 2)
                if l:
                    leaf, path = bytes(from_layers[l - 1][0]), [bytes(s) for s in from_layers[l - 1][1]]
                    if not self._path_ok(roots[l - 1], path, j, leaf, depth0 - l):
                        return False
                    lo, hi = int.from_bytes(leaf[:32], "little"), int.from_bytes(leaf[32:], "little")
                    if lo >= r or hi >= r or (lo if pos < m // 2 else hi) != value:
                        return False
                value = self._fold_value(l, j, lo, hi, alphas[l])
                pos = j
            x, acc = pow(self.shift, 1 << L, r) * pow(w0, pos << L, r) % r, 0
            for c in reversed(final):
                acc = (acc * x + c) % r
            if value != acc:
                return False
        return True
