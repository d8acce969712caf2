"""
What the polynomial commitment schemes share, with the reference's interface (python/zksnake/commitment/polynomial/base.py):
`MultiOpeningQuery`, the abstract `PolynomialCommitmentScheme`, and -- because KZG and IPA run the same halo2 multipoint
argument (kzg.py:62-259, ipa.py:219-439 of the reference are the same code twice) -- the two halves of that argument that do not
depend on how a polynomial is committed.

Inside the schemes a polynomial is a `DevVec` of coefficients, low degree first.  A polynomial may be handed in as a univariate
`Polynomial`, a list of ints, an (n, 4) uint64 limb array (canonicalised on upload) or a `DevVec` (used as it is, never
modified); on the path of the last two there is no Python integer per coefficient.

One deliberate difference from the reference.  It orders the groups of a multi-opening, the commitments inside a group and a
group's points by iterating over Python sets, so the order depends on hashes.  Here the order is fixed: groups by the lowest
index in `commitments` among their members, commitments inside a group by that index, points by first appearance in
`opening_points`.  Prover and verifier agree with each other in either implementation; a multi-opening proof is interchangeable
with the reference's exactly when the reference's set order happens to be this one.
"""

from abc import ABC, abstractmethod

import numpy as np

from ...constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from ...ecc import ispointG1, ispointG2
from ...frvec import DevVec, FrOps
from ...polynomial import lagrange_interpolation
from ...transcript import FiatShamirTranscript

_ORDER = {0: BN254_SCALAR_FIELD, 1: BLS12_381_SCALAR_FIELD}
EVAL_MANY_MAX = 64   # zk_poly_eval_many_dev takes this many evaluations per call


def _is_polynomial(x):
    return hasattr(x, "coeffs") and hasattr(x, "is_univariate")


def to_device(ops, polynomial):
    """the polynomial's coefficients as a DevVec (a DevVec is returned as it is)"""
    if isinstance(polynomial, DevVec):
        return polynomial
    if _is_polynomial(polynomial):
        if not polynomial.is_univariate():
            raise TypeError("a univariate polynomial is expected")
        polynomial = polynomial.coeffs()
    if not isinstance(polynomial, (list, tuple, np.ndarray)):
        raise TypeError("a polynomial is a Polynomial, a list of ints, an (n, 4) limb array or a DevVec")
    if isinstance(polynomial, np.ndarray):
        polynomial = ops.limbs(polynomial)
    vec = DevVec(len(polynomial), zero=False)
    ops.d_load(vec, 0, polynomial, vec.n)
    return vec


def _find(items, x):
    """index of x: by identity first, by == only for Polynomial objects, points and bytes (`in` on a numpy array raises); -1 if
    absent"""
    for i, item in enumerate(items):
        if item is x:
            return i
    if _is_polynomial(x) or ispointG1(x) or ispointG2(x) or isinstance(x, bytes):   # bytes: a hash commitment (FRI)
        for i, item in enumerate(items):
            if type(item) is type(x) and item == x:
                return i
    return -1


def _index(items, x):
    i = _find(items, x)
    if i < 0:
        raise ValueError("not part of this query")
    return i


class MultiOpeningQuery:
    """The reference's query object.  `add_polynomial` uploads the polynomial once (when the commitment tells the curve; a
    polynomial that came in through `prover_query` alone is uploaded by `multi_open`).  `prover_query` leaves the evaluation to
    `multi_open` unless one is given: `evaluations[point][index]` is None until then."""

    def __init__(self):
        self.polynomials = []
        self.commitments = []
        self.opening_points = {}
        self.evaluations = {}
        self.blindings = []
        self._vectors = []    # DevVec (or None: not uploaded yet) per polynomial

    def _query(self, index, point, evaluation):
        if point not in self.opening_points:
            self.opening_points[point] = [index]
            self.evaluations[point] = {index: evaluation}
        else:
            self.opening_points[point] += [index]
            self.evaluations[point][index] = evaluation

    def prover_query(self, polynomial, point, evaluation=None):
        index = _find(self.polynomials, polynomial)
        if index < 0:
            self.polynomials.append(polynomial)
            self._vectors.append(polynomial if isinstance(polynomial, DevVec) else None)
            index = len(self.polynomials) - 1
        self._query(index, point, evaluation)

    def verifier_query(self, commitment, point, evaluation):
        index = _find(self.commitments, commitment)
        if index < 0:
            self.commitments.append(commitment)
            index = len(self.commitments) - 1
        self._query(index, point, evaluation)

    def to_polynomial(self, commitment):
        return self.polynomials[_index(self.commitments, commitment)]

    def to_commitment(self, polynomial):
        return self.commitments[_index(self.polynomials, polynomial)]

    def get_blinding(self, commitment):
        return self.blindings[_index(self.commitments, commitment)]

    def get_evaluation(self, commitment, point):
        return self.evaluations[point][_index(self.commitments, commitment)]

    def add_polynomial(self, polynomial, commitment, blinding=None):
        if _find(self.polynomials, polynomial) >= 0:
            return
        vec = polynomial if isinstance(polynomial, DevVec) else None
        if vec is None and (ispointG1(commitment) or ispointG2(commitment)):
            vec = to_device(FrOps(_ORDER[commitment.CURVE]), polynomial)
        self.polynomials += [polynomial]
        self.commitments += [commitment]
        self.blindings += [blinding if blinding else 1]
        self._vectors += [vec]

    def vector(self, index, ops):
        """polynomial `index` on the device"""
        if self._vectors[index] is None:
            self._vectors[index] = to_device(ops, self.polynomials[index])
        return self._vectors[index]

    def get_polynomials(self):
        item = self.polynomials
        for point, idx in self.opening_points.items():
            yield point, [item[i] for i in idx]

    def get_commitments(self):
        item = self.commitments
        for point, idx in self.opening_points.items():
            yield point, [item[i] for i in idx]

    def groups(self):
        """[(indices, points)]: the polynomials (commitments) that are opened at the same set of points, in the fixed order of the
        module docstring"""
        points_of = {}
        for point, idx in self.opening_points.items():
            for i in idx:
                seen = points_of.setdefault(i, [])
                if point not in seen:
                    seen.append(point)
        out = {}
        for i in sorted(points_of):
            key = frozenset(points_of[i])
            if key not in out:
                out[key] = ([], points_of[i])
            out[key][0].append(i)
        order = {point: k for k, point in enumerate(self.opening_points)}
        return [(members, sorted(points, key=order.__getitem__)) for members, points in out.values()]


class PolynomialCommitmentScheme(ABC):

    def __init__(self, max_degree, group):
        self.degree = max_degree
        self.group = group
        self.order = None
        self.name = ""
        self.is_setup = False
        self._ops = None

    def list_to_poly(self, values):
        assert len(values) <= self.degree
        return lagrange_interpolation(list(range(len(values))), values, self.order)

    @abstractmethod
    def zero_commitment(self):
        raise NotImplementedError()

    @abstractmethod
    def setup(self):
        raise NotImplementedError()

    @abstractmethod
    def commit(self, polynomial):
        raise NotImplementedError()

    @abstractmethod
    def open(self, polynomial, point):
        raise NotImplementedError()

    @abstractmethod
    def verify(self, commitment, proof, point, evaluation, transcript=None):
        raise NotImplementedError()

    @abstractmethod
    def multi_open(self, points_query: MultiOpeningQuery, transcript: FiatShamirTranscript = None):
        raise NotImplementedError()

    @abstractmethod
    def multi_verify(self, points_query: MultiOpeningQuery, proof: list, transcript: FiatShamirTranscript = None):
        raise NotImplementedError()

    # -- the multipoint argument (https://zcash.github.io/halo2/design/proving-system/multipoint-opening.html), scheme independent --
    def _vec(self, polynomial, limit):
        vec = to_device(self._ops, polynomial)
        if vec.n > limit:
            raise ValueError(f"the polynomial has {vec.n} coefficients, the scheme takes at most {limit}")
        return vec

    def _eval_many(self, jobs):
        out = []
        for i in range(0, len(jobs), EVAL_MANY_MAX):
            out += self._ops.d_eval_many(jobs[i:i + EVAL_MANY_MAX])
        return out

    def _multi_open_polys(self, query, transcript, limit):
        """Up to the commitment to f: every evaluation in one pass (written back into `query`, collected in a verifier's query and
        appended to the transcript), q_i = sum_j x1^j p_j per group, f_i = q_i / prod (X - z) over the group's points as a chain of
        linear divisions with the remainders ignored -- it equals (q_i - r_i) / prod (X - z), because deg r_i is below the number of
        points, repeated roots included -- and f = sum_i x2^i f_i.  Returns (verifier's query, groups, q vectors, f, size, x1)."""
        ops, r = self._ops, self.order
        transcript.append(query.commitments)
        vecs = [query.vector(i, ops) for i in range(len(query.polynomials))]
        for vec in vecs:
            if vec.n > limit:
                raise ValueError(f"a polynomial has {vec.n} coefficients, the scheme takes at most {limit}")
        asked = [(point, i) for point, idx in query.opening_points.items() for i in idx]
        values = self._eval_many([(vecs[i].n, vecs[i].ptr(), point) for point, i in asked])
        verifier_query = MultiOpeningQuery()
        for (point, i), value in zip(asked, values):
            query.evaluations[point][i] = value
            verifier_query.verifier_query(query.commitments[i], point, value)
            transcript.append(value)
        x1 = transcript.get_challenge_scalar()
        x2 = transcript.get_challenge_scalar()

        groups = query.groups()
        size = max([vec.n for vec in vecs] + [1])
        q_vecs, keep, f_terms = [], [], []
        for g, (members, points) in enumerate(groups):
            q = DevVec(size)
            ops.d_lincomb(q, [(vecs[i].n, pow(x1, j, r), vecs[i].ptr()) for j, i in enumerate(members) if vecs[i].n])
            q_vecs.append(q)
            cur, count = q, size
            spare = [DevVec(size, zero=False), DevVec(size, zero=False)]
            for t, z in enumerate(points):
                if count <= 1:        # a constant divided by a linear factor: the quotient is zero
                    count = 0
                    break
                ops.d_div_linear(count, cur.ptr(), z, spare[t & 1].ptr())
                cur, count = spare[t & 1], count - 1
            keep.append(cur)
            if count:
                f_terms.append((count, pow(x2, g, r), cur.ptr()))
        f = DevVec(size)
        ops.d_lincomb(f, f_terms)
        return verifier_query, groups, q_vecs, f, size, x1

    def _multi_open_final(self, q_vecs, f, size, x3, transcript):
        """(q_i(x3) list, x4); f becomes the final polynomial f + sum_i x4^(i+1) q_i in place"""
        ops, r = self._ops, self.order
        q_x3 = self._eval_many([(size, q.ptr(), x3) for q in q_vecs])
        transcript.append(q_x3)
        x4 = transcript.get_challenge_scalar()
        ops.d_lincomb(f, [(size, pow(x4, i + 1, r), q.ptr()) for i, q in enumerate(q_vecs)])
        return q_x3, x4

    def _multi_verify_front(self, query, proof, transcript):
        """the verifier's side up to the single opening it ends in: (final commitment, x3, the final polynomial's value at x3,
        opening proof), or None for a proof of the wrong shape.  The Lagrange part runs on the host over a handful
        of points."""
        r = self.order
        transcript.append(query.commitments)
        for point, idx in query.opening_points.items():
            for i in idx:
                transcript.append(query.evaluations[point][i])
        x1 = transcript.get_challenge_scalar()
        x2 = transcript.get_challenge_scalar()
        f_commitment, q_x3, opening_proof = proof[0], list(proof[1:-1]), proof[-1]
        transcript.append(f_commitment)
        x3 = transcript.get_challenge_scalar()
        transcript.append(q_x3)
        x4 = transcript.get_challenge_scalar()

        groups = query.groups()
        if len(groups) != len(q_x3):
            return None
        f_x3, q_x4 = 0, 0
        final_commitment = f_commitment
        for g, (members, points) in enumerate(groups):
            q_commitment = self.zero_commitment()
            for j, i in enumerate(members):
                q_commitment = q_commitment + query.commitments[i] * pow(x1, j, r)
            ys = [sum(pow(x1, j, r) * query.evaluations[point][i] for j, i in enumerate(members)) % r for point in points]
            r_x3, denominator = 0, 1
            for a, (xa, ya) in enumerate(zip(points, ys)):     # r_g(x3) by Lagrange's formula
                num, den = ya, 1
                for b, xb in enumerate(points):
                    if b != a:
                        num = num * (x3 - xb) % r
                        den = den * (xa - xb) % r
                r_x3 = (r_x3 + num * pow(den, -1, r)) % r
                denominator = denominator * (x3 - xa) % r
            if denominator == 0:
                return None
            f_x3 += pow(x2, g, r) * (q_x3[g] - r_x3) * pow(denominator, -1, r) % r
            final_commitment = final_commitment + q_commitment * pow(x4, g + 1, r)
            q_x4 += pow(x4, g + 1, r) * q_x3[g]
        return final_commitment, x3, (f_x3 + q_x4) % r, opening_proof
