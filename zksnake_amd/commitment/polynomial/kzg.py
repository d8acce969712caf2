"""
KZG polynomial commitments with the reference's interface and equations (python/zksnake/commitment/polynomial/kzg.py) over
device-resident coefficients: the powers of tau are one MSM plan in HBM, a commitment is one plan run, an opening is ONE linear
division (its remainder is the evaluation, so there is no separate evaluation pass and no subtraction) and one plan run over
the quotient, a multi-opening is two.  With the same tau, `commit` and `open` give the reference's group elements.  G1
commitments, both curves.  base.py has the one deliberate difference of `multi_open` / `multi_verify` (a fixed group order).
"""

from ... import _native as N
from ..._algebra import PointArray
from ...ecc import EllipticCurve
from ...frvec import DevVec, FrOps
from ...transcript import FiatShamirTranscript
from ...utils import get_random_int
from .base import MultiOpeningQuery, PolynomialCommitmentScheme

MAX_BASES = 1 << 26   # what an MSM plan takes (zk_msm_plan_create)


class KZG(PolynomialCommitmentScheme):
    """KZG(max_degree, curve).  `setup(tau=None)` draws tau unless one is given.  `G1_tau` (a PointArray of max_degree + 1
    points) and `G2_tau` may be assigned, which is how an existing SRS is loaded; assigning `G1_tau` drops its MSM plan."""

    def __init__(self, max_degree, group):
        super().__init__(max_degree, group)
        self.name = "KZG"
        if max_degree < 0 or max_degree + 1 > MAX_BASES:
            raise ValueError(f"KZG takes at most {MAX_BASES} powers of tau")
        self.E = EllipticCurve(self.group)
        self.order = self.E.order
        self._ops = FrOps(self.order)
        self._G1_tau = None
        self._G2_tau = None

    # -- the SRS --
    def _set_g1(self, points):
        if points is not None:
            points = PointArray.from_points(self.E.curve_id, 1, points, count=self.degree + 1, what="powers of tau")
        if self._G1_tau is not None and self._G1_tau is not points:
            self._G1_tau.release()
        self._G1_tau = points
        self.is_setup = self._G1_tau is not None and self._G2_tau is not None

    def _set_g2(self, point):
        if point is not None and not isinstance(point, self.E.curve.PointG2):
            raise TypeError("tau in G2 is a G2 point of the scheme's curve")
        self._G2_tau = point
        self.is_setup = self._G1_tau is not None and self._G2_tau is not None

    G1_tau = property(lambda self: self._G1_tau, _set_g1)
    G2_tau = property(lambda self: self._G2_tau, _set_g2)

    def setup(self, tau=None):
        N.ensure_gpu()
        if tau is None:
            tau = get_random_int(self.order)
        powers = self._ops.d_powers(tau % self.order, self.degree + 1).download()
        self.G1_tau = self.E.batch_mul(self.E.G1(), powers, as_array=True)
        self.G2_tau = self.E.G2() * (tau % self.order)

    def zero_commitment(self):
        return self.E.curve.PointG1.identity()

    def commit(self, polynomial):
        assert self.is_setup, "Trusted setup has not been run"
        N.ensure_gpu()
        vec = self._vec(polynomial, self.degree + 1)
        return self._G1_tau.msm(vec)

    def _open_vec(self, vec, count, point):
        """(proof, evaluation) for the first `count` coefficients of a device vector"""
        if count == 0:
            return self.zero_commitment(), 0
        quotient = DevVec(max(count - 1, 1), zero=False)
        evaluation = self._ops.d_div_linear(count, vec.ptr(), point % self.order, quotient.ptr())
        return self._G1_tau.msm(quotient, count - 1), evaluation

    def open(self, polynomial, point):
        assert self.is_setup, "Trusted setup has not been run"
        N.ensure_gpu()
        vec = self._vec(polynomial, self.degree + 1)
        return self._open_vec(vec, vec.n, point)

    def verify(self, commitment, proof, point, evaluation, transcript=None):
        assert self.is_setup, "Trusted setup has not been run"
        r = self.order
        lhs = self.E.pairing(proof, self._G2_tau - self.E.G2() * (point % r))
        rhs = self.E.pairing(commitment - self.E.G1() * (evaluation % r), self.E.G2())
        return lhs == rhs

    def multi_open(self, points_query: MultiOpeningQuery, transcript: FiatShamirTranscript = None):
        """(proof, the verifier's query).  proof = [commitment to f, q_1(x3), .., q_k(x3), opening of the final polynomial at x3]"""
        assert self.is_setup, "Trusted setup has not been run"
        N.ensure_gpu()
        transcript = transcript or FiatShamirTranscript(self.name.encode(), self.order)
        verifier_query, _, q_vecs, f, size, _ = self._multi_open_polys(points_query, transcript, self.degree + 1)
        f_commitment = self._G1_tau.msm(f, size)
        transcript.append(f_commitment)
        x3 = transcript.get_challenge_scalar()
        q_x3, _ = self._multi_open_final(q_vecs, f, size, x3, transcript)
        opening_proof, _ = self._open_vec(f, size, x3)
        return [f_commitment] + q_x3 + [opening_proof], verifier_query

    def multi_verify(self, points_query: MultiOpeningQuery, proof: list, transcript: FiatShamirTranscript = None):
        assert self.is_setup, "Trusted setup has not been run"
        assert len(proof) > 2, "Invalid proof"
        transcript = transcript or FiatShamirTranscript(self.name.encode(), self.order)
        front = self._multi_verify_front(points_query, proof, transcript)
        if front is None:
            return False
        final_commitment, x3, final_value, opening_proof = front
        return self.verify(final_commitment, opening_proof, x3, final_value)
