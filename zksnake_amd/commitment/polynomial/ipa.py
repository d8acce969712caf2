"""
The inner-product polynomial commitment of BCMS20 (https://eprint.iacr.org/2020/499.pdf, appendix A) with the reference's
interface, equations and transcript (python/zksnake/commitment/polynomial/ipa.py).

The reference folds n generators on the host every round and keeps b = (1, z, z^2, ..) as a list.  Here G is NEVER folded and b
does not exist: with s_i = prod_{t<k} (bit (log_n-1-t) of i ? u_t : 1) the folded generator is G^(k)_j = sum_{i = j mod m} s_i G_i
and the folded b^(k)_j is B_k z^j with the single scalar B_k = prod_{t<k} (1 + u_t z^(n >> (t+1))), so with m = n >> k, h = m / 2

    L_k = <scal_L, G> + B_k     (sum_{j<h} c[j+h] z^j) h'
    R_k = <scal_R, G> + B_k z^h (sum_{j<h} c[j]   z^j) h'

are MSMs over the original G whose scalars, and the two sums, one kernel pass writes (zk_pcs_round_dev, include/zkmi.h).  One MSM
plan over G || H (n + 1 bases) serves the commitments (all n + 1 scalars), every round and the verifier (the first n); c, s and
the MSM scalars stay in HBM.  The verifier's g(X) has s itself as its coefficient vector and <b, g> is a product of log n
factors, so its final test C == <c s, G> + (c b) h' costs one MSM.

Differences from the reference, all deliberate:
  * the generators come from this project's own `hash_to_curve` (transcript.py), so proofs are not interchangeable with it;
  * t' = blinding + alpha t_bar is reduced mod r in the proof (the reference leaves the integer unreduced; both verifiers reduce);
  * `open` / `multi_open` take their randomness as an argument (`random()` draws it) so that a proof can be reproduced;
  * the fixed group order of a multi-opening (base.py).

G1 only, both curves, n = next_power_of_two(max_degree) <= 2^21.
"""

import secrets
import time

from ... import _native as N
from ..._algebra import PointArray
from ...ecc import EllipticCurve
from ...frvec import DevVec, FrOps
from ...subprotocol._generators import GeneratorSet, round_profile
from ...transcript import FiatShamirTranscript, hash_to_curve, hash_to_curve_limbs
from ...utils import next_power_of_two
from .base import MultiOpeningQuery, PolynomialCommitmentScheme

MAX_LOG = N.PCS_MAX_LOG


class IPA(PolynomialCommitmentScheme):
    """IPA(max_degree, curve); `setup(seed=None)` hashes the generators (on the host, about a millisecond per point).  `G` (a
    PointArray of n G1 points) and `H` (one point) may be assigned, which drops the MSM plan and the cached transcript bytes.
    `open(.., profile=True)` runs the two MSMs of a round one after the other and leaves the per-round milliseconds in
    `last_profile` (tools/pcs_bench.py)."""

    def __init__(self, max_degree, group):
        super().__init__(max_degree, group)
        self.name = "IPA-PCS"
        self.n = next_power_of_two(max_degree)
        self.log_n = self.n.bit_length() - 1
        if self.log_n > MAX_LOG:
            raise ValueError(f"the inner-product commitment takes at most 2^{MAX_LOG} coefficients")
        self.E = EllipticCurve(self.group)
        self.order = self.E.order
        self._ops = FrOps(self.order)
        self._gens = GeneratorSet(self.E, (self.n, None))    # G, H and the MSM plan over G || H (n + 1 bases in HBM)
        self.last_profile = None

    # -- generators --
    def _set(self, i, value):
        self._gens.set(i, value)
        self.is_setup = all(part is not None for part in self._gens.parts)

    G = property(lambda self: self._gens.parts[0], lambda self, v: self._set(0, v))
    H = property(lambda self: self._gens.parts[1], lambda self, v: self._set(1, v))

    def setup(self, seed=None):
        seed = seed or self.name.encode()
        self.G = PointArray(self.E.curve_id, 1, hash_to_curve_limbs(seed, b"G", self.E.name, self.n))
        self.H = hash_to_curve(seed, b"H", self.E.name, 1)

    def zero_commitment(self):
        return self.E.curve.PointG1.identity()

    def release(self):
        """free the MSM plan over G || H (it is rebuilt on the next use)"""
        self._gens.release()

    def _blinded(self, polynomial, blinding):
        """DevVec of n + 1 elements: the coefficients, zero padded to n, then the blinding"""
        ops, n = self._ops, self.n
        vec = self._vec(polynomial, n)
        out = DevVec(n + 1)
        if vec.n:
            ops.d_copy(vec.n, vec.ptr(), out.ptr())
        out.upload(ops.one(blinding), n)
        return out

    def _transcript(self, transcript):
        """the caller's transcript, or the default one, with every G_i and then H appended"""
        return self._gens.transcript(transcript, self.name.encode(), self.order)

    # -- randomness --
    def random(self, multi=False):
        """the randomness of one opening as `open(.., randomness=)` takes it: {"poly_r": n coefficients as an (n, 4) limb array,
        exactly uniform below r, "t_bar": int}, and "f_blind" for `multi_open` (multi=True)"""
        out = {"poly_r": self._ops.random_vector(self.n), "t_bar": secrets.randbelow(self.order)}
        if multi:
            out["f_blind"] = secrets.randbelow(self.order)
        return out

    # -- the scheme --
    def commit(self, polynomial, blinding: int):
        assert self.is_setup, "Trusted setup has not been run"
        N.ensure_gpu()
        return self._gens.msm(self._blinded(polynomial, blinding), self.n + 1)

    def open(self, polynomial, point, commitment, blinding, transcript=None, *, randomness=None, profile=False):
        """([L list, R list, C_bar, c, t'], evaluation)"""
        assert self.is_setup, "Trusted setup has not been run"
        N.ensure_gpu()
        ops, n, log_n, r = self._ops, self.n, self.log_n, self.order
        randomness = randomness if randomness is not None else self.random()
        vec = self._vec(polynomial, n)
        evaluation = ops.d_eval(vec.n, vec.ptr(), point) if vec.n else 0

        transcript = self._transcript(transcript)
        transcript.append(point)
        transcript.append(evaluation)
        transcript.append(commitment)

        # a_bar: poly_r with its constant term lowered by poly_r(point), so that it vanishes at the point; then the blinding
        a_bar = self._blinded(randomness["poly_r"], randomness["t_bar"])
        ops.d_add_at(a_bar, 0, -ops.d_eval(n, a_bar.ptr(), point))
        commitment_bar = self._gens.msm(a_bar, n + 1)
        transcript.append(commitment_bar)
        alpha = transcript.get_challenge_scalar()

        c = DevVec(n)                         # c = a + alpha a_bar, folded in place
        if vec.n:
            ops.d_copy(vec.n, vec.ptr(), c.ptr())
        N.check(N.load().zk_vec_axpby_dev(ops.cid, n, N.u64p(ops.one(1)), c.ptr(), N.u64p(ops.one(alpha)), a_bar.ptr(), None, c.ptr(), None))
        t_prime = (blinding + alpha * randomness["t_bar"]) % r

        commitment_prime = self._gens.msm(c, n)
        transcript.append(commitment_prime)
        h_prime = hash_to_curve(transcript.get_challenge(), b"U", self.E.name, 1)
        transcript.append(commitment_prime + h_prime * evaluation)

        L_list, R_list, c_final = self._rounds(c, point % r, h_prime, transcript, profile)
        return [L_list, R_list, commitment_bar, c_final, t_prime], evaluation

    def _rounds(self, c, z, h_prime, transcript, profile=False):
        """the log2(n) rounds over the device vector c (n elements, folded in place): (L list, R list, the final c).  Every L, R is
        appended to `transcript`.  A challenge of 0 has no inverse: ValueError."""
        ops, n, log_n, r = self._ops, self.n, self.log_n, self.order
        s = DevVec(n, zero=False)
        scal_l, scal_r = DevVec(n, zero=False), DevVec(n, zero=False)
        L_list, R_list, rounds = [], [], []
        u = u_inv = None
        b_scale = 1                            # B_k
        for k in range(log_n + 1):
            t0 = time.perf_counter()
            if k == log_n:
                ops.d_pcs_round(log_n, k, c.ptr(), s.ptr(), u, u_inv)
                break
            hi, lo = ops.d_pcs_round(log_n, k, c.ptr(), s.ptr(), u, u_inv, z, scal_l.ptr(), scal_r.ptr())
            t1 = time.perf_counter()
            L, R, msm_ms = self._gens.msm_lr(scal_l, scal_r, n, profile)
            t2 = time.perf_counter()
            z_h = pow(z, n >> (k + 1), r)
            L = L + h_prime * (b_scale * hi % r)
            R = R + h_prime * (b_scale * z_h * lo % r)
            L_list.append(L)
            R_list.append(R)
            transcript.append(L)
            transcript.append(R)
            u = transcript.get_challenge_scalar()
            u_inv = pow(u, -1, r)
            b_scale = b_scale * (1 + u * z_h) % r
            if profile:
                rounds.append(round_profile(k, t0, t1, t2, time.perf_counter(), msm_ms))
        if profile:
            self.last_profile = rounds
        return L_list, R_list, ops.ints(c.download(1, 0))[0]

    def verify(self, commitment, proof, point, evaluation, transcript=None):
        assert self.is_setup, "Trusted setup has not been run"
        if len(proof) != 5:
            return False
        ops, n, log_n, r = self._ops, self.n, self.log_n, self.order
        L_list, R_list, commitment_bar, c, t_prime = proof
        if len(L_list) != log_n or len(R_list) != log_n:
            return False
        if commitment.is_zero() or commitment_bar.is_zero() or t_prime % r == 0 or c % r == 0:
            return False
        if any(L.is_zero() or R.is_zero() for L, R in zip(L_list, R_list)):
            return False
        N.ensure_gpu()

        transcript = self._transcript(transcript)
        transcript.append(point)
        transcript.append(evaluation)
        transcript.append(commitment)
        transcript.append(commitment_bar)
        alpha = transcript.get_challenge_scalar()
        commitment_prime = commitment + commitment_bar * alpha - self.H * (t_prime % r)
        transcript.append(commitment_prime)
        h_prime = hash_to_curve(transcript.get_challenge(), b"U", self.E.name, 1)
        C = commitment_prime + h_prime * (evaluation % r)
        transcript.append(C)

        us = []
        for L, R in zip(L_list, R_list):
            transcript.append(L)
            transcript.append(R)
            u = transcript.get_challenge_scalar()
            us.append(u)
            C = L * pow(u, -1, r) + C + R * u

        # g(X) = prod_i (1 + u_(log_n-1-i) X^(2^i)): its coefficient vector is s, and <b, g> = g(point)
        b, z_pow = 1, point % r
        for i in range(log_n):
            b = b * (1 + us[log_n - 1 - i] * z_pow) % r
            z_pow = z_pow * z_pow % r
        scal = DevVec(n, zero=False)
        ops.d_pcs_verify_scalars(log_n, us, c, scal.ptr())
        return C == self._gens.msm(scal, n) + h_prime * (c * b % r)

    def multi_open(self, points_query: MultiOpeningQuery, transcript: FiatShamirTranscript = None, *, randomness=None):
        """(proof, the verifier's query).  proof = [commitment to f, q_1(x3), .., q_k(x3), opening of the final polynomial at x3]"""
        assert self.is_setup, "Trusted setup has not been run"
        N.ensure_gpu()
        r = self.order
        randomness = randomness if randomness is not None else self.random(multi=True)
        transcript = transcript or FiatShamirTranscript(self.name.encode(), self.order)
        verifier_query, groups, q_vecs, f, size, x1 = self._multi_open_polys(points_query, transcript, self.n)
        f_blind = randomness["f_blind"] % r
        f_commitment = self.commit(f, f_blind)
        transcript.append(f_commitment)
        x3 = transcript.get_challenge_scalar()
        q_x3, x4 = self._multi_open_final(q_vecs, f, size, x3, transcript)

        final_blinding = f_blind
        for g, (members, _) in enumerate(groups):
            blind = sum(pow(x1, j, r) * points_query.blindings[i] for j, i in enumerate(members)) % r
            final_blinding += pow(x4, g + 1, r) * blind
        final_blinding %= r
        final_commitment = self.commit(f, final_blinding)
        opening_proof, _ = self.open(f, x3, final_commitment, final_blinding, transcript, randomness=randomness)
        return [f_commitment] + q_x3 + [opening_proof], verifier_query

    def multi_verify(self, points_query: MultiOpeningQuery, proof: list, transcript: FiatShamirTranscript = None):
        assert self.is_setup, "Trusted setup has not been run"
        assert len(proof) > 2, "Invalid proof"
        transcript = transcript or FiatShamirTranscript(self.name.encode(), self.order)
        front = self._multi_verify_front(points_query, proof, transcript)
        if front is None:
            return False
        final_commitment, x3, final_value, opening_proof = front
        return self.verify(final_commitment, opening_proof, x3, final_value, transcript)
