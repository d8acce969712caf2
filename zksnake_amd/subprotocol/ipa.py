"""
The Bulletproofs inner-product argument with the reference's interface and transcript
(python/zksnake/subprotocol/bulletproofs/ipa.py:6-213): prove knowledge of a, b with commitment = <a, G> + <b, H> and
<a, b> = the claimed product, in log2(n) rounds of two points each.

The reference folds its generators every round (G' = u^-1 G_lo + u G_hi, about 2n two-scalar multiplications over a
proof and new bases for every MSM).  Here G and H are NEVER folded: after k rounds the folded generator is
G^(k)_j = sum_{i = j mod m} s_i G_i with the verifier's s vector, so every L_k, R_k is an MSM over the original G || H with
scalars that one kernel writes (zk_ipa_round_dev, include/zkmi.h).  One MSM plan over the 2n fixed bases serves the
commitment, every round and the verifier; a, b, s and the MSM scalars stay in HBM; per round only the challenge goes to
the device and only the two cross products and L, R come back.

Two differences from the reference, both deliberate:
  * the generators come from this project's own `hash_to_curve` (transcript.py), so proofs are not interchangeable with
    the reference's;
  * when `Q` was given to the constructor, `verify` mirrors `prove`: it uses that Q and does not append the commitment.
    The reference's verify always derives Q from the transcript and therefore rejects its own Q-given proofs.

G1 only, both curves, n <= 2^21 (2n bases fit the largest split-scalar MSM plan).
"""

import time

import numpy as np

from .. import _native as N
from .._algebra import PointArray
from ..ecc import CurvePointSize, EllipticCurve
from ..frvec import DevVec, FrOps
from ..mle import sumcheck_round
from ..transcript import hash_to_curve, hash_to_curve_limbs
from ..utils import next_power_of_two, split_list
from ._generators import GeneratorSet, round_profile

MAX_LOG = 21


class InnerProductProof:

    def __init__(self, a: int, b: int, L: list, R: list):
        self.a = a
        self.b = b
        self.L = L
        self.R = R

    def to_bytes(self) -> bytes:
        s = b""
        for L, R in zip(self.L, self.R):
            s += bytes(L.to_bytes())
            s += bytes(R.to_bytes())
        s += self.a.to_bytes(32, "little")
        s += self.b.to_bytes(32, "little")
        return bytes(s)

    @classmethod
    def from_bytes(cls, s: bytes, crv="BN254"):
        E = EllipticCurve(crv)
        n = CurvePointSize[crv].value
        assert (len(s) - 64) % n == 0, "Invalid proof length"
        field_s = split_list(s[-64:], 32)
        s = split_list(s[:-64], n)
        Ls, Rs = [], []
        for i in range(0, len(s), 2):
            Ls.append(E.from_hex(s[i].hex()))
            Rs.append(E.from_hex(s[i + 1].hex()))
        return InnerProductProof(int.from_bytes(field_s[0], "little"), int.from_bytes(field_s[1], "little"), Ls, Rs)


class InnerProductArgument:
    """InnerProductArgument(size, curve, seed=b"InnerProductProof", Q=None): vectors of next_power_of_two(size) elements.

    `G`, `H` are PointArrays of n G1 points, hashed from `seed` (on the host, about a millisecond per point) unless
    `generators=(G, H)` hands them in; they may be assigned (a PointArray or a list of n points), which drops the MSM plan and
    the cached transcript bytes.  `prove(.., profile=True)` runs the two MSMs of a round one after the other instead of side
    by side and leaves the per-round milliseconds in `last_profile` (tools/ipa_bench.py)."""

    def __init__(self, size, curve, seed=b"InnerProductProof", Q=None, *, generators=None):
        self.n = next_power_of_two(size)
        self.log_n = self.n.bit_length() - 1
        if self.log_n > MAX_LOG:
            raise ValueError(f"the inner-product argument takes at most 2^{MAX_LOG} elements")
        self.E = EllipticCurve(curve)
        self._ops = FrOps(self.E.order)
        self._gens = GeneratorSet(self.E, (self.n, self.n))    # G, H and the MSM plan over G || H (2n bases in HBM)
        if generators is not None:
            self.G, self.H = generators
        else:
            self.G = PointArray(self.E.curve_id, 1, hash_to_curve_limbs(seed, b"G", curve, self.n))
            self.H = PointArray(self.E.curve_id, 1, hash_to_curve_limbs(seed, b"H", curve, self.n))
        self.Q = Q
        self.last_profile = None

    G = property(lambda self: self._gens.parts[0], lambda self, v: self._gens.set(0, v))
    H = property(lambda self: self._gens.parts[1], lambda self, v: self._gens.set(1, v))

    def _transcript(self, transcript):
        """the caller's transcript, or the default one, with every G_i and then every H_i appended"""
        return self._gens.transcript(transcript, self.n.to_bytes(32, "big"), self.E.order)

    def prove(self, a, b, transcript=None, profile=False):
        """(InnerProductProof, commitment, <a, b>).  a, b: lists of ints, (k, 4) limb arrays or DevVecs of at most n elements
        (zero padded); device vectors of the caller are not modified."""
        N.ensure_gpu()
        lib, ops, n, log_n, r = N.load(), self._ops, self.n, self.log_n, self.E.order
        transcript = self._transcript(transcript)

        ab_vec = DevVec(2 * n)                       # a || b: the commitment's scalars, then folded in place
        ops.d_load(ab_vec, 0, a, n)
        ops.d_load(ab_vec, n, b, n)
        ab = sum(sumcheck_round(ops, log_n, [ab_vec.ptr(0), ab_vec.ptr(n)], [(1, (0, 1))])[:2 if log_n else 1]) % r
        commitment = self._gens.msm(ab_vec, 2 * n)
        if self.Q is not None:
            Q = self.Q
        else:
            transcript.append(commitment)
            Q = hash_to_curve(transcript.get_challenge(), b"Q", self.E.name)

        L_list, R_list, a_final, b_final = self._rounds(ab_vec, Q, transcript, profile=profile)
        return InnerProductProof(a_final, b_final, L_list, R_list), commitment, ab

    def _rounds(self, ab_vec, Q, transcript, h_weight=None, profile=False):
        """The log2(n) rounds over the device vector a || b (2n elements, folded in place): (L list, R list, a, b).  Every L, R is
        appended to `transcript`.  h_weight (a DevVec of n elements, or None) starts s_inv at h_weight[i] instead of 1, so that
        the argument runs over H'_i = h_weight[i] H_i with the plan over the original H (zk_ipa_round_seeded_dev): a range
        proof's y^-i.  A challenge of 0 has no inverse: ValueError."""
        lib, ops, n, log_n, r = N.load(), self._ops, self.n, self.log_n, self.E.order
        a_ptr, b_ptr = ab_vec.ptr(0), ab_vec.ptr(n)
        s, s_inv = DevVec(n, zero=False), DevVec(n, zero=False)
        scal_l, scal_r = DevVec(2 * n, zero=False), DevVec(2 * n, zero=False)
        cross = np.zeros((2, 4), dtype=np.uint64)
        L_list, R_list, rounds = [], [], []
        u = u_inv = None
        for k in range(log_n + 1):
            t0 = time.perf_counter()
            last = k == log_n
            N.check(lib.zk_ipa_round_seeded_dev(ops.cid, log_n, k, a_ptr, b_ptr, s.ptr(), s_inv.ptr(),
                                                h_weight.ptr() if h_weight is not None and k == 0 else None,
                                                None if u is None else N.u64p(u), None if u is None else N.u64p(u_inv),
                                                None if last else scal_l.ptr(), None if last else scal_r.ptr(),
                                                None if last else N.u64p(cross), None))
            if last:
                break
            t1 = time.perf_counter()
            L, R, msm_ms = self._gens.msm_lr(scal_l, scal_r, 2 * n, profile)
            t2 = time.perf_counter()
            c = ops.ints(cross)
            L = L + Q * c[0]
            R = R + Q * c[1]
            L_list.append(L)
            R_list.append(R)
            transcript.append(L)
            transcript.append(R)
            challenge = transcript.get_challenge_scalar()
            u, u_inv = ops.one(challenge), ops.one(pow(challenge, -1, r))
            if profile:
                rounds.append(round_profile(k, t0, t1, t2, time.perf_counter(), msm_ms))
        final = ops.ints(ab_vec.download(1, 0)) + ops.ints(ab_vec.download(1, n))
        if profile:
            self.last_profile = rounds
        return L_list, R_list, final[0], final[1]

    def verify(self, proof: InnerProductProof, commitment, inner_product_result, transcript=None):
        assert len(proof.L) < 32, "Argument size is too big"
        if len(proof.L) != self.log_n or len(proof.R) != self.log_n:
            return False
        N.ensure_gpu()
        lib, ops, n, log_n, r = N.load(), self._ops, self.n, self.log_n, self.E.order
        transcript = self._transcript(transcript)
        if self.Q is not None:
            Q = self.Q
        else:
            transcript.append(commitment)
            Q = hash_to_curve(transcript.get_challenge(), b"Q", self.E.name)

        us, sum_LR = [], self.E.curve.PointG1.identity()
        for L, R in zip(proof.L, proof.R):
            transcript.append(L)
            transcript.append(R)
            u = transcript.get_challenge_scalar()
            us.append(u)
            sum_LR = sum_LR + L * pow(u, 2, r) + R * pow(u, -2, r)

        scal = DevVec(2 * n, zero=False)
        u_l = ops.limbs(us) if us else None
        ui_l = ops.limbs([pow(u, -1, r) for u in us]) if us else None
        N.check(lib.zk_ipa_verify_scalars_dev(ops.cid, log_n, None if u_l is None else N.u64p(u_l), None if ui_l is None else N.u64p(ui_l),
                                              N.u64p(ops.one(proof.a)), N.u64p(ops.one(proof.b)), scal.ptr(), None))
        lhs = commitment + Q * (inner_product_result % r)
        rhs = self._gens.msm(scal, 2 * n) + Q * (proof.a * proof.b % r) - sum_LR
        return lhs == rhs

    def release(self):
        """free the MSM plan over G || H (it is rebuilt on the next use)"""
        self._gens.release()


__all__ = ["InnerProductArgument", "InnerProductProof"]
