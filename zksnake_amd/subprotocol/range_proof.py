"""
Bulletproofs range proofs with the reference's interface (python/zksnake/subprotocol/bulletproofs/range_proof.py:8-317):
prove that a committed value lies in [0, 2^bitsize) -- and, beyond the reference, that each of `values` committed values
does, in ONE argument over N = bitsize * values positions (the standard aggregation: value j is weighted by z^(2+j) where a
single proof has z^2).  With values = 1 the protocol is the reference's, equation for equation.

All scalar-side work is four kernels (csrc/rangeproof.hip, include/zkmi.h): the bit vectors a_L || a_R, the coefficients
t0, t1, t2 of t(X) in one pass, l || r at the challenge x, and the verifier's 2N scalars.  The inner-product argument is the
one of ipa.py, over the same MSM plan on G || H that serves A, S, every round and the verifier.  The reference runs that
argument over H'_k = y^-k H_k; here H' IS NEVER FORMED: after k rounds the folded H-side generator is
sum_{i = j mod m} s_i^-1 y^-i H_i, so the argument's s_inv vector starts at y^-i instead of 1 (zk_ipa_round_seeded_dev) and
every later round and the verifier's H scalars carry the weight by themselves.

Differences from the reference, all deliberate:
  * GENERATORS IN THE TRANSCRIPT.  After w the reference appends every G_k and every H'_k: N scalar multiplications and
    64 N bytes of blake2b per prove and per verify.  Here the transcript takes ONE 64-byte item instead,
    blake2b(G bytes || H bytes) over the unscaled generators, computed once per object and dropped when G or H is assigned.
    H' is a function of H and of y, which the transcript already holds, so nothing is left unbound.
  * `verify` DOES NOT CALL `transcript.reset()`: it mirrors `prove`, so a caller's transcript that is already in use works
    (the reference's reset makes it fail).
  * `bitsize` is a power of two, 1 <= bitsize <= 128, and `values` is a power of two with bitsize * values <= 2^21 (the
    inner-product argument's limit); anything else is a ValueError.  The reference accepts any bitsize below 2^32, but its
    own inner-product argument only works for powers of two, and 2^i must stay a plain integer below r.
  * the generators come from this project's `hash_to_curve` (transcript.py), as for the inner-product argument, so proofs are
    not interchangeable with the reference's.

What stays the reference's: only bits below `bitsize` are read from v and V commits to v mod r, so `prove(500)` at bitsize 8
returns a proof that `verify` rejects (it does not raise); a transcript that yields y = 0, z in {0, 1} or a round challenge
u = 0 makes `prove` raise ValueError and `verify` return False.

Transcript: label bitsize.to_bytes(32, "big") (followed by values.to_bytes(32, "big") when values > 1); V_0 .. V_(m-1), A, S
-> y, z; T1, T2 -> x; t, t_blinding, e_blinding -> w; the generator digest; L_t, R_t per round -> u_t.  Q = w B is given to the
argument, so no commitment is appended and no commitment MSM is run.
"""

import hashlib
import secrets
import time

import numpy as np

from .. import _native as N
from .._algebra import PointArray
from ..ecc import CurvePointSize, EllipticCurve
from ..frvec import DevVec
from ..transcript import FiatShamirTranscript, hash_to_curve, hash_to_curve_limbs
from ..utils import split_list
from .ipa import MAX_LOG, InnerProductArgument, InnerProductProof

MAX_BITSIZE = 128
BATCH_MIN = 64      # from this many values on, the V_j and their sum in the verifier go through batch_mul / multiexp
RANDOMNESS_KEYS = ("s_L", "s_R", "a_blinding", "s_blinding", "v_blinding", "t1_blinding", "t2_blinding")


class RangeProofObject:

    def __init__(self, V, A, S, T1, T2, t, t_blinding, e_blinding, ipa_proof: InnerProductProof):
        self.V = V          # a point, or a list of m points for an aggregated proof
        self.A = A
        self.S = S
        self.T1 = T1
        self.T2 = T2
        self.t = t
        self.t_blinding = t_blinding
        self.e_blinding = e_blinding
        self.ipa_proof = ipa_proof

    def _commitments(self):
        return list(self.V) if isinstance(self.V, (list, tuple)) else [self.V]

    def to_bytes(self) -> bytes:
        s = b""
        for p in self._commitments() + [self.A, self.S, self.T1, self.T2]:
            s += bytes(p.to_bytes())
        s += self.t.to_bytes(32, "little")
        s += self.t_blinding.to_bytes(32, "little")
        s += self.e_blinding.to_bytes(32, "little")
        s += self.ipa_proof.to_bytes()
        return s

    @classmethod
    def from_bytes(cls, s: bytes, crv="BN254", values=1):
        E = EllipticCurve(crv)
        n = CurvePointSize[crv].value
        k = values + 4

        assert (len(s) - 160) % n == 0, "Invalid proof length"

        point_s = split_list(s[: k * n], n)
        field_s = split_list(s[k * n: k * n + 32 * 3], 32)
        ipa_s = s[k * n + 32 * 3:]

        assert len(point_s) == k and len(field_s) == 3, "Malformed proof structure"

        points = [E.from_hex(p.hex()) for p in point_s]
        V = points[0] if values == 1 else points[:values]
        A, S, T1, T2 = points[values:]
        t, t_blinding, e_blinding = (int.from_bytes(f, "little") for f in field_s)
        ipa_proof = InnerProductProof.from_bytes(ipa_s, crv)

        return RangeProofObject(V, A, S, T1, T2, t, t_blinding, e_blinding, ipa_proof)


class RangeProof:
    """RangeProof(bitsize, curve, seed=b"RangeProof", *, values=1, generators=None).

    `G`, `H` are PointArrays of N = bitsize * values G1 points and `B`, `B_blinding` single points, hashed from `seed` with the
    reference's tags (on the host, about a millisecond per point) unless `generators=(G, H)` hands G and H in.  All four may be
    assigned; assigning G or H drops the MSM plan and the generator digest.  The object owns one InnerProductArgument over
    (G, H) and uses its plan, the clone for MSM pairs, and `release()`."""

    def __init__(self, bitsize, curve, seed=b"RangeProof", *, values=1, generators=None):
        for what, x in (("bitsize", bitsize), ("values", values)):
            if not isinstance(x, int) or isinstance(x, bool) or x < 1 or x & (x - 1):
                raise ValueError(f"{what} must be a power of two")
        if bitsize > MAX_BITSIZE:
            raise ValueError(f"bitsize is at most {MAX_BITSIZE}")
        if bitsize * values > 1 << MAX_LOG:
            raise ValueError(f"bitsize * values is at most 2^{MAX_LOG}")
        self.n, self.m = bitsize, values
        self.E = EllipticCurve(curve)
        size = bitsize * values
        self._log_bits, self._log_size = bitsize.bit_length() - 1, size.bit_length() - 1
        if generators is None:
            cid = self.E.curve_id
            generators = (PointArray(cid, 1, hash_to_curve_limbs(seed, b"G", curve, size)),
                          PointArray(cid, 1, hash_to_curve_limbs(seed, b"H", curve, size)))
        self._ipa = InnerProductArgument(size, curve, generators=generators)
        self._ops = self._ipa._ops
        self._digest = None
        self.B = hash_to_curve(seed, b"B", curve, 1)
        self.B_blinding = hash_to_curve(seed, b"Blinding", curve, 1)
        self.last_profile = None

    # -- generators --
    def _set(self, name, points):
        setattr(self._ipa, name, points)
        self._digest = None

    G = property(lambda self: self._ipa.G, lambda self, v: self._set("G", v))
    H = property(lambda self: self._ipa.H, lambda self, v: self._set("H", v))

    def _generator_digest(self):
        """the one transcript item that binds the generators: blake2b over every G_k and then every H_k, unscaled"""
        if self._digest is None:
            self._digest = hashlib.blake2b(self.G.to_bytes() + self.H.to_bytes()).digest()
        return self._digest

    def release(self):
        """free the MSM plan over G || H (it is rebuilt on the next use)"""
        self._ipa.release()

    def _transcript(self, transcript):
        if transcript is not None:
            return transcript
        label = self.n.to_bytes(32, "big") + (self.m.to_bytes(32, "big") if self.m > 1 else b"")
        return FiatShamirTranscript(label, field=self.E.order)

    # -- randomness --
    def random_vector(self, count):
        """`count` scalars, exactly uniform below r, from the OS CSPRNG, as a (count, 4) limb array (FrOps.random_vector)"""
        return self._ops.random_vector(count)

    def random(self):
        """the randomness of one proof, as `prove(.., randomness=)` takes it"""
        r, size = self.E.order, self.n * self.m
        blind = lambda: secrets.randbelow(r)  # noqa: E731
        return {"s_L": self.random_vector(size), "s_R": self.random_vector(size), "a_blinding": blind(), "s_blinding": blind(),
                "v_blinding": [blind() for _ in range(self.m)], "t1_blinding": blind(), "t2_blinding": blind()}

    # -- helpers --
    def _values(self, v):
        if isinstance(v, int):
            v = [v]
        v = list(v)
        if len(v) != self.m:
            raise ValueError(f"{self.m} value(s) expected, got {len(v)}")
        return v

    def _upload_values(self, values):
        """m x 2 64-bit limbs in HBM: the low 128 bits of each value"""
        mask = (1 << 128) - 1
        limbs = N.ints_to_limbs([x & mask for x in values], 2)
        vec = DevVec((self.m + 1) // 2, zero=False)
        vec.buf.upload(limbs)
        return vec

    def _commit_values(self, values, gamma):
        """V_j = v_j B + gamma_j B~"""
        r = self.E.order
        if self.m < BATCH_MIN:
            return [self.B * (x % r) + self.B_blinding * g for x, g in zip(values, gamma)]
        vb = self.E.batch_mul(self.B, [x % r for x in values])
        gb = self.E.batch_mul(self.B_blinding, gamma)
        return [p + q for p, q in zip(vb, gb)]

    def _weights(self, z):
        """z^(2+j) for j < m"""
        r, out, w = self.E.order, [], z * z % self.E.order
        for _ in range(self.m):
            out.append(w)
            w = w * z % r
        return out

    def _delta(self, y, z):
        """(z - z^2) sum_{k<N} y^k - (sum_{j<m} z^(3+j)) (2^n - 1), the two series by their closed forms"""
        r, size, m = self.E.order, self.n * self.m, self.m
        sum_y = size % r if y == 1 else (pow(y, size, r) - 1) * pow(y - 1, -1, r) % r
        sum_z = m * pow(z, 3, r) % r if z == 1 else pow(z, 3, r) * (pow(z, m, r) - 1) * pow(z - 1, -1, r) % r
        return ((z - z * z) * sum_y - sum_z * ((1 << self.n) - 1)) % r

    def prove(self, v, transcript=None, *, randomness=None, profile=False):
        """RangeProofObject for v: an int (values = 1) or a sequence of `values` ints.  `randomness`: a mapping with the keys
        s_L, s_R (lists of ints, (N, 4) limb arrays or DevVecs of N elements; the caller's are not modified), a_blinding,
        s_blinding, t1_blinding, t2_blinding (ints) and v_blinding (an int or `values` ints); by default everything is drawn
        from the OS CSPRNG.  `profile=True` leaves the milliseconds of each part in `last_profile` (tools/range_proof_bench.py)."""
        N.ensure_gpu()
        lib, ops, r, ipa = N.load(), self._ops, self.E.order, self._ipa
        size, m, lb, ln = self.n * self.m, self.m, self._log_bits, self._log_size
        clock = time.perf_counter
        t_start = clock()
        values = self._values(v)
        rnd = randomness if randomness is not None else self.random()
        t_random = clock()
        missing = [k for k in RANDOMNESS_KEYS if k not in rnd]
        if missing:
            raise ValueError(f"randomness lacks {missing}")
        gamma = rnd["v_blinding"]
        gamma = [gamma % r] if isinstance(gamma, int) else [g % r for g in gamma]
        if len(gamma) != m:
            raise ValueError(f"{m} blinding factor(s) of V expected, got {len(gamma)}")
        alpha, rho, tau1, tau2 = (rnd[k] % r for k in ("a_blinding", "s_blinding", "t1_blinding", "t2_blinding"))
        transcript = self._transcript(transcript)

        d_values = self._upload_values(values)
        s_vec = DevVec(2 * size, zero=False)      # s_L || s_R: the scalars of S
        for offset, key in ((0, "s_L"), (size, "s_R")):
            given = rnd[key]
            if (given.n if isinstance(given, DevVec) else len(given)) != size:
                raise ValueError(f"{key} must have {size} elements")
            ops.d_load(s_vec, offset, given, size)
        bits_vec = DevVec(2 * size, zero=False)   # a_L || a_R: the scalars of A
        if profile:
            N.check(lib.zk_dev_synchronize())
        t_upload = clock()
        N.check(lib.zk_rp_bits_dev(ops.cid, lb, ln, d_values.ptr(), bits_vec.ptr(), None))
        if profile:
            N.check(lib.zk_dev_synchronize())
        t_load = clock()
        V = self._commit_values(values, gamma)
        t_commit = clock()
        A, S, _ = ipa._gens.msm_lr(bits_vec, s_vec, 2 * size)
        A = A + self.B_blinding * alpha
        S = S + self.B_blinding * rho
        t_pair = clock()
        for p in V:
            transcript.append(p)
        transcript.append(A)
        transcript.append(S)
        y = transcript.get_challenge_scalar()
        z = transcript.get_challenge_scalar()
        if z in (0, 1):
            raise ValueError("the transcript gave z in {0, 1}")
        y_inv = pow(y, -1, r)       # ValueError for y = 0

        t_host = clock()
        coeffs = np.zeros((3, 4), dtype=np.uint64)
        N.check(lib.zk_rp_poly_dev(ops.cid, lb, ln, d_values.ptr(), s_vec.ptr(), N.u64p(ops.one(y)), N.u64p(ops.one(z)), N.u64p(coeffs),
                                   None))
        t0, t1, t2 = ops.ints(coeffs)
        t_poly = clock()
        T1 = self.B * t1 + self.B_blinding * tau1
        T2 = self.B * t2 + self.B_blinding * tau2
        transcript.append(T1)
        transcript.append(T2)
        x = transcript.get_challenge_scalar()
        t = (t0 + t1 * x + t2 * x * x) % r
        t_blinding = (sum(w * g for w, g in zip(self._weights(z), gamma)) + tau1 * x + tau2 * x * x) % r
        e_blinding = (alpha + x * rho) % r
        transcript.append(t)
        transcript.append(t_blinding)
        transcript.append(e_blinding)
        w = transcript.get_challenge_scalar()
        Q = self.B * w
        transcript.append(self._generator_digest())

        t_host2 = clock()
        lr_vec = bits_vec                          # l || r overwrite a_L || a_R, which A has consumed
        h_weight = DevVec(size, zero=False)
        N.check(lib.zk_rp_eval_dev(ops.cid, lb, ln, d_values.ptr(), s_vec.ptr(), N.u64p(ops.one(y)), N.u64p(ops.one(y_inv)),
                                   N.u64p(ops.one(z)), N.u64p(ops.one(x)), lr_vec.ptr(), h_weight.ptr(), None))
        if profile:
            N.check(lib.zk_dev_synchronize())
        t_eval = clock()
        L_list, R_list, a, b = ipa._rounds(lr_vec, Q, transcript, h_weight=h_weight, profile=profile)
        t_rounds = clock()
        if profile:
            ms = lambda begin, end: (end - begin) * 1e3  # noqa: E731
            self.last_profile = {"random_ms": ms(t_start, t_random), "upload_ms": ms(t_random, t_upload), "bits_kernel_ms": ms(t_upload, t_load), "commit_v_ms": ms(t_load, t_commit),
                                 "msm_pair_ms": ms(t_commit, t_pair), "poly_kernel_ms": ms(t_host, t_poly),
                                 "eval_kernel_ms": ms(t_host2, t_eval), "rounds_ms": ms(t_eval, t_rounds),
                                 "host_ms": ms(t_pair, t_host) + ms(t_poly, t_host2), "rounds": ipa.last_profile}
        return RangeProofObject(V[0] if m == 1 else V, A, S, T1, T2, t, t_blinding, e_blinding, InnerProductProof(a, b, L_list, R_list))

    def verify(self, proof: RangeProofObject, transcript=None, *, c=None):
        """True when the proof's V (a point, or `values` points) commit to values below 2^bitsize.  One check with a random c
        (given for tests): the MSM plan runs once over the 2N scalars of zk_rp_verify_scalars_dev, the V_j term is a multiexp
        when there are many, and the remaining 6 + 2 log2(N) terms are computed on the host."""
        N.ensure_gpu()
        lib, ops, r, ipa = N.load(), self._ops, self.E.order, self._ipa
        size, m, lb, ln = self.n * self.m, self.m, self._log_bits, self._log_size
        V = proof._commitments()
        ip = proof.ipa_proof
        if len(V) != m or len(ip.L) != ln or len(ip.R) != ln:
            return False
        transcript = self._transcript(transcript)
        for p in V:
            transcript.append(p)
        transcript.append(proof.A)
        transcript.append(proof.S)
        y = transcript.get_challenge_scalar()
        z = transcript.get_challenge_scalar()
        transcript.append(proof.T1)
        transcript.append(proof.T2)
        x = transcript.get_challenge_scalar()
        transcript.append(proof.t)
        transcript.append(proof.t_blinding)
        transcript.append(proof.e_blinding)
        w = transcript.get_challenge_scalar()
        transcript.append(self._generator_digest())
        us = []
        for L, R in zip(ip.L, ip.R):
            transcript.append(L)
            transcript.append(R)
            us.append(transcript.get_challenge_scalar())
        if y == 0 or z in (0, 1) or 0 in us:
            return False
        if c is None:
            c = secrets.randbelow(r)
        c %= r

        scal = DevVec(2 * size, zero=False)
        u_l = ops.limbs(us) if us else None
        ui_l = ops.limbs([pow(u, -1, r) for u in us]) if us else None
        N.check(lib.zk_rp_verify_scalars_dev(ops.cid, lb, ln, None if u_l is None else N.u64p(u_l), None if ui_l is None else N.u64p(ui_l),
                                             N.u64p(ops.one(ip.a)), N.u64p(ops.one(ip.b)), N.u64p(ops.one(pow(y, -1, r))), N.u64p(ops.one(z)),
                                             scal.ptr(), None))
        check = ipa._gens.msm(scal, 2 * size)
        v_scalars = [c * wj % r for wj in self._weights(z)]
        if m < BATCH_MIN:
            for p, s in zip(V, v_scalars):
                check = check + p * s
        else:
            check = check + self.E.multiexp(V, v_scalars)
        a, b = ip.a % r, ip.b % r
        check = check + proof.A + proof.S * x + proof.T1 * (c * x % r) + proof.T2 * (c * x * x % r)
        check = check + self.B * ((w * (proof.t - a * b) + c * (self._delta(y, z) - proof.t)) % r)
        check = check + self.B_blinding * ((-proof.e_blinding - c * proof.t_blinding) % r)
        for L, R, u in zip(ip.L, ip.R, us):
            check = check + L * pow(u, 2, r) + R * pow(u, -2, r)
        return check.is_zero()


__all__ = ["RangeProof", "RangeProofObject"]
