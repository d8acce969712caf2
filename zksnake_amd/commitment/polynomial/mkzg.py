"""
Multilinear KZG commitments (PST13, the scheme of arkworks' `MultilinearPC`) over the dense tables of `zksnake_amd.mle`: commit
to a multilinear polynomial and prove its value at a point, which is what a sumcheck or GKR proof ends in.  The reference has no
multilinear commitment, so there is nothing to interchange with; tests/mlpcs_model.py is the specification.

Conventions are those of mle.py: a polynomial in m variables is its table of 2^m evaluations, variable 0 is the least significant
bit of the index, `point[i]` goes to variable i, scalars are reduced mod r on entry.

With n = num_vars and the trapdoor tau = (tau_0 .. tau_(n-1)) the SRS holds, for every level k = 0 .. n, the 2^(n-k) points
eq(tau_k .. tau_(n-1); b) G1 (level n is G1 alone) and in G2 the points tau_k G2.  Level k is the Lagrange basis of a polynomial
in the LAST n - k variables, so a polynomial of m <= n variables lives on levels n - m and above:
    commit   C   = <f, level_(n-m)>                                           one MSM
    open     Q_k = <q_k, level_(n-m+k+1)>,  k < m                             one kernel chain (csrc/mlpcs.hip), then m MSMs
             q_k[b] = f_k[2b+1] - f_k[2b],  f_(k+1)[b] = f_k[2b] + z_k q_k[b],  f_0 = f,  f(z) = f_m[0]
    verify   e(f(z) G1 - C, G2) * prod_k e(Q_k, tau_(n-m+k) G2 - z_k G2) == 1  ONE multi-pairing on the host
Every level is a `PointArray` with its own lazily created MSM plan.  The quotients of all levels stay in one device buffer; each
level's MSM reads its slice of that buffer in place.  NO ZERO-KNOWLEDGE BLINDING: a commitment and a proof are deterministic in
the polynomial.
"""

import numpy as np

from ... import _native as N
from ...ecc import EllipticCurve
from ...frvec import DevVec, FrOps
from ...mle import MultilinearPolynomial
from ...transcript import FiatShamirTranscript
from ...utils import get_random_int

MAX_VARS = N.MLPCS_MAX_LOG   # all levels together hold 2^(num_vars + 1) points
TILE_LOG = N.MLE_TILE_LOG


class MultilinearKZG:
    """MultilinearKZG(num_vars, curve): commitments in G1, both curves.  `setup(tau=None)` draws the num_vars trapdoor scalars
    unless a list is given.  A polynomial is a `MultilinearPolynomial` of the scheme's field (its resident table is used as it
    is), a list of 2^m ints, a (2^m, 4) limb array or a `DevVec` of 2^m elements, m <= num_vars."""

    def __init__(self, num_vars, curve):
        num_vars = int(num_vars)
        if num_vars < 0 or num_vars > MAX_VARS:
            raise ValueError(f"num_vars must be in 0 .. {MAX_VARS}")
        self.name = "MultilinearKZG"
        self.num_vars = num_vars
        self.group = curve
        self.E = EllipticCurve(curve)
        self.order = self.E.order
        self._ops = FrOps(self.order)
        self._levels = None    # level k: PointArray of 2^(num_vars - k) points
        self.G2_tau = None     # [tau_k G2]
        self.is_setup = False

    # -- the SRS --
    def setup(self, tau=None):
        lib = N.ensure_gpu()
        n, r, ops = self.num_vars, self.order, self._ops
        tau = [get_random_int(r) for _ in range(n)] if tau is None else [int(t) % r for t in tau]
        if len(tau) != n:
            raise ValueError(f"{n} trapdoor scalars expected, got {len(tau)}")
        self.release()
        levels = []
        for k in range(n + 1):
            eq = DevVec(1 << (n - k), zero=False)
            N.check(lib.zk_gkr_eq_table_dev(ops.cid, n - k, N.u64p(ops.limbs(tau[k:])) if k < n else None, eq.ptr(), None))
            levels.append(self.E.batch_mul(self.E.G1(), eq.download(), as_array=True))
        self._levels = levels
        self.G2_tau = [self.E.G2() * t for t in tau]
        self.is_setup = True

    def release(self):
        """free every level's MSM plan and drop the SRS"""
        for level in self._levels or ():
            level.release()
        self._levels = None
        self.G2_tau = None
        self.is_setup = False

    def _need_setup(self):
        if not self.is_setup:
            raise RuntimeError("Trusted setup has not been run")

    # -- inputs --
    def _shape(self, poly):
        """(number of entries, m) of a polynomial, checked before anything moves to the device"""
        if isinstance(poly, MultilinearPolynomial):
            if poly.p != self.order:
                raise TypeError("the polynomial is over another field than the scheme")
            count = len(poly)
        elif isinstance(poly, DevVec):
            count = poly.n
        elif isinstance(poly, np.ndarray):
            count = self._ops.limbs(poly).shape[0]
        elif isinstance(poly, (list, tuple)):
            count = len(poly)
        else:
            raise TypeError("a polynomial is a MultilinearPolynomial, a list of ints, a (2^m, 4) limb array or a DevVec")
        if count == 0 or count & (count - 1):
            raise ValueError("the number of evaluations must be a power of two")
        m = count.bit_length() - 1
        if m > self.num_vars:
            raise ValueError(f"the polynomial has {m} variables, the scheme takes at most {self.num_vars}")
        return count, m

    def _table(self, poly, count):
        """(device address, what keeps it alive) of a polynomial's table: resident tables as they are, host values uploaded"""
        if isinstance(poly, MultilinearPolynomial):
            return poly.device_ptr(), poly
        if isinstance(poly, DevVec):
            return poly.ptr(), poly
        vec = self._ops.d_from(self._ops.limbs(poly))      # ints are reduced here, limb arrays on the device
        if isinstance(poly, np.ndarray):
            N.check(N.load().zk_vec_canon_dev(self._ops.cid, count, vec.ptr(), None))
        return vec.ptr(), vec

    def _point(self, point, m):
        point = [int(z) % self.order for z in point]
        if len(point) != m:
            raise ValueError(f"the point has {len(point)} coordinates, the polynomial {m} variables")
        return point

    # -- commit / open / verify --
    def zero_commitment(self):
        return self.E.curve.PointG1.identity()

    def _commit(self, ptr, m):
        return self._levels[self.num_vars - m].msm(ptr, 1 << m)

    def commit(self, poly):
        self._need_setup()
        count, m = self._shape(poly)
        N.ensure_gpu()
        ptr, _keep = self._table(poly, count)
        return self._commit(ptr, m)

    def _quotients(self, ptr, m, point):
        """the quotient chain of the table at `ptr`: (DevVec of 2^m - 1 entries, level 0 first; the evaluation)"""
        quotients = DevVec(max((1 << m) - 1, 1), zero=False)
        work = DevVec(1 << (max(m - TILE_LOG, 0) + 1), zero=False)
        out = np.zeros(4, dtype=np.uint64)
        z = self._ops.limbs(point) if m else None
        N.check(N.load().zk_mlpcs_quotients_dev(self._ops.cid, m, ptr, None if z is None else N.u64p(z), quotients.ptr(), N.u64p(out),
                                                 work.ptr(), None))
        return quotients, int.from_bytes(out.tobytes(), "little")

    def _open(self, ptr, m, point):
        quotients, evaluation = self._quotients(ptr, m, point)
        first = self.num_vars - m + 1
        proof = [self._levels[first + k].msm(quotients.ptr((1 << m) - (1 << (m - k))), 1 << (m - 1 - k))
                 for k in range(m)]
        return proof, evaluation

    def open(self, poly, point):
        """([Q_0 .. Q_(m-1)], the evaluation at `point`)"""
        self._need_setup()
        count, m = self._shape(poly)
        point = self._point(point, m)
        N.ensure_gpu()
        ptr, _keep = self._table(poly, count)
        return self._open(ptr, m, point)

    def verify(self, commitment, proof, point, evaluation, transcript=None):
        """needs `G2_tau` only: a verifier may assign that list and never run `setup`"""
        if self.G2_tau is None or len(self.G2_tau) != self.num_vars:
            raise RuntimeError("Trusted setup has not been run")
        G1, G2, r = self.E.curve.PointG1, self.E.G2(), self.order
        point = list(point)
        m = len(point)
        if m > self.num_vars or not isinstance(proof, (list, tuple)) or len(proof) != m:
            return False
        if not isinstance(commitment, G1) or any(not isinstance(q, G1) for q in proof):
            return False
        first = self.num_vars - m
        g1 = [self.E.G1() * (int(evaluation) % r) - commitment] + list(proof)
        g2 = [G2] + [self.G2_tau[first + k] - G2 * (int(z) % r) for k, z in enumerate(point)]
        return self.E.multi_pairing(g1, g2).is_one()

    # -- several polynomials at one point --
    def _challenge(self, transcript, commitments, point, evaluations):
        transcript = transcript or FiatShamirTranscript(self.name.encode(), self.order)
        transcript.append(list(commitments))
        if point:                       # a transcript takes no empty list
            transcript.append([int(z) % self.order for z in point])
        transcript.append([int(v) % self.order for v in evaluations])
        return transcript.get_challenge_scalar()

    def batch_open(self, polys, point, transcript=None, commitments=None):
        """(proof, [evaluations]) for polynomials of the same number of variables at one point: the transcript takes the
        commitments (computed here unless given), the point and the evaluations and yields rho; the proof is the opening of
        sum_i rho^i f_i."""
        self._need_setup()
        polys = list(polys)
        shapes = [self._shape(p) for p in polys]
        if not shapes:
            raise ValueError("no polynomial to open")
        count, m = shapes[0]
        if any(s != shapes[0] for s in shapes):
            raise ValueError("the polynomials of a batch have the same number of variables")
        point = self._point(point, m)
        if commitments is not None and len(commitments) != len(polys):
            raise ValueError("one commitment per polynomial")
        N.ensure_gpu()
        tables = [self._table(p, count) for p in polys]
        if commitments is None:
            commitments = [self._commit(t[0], m) for t in tables]
        ops, lib = self._ops, N.load()
        work = DevVec(1 << (max(m - TILE_LOG, 0) + 1), zero=False)
        z = ops.limbs(point) if m else np.zeros((1, 4), dtype=np.uint64)
        evaluations = []
        for ptr, _keep in tables:
            out = np.zeros(4, dtype=np.uint64)
            N.check(lib.zk_mle_eval_dev(ops.cid, m, ptr, N.u64p(z), N.u64p(out), work.ptr(), None))
            evaluations.append(int.from_bytes(out.tobytes(), "little"))
        rho = self._challenge(transcript, commitments, point, evaluations)
        combined = DevVec(1 << m)
        ops.d_lincomb(combined, [(1 << m, pow(rho, i, self.order), t[0]) for i, t in enumerate(tables)])
        proof, _ = self._open(combined.ptr(), m, point)
        return proof, evaluations

    def batch_verify(self, commitments, proof, point, evaluations, transcript=None):
        commitments, evaluations, point = list(commitments), list(evaluations), list(point)
        G1, r = self.E.curve.PointG1, self.order
        if not commitments or len(commitments) != len(evaluations) or any(not isinstance(c, G1) for c in commitments):
            return False
        rho = self._challenge(transcript, commitments, point, evaluations)
        commitment, evaluation, power = self.zero_commitment(), 0, 1
        for c, v in zip(commitments, evaluations):
            commitment = commitment + c * power
            evaluation = (evaluation + power * (int(v) % r)) % r
            power = power * rho % r
        return self.verify(commitment, proof, point, evaluation)
