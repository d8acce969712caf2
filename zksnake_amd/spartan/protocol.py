"""
Spartan (Setty, CRYPTO 2020; the NIZK variant of section 5.1) for R1CS: two sumchecks, one multilinear KZG commitment and one
opening.  The reference has no Spartan, so there is nothing to interchange with; tests/spartan_model.py is the specification.

NO ZERO-KNOWLEDGE BLINDING: the commitment and the sumcheck messages are deterministic in the witness.  NIZK VARIANT: the verifier
reads the matrices (O(nnz), on the GPU); the computation commitment (SPARK) that would make it sublinear is not here.  Soundness
rests on the multilinear KZG SRS being honest; the SRS is universal -- `setup` does not depend on the circuit.

Layout.  n_row constraints, n_col wires of which the first n_public (the constant 1 included) are public.
    s_x = max(1, ceil(log2 n_row))                                variables of a constraint index
    h   = max(1, ceil(log2 max(n_col - n_public, n_public)))      variables of the committed table w
    s   = h + 1                                                   variables of z
Variable t is bit t of an index and point[t] goes to variable t (mle.py).  The columns are permuted so that the committed part of
z is a clean half of the hypercube: private wire j >= n_public sits at j - n_public (variable h = 0: the table w, zero padded),
public wire j < n_public at 2^h + j.  Then z~(ry) = (1 - ry[h]) w~(ry[:h]) + ry[h] pub~(ry[:h]) and the verifier needs one
opening of w and an O(n_public h) sum.

Both passes over the matrices read ONE merged three-matrix CSR (csrc/spartan.hip, include/zkmi.h): the row-major one gives
Az, Bz, Cz in one pass (zk_r1cs_products_dev), the column-major one M_r(y) = sum_i eq(rx, i) (rA A + rB B + rC C)[i, y]
(zk_r1cs_bind_dev).

Transcript (label b"spartan"), which is also the prover's order:
    instance digest (64 bytes), [public witness], C_w            -> tau (s_x challenges)
    outer sumcheck of E (Az Bz - Cz), E = eq(tau, .), claim 0: every round appends its 4 coefficients (zero padded) and draws one
        challenge                                                -> rx
    [va, vb, vc] = Az~(rx), Bz~(rx), Cz~(rx)                      -> rA, rB, rC
    inner sumcheck of M_r z, claim rA va + rB vb + rC vc: every round appends its 3 coefficients (zero padded) and draws one
        challenge                                                -> ry
    v_w = w~(ry[:h])
The rounds are driven here and not by Sumcheck.prove_arbitrary: a round polynomial that is identically zero is four (three)
zeros on this transcript, not the empty list the reference's sumcheck cannot append.
"""

import hashlib
import time

import numpy as np

from .. import _native as N
from ..commitment.polynomial import MultilinearKZG
from ..device import DeviceBuffer
from ..ecc import EllipticCurve
from ..frvec import DevVec, FrOps
from ..mle import MLE_OBJECT, TILE_LOG
from ..spmv import long_row_items
from ..subprotocol.gkr import eq_table
from ..subprotocol.sumcheck import ProductPolynomial
from ..transcript import FiatShamirTranscript
from .serialization import SpartanProof

MAX_LOG = N.R1CS_MAX_LOG


def _log2_ceil(n):
    return max(1, (int(n) - 1).bit_length())


def sizes(n_row, n_col, n_public):
    """(s_x, h, s) of an instance; ValueError when it does not fit"""
    if n_row < 1 or not 1 <= n_public <= n_col:
        raise ValueError("an R1CS has at least one constraint and 1 <= n_public <= n_col")
    s_x, h = _log2_ceil(n_row), _log2_ceil(max(n_col - n_public, n_public))
    if s_x > MAX_LOG or h > MAX_LOG:
        raise ValueError(f"at most 2^{MAX_LOG} constraints and 2^{MAX_LOG} private or public wires")
    return s_x, h, h + 1


def merged_csr(log_seg, mats):
    """The merged CSR of three matrices given as (segment, idx, value limbs) numpy columns: (ptr u32[3 * 2^log_seg + 1], idx u32,
    val (nnz, 4) uint64).  Entries keep their order within a sub-segment."""
    q = np.concatenate([3 * np.asarray(seg, dtype=np.int64) + m for m, (seg, _, _) in enumerate(mats)])
    idx = np.concatenate([np.asarray(i, dtype=np.int64) for _, i, _ in mats])
    val = np.concatenate([np.asarray(v, dtype=np.uint64).reshape(-1, 4) for _, _, v in mats])
    order = np.argsort(q, kind="stable")
    ptr = np.zeros(3 * (1 << log_seg) + 1, dtype=np.uint32)
    np.cumsum(np.bincount(q, minlength=3 * (1 << log_seg)), out=ptr[1:])
    return ptr, np.ascontiguousarray(idx[order].astype(np.uint32)), np.ascontiguousarray(val[order])


def long_segments(ptr):
    """(long_segs, item_ptr u32[3 n_long + 1], items): `long_row_items` applied to the sub-segment pointer, regrouped by segment --
    a segment is long when one of its sub-segments is, and its short sub-segments have no item"""
    long_q, q_item_ptr, items = long_row_items(ptr)
    long_segs = np.unique(long_q // 3).astype(np.uint32)
    counts = np.zeros(3 * long_segs.shape[0], dtype=np.int64)
    counts[3 * np.searchsorted(long_segs, long_q // 3) + long_q % 3] = np.diff(q_item_ptr.astype(np.int64))
    item_ptr = np.zeros(3 * long_segs.shape[0] + 1, dtype=np.uint32)
    np.cumsum(counts, out=item_ptr[1:])
    return long_segs, item_ptr, items


class DeviceR1csCsr:
    """a merged three-matrix CSR resident on the device with its long-segment work items"""

    def __init__(self, curve_id, log_seg, ptr, idx, val):
        self.cid, self.log_seg, self.n_entries = curve_id, log_seg, int(idx.shape[0])
        assert ptr.shape[0] == 3 * (1 << log_seg) + 1 and int(ptr[-1]) == self.n_entries
        self.ptr = DeviceBuffer.from_numpy(np.ascontiguousarray(ptr, dtype=np.uint32))
        self.idx = DeviceBuffer.from_numpy(idx) if self.n_entries else None
        self.val = DeviceBuffer.from_numpy(val) if self.n_entries else None
        long_segs, item_ptr, items = long_segments(ptr)
        self.n_long, self.n_items = int(long_segs.shape[0]), int(items.shape[0])
        self.long_segs = self.item_ptr = self.items = self.partials = None
        if self.n_long:
            self.long_segs, self.item_ptr = DeviceBuffer.from_numpy(long_segs), DeviceBuffer.from_numpy(item_ptr)
            self.items, self.partials = DeviceBuffer.from_numpy(items), DeviceBuffer(self.n_items * 32)

    def args(self):
        p = lambda b: None if b is None else b.ptr  # noqa: E731
        return (self.log_seg, self.n_entries, self.ptr.ptr, p(self.idx), p(self.val), self.n_long, p(self.long_segs), p(self.item_ptr),
                self.n_items, p(self.items), p(self.partials))

    def products(self, log_x, d_z, d_az, d_bz, d_cz, stream=None):
        N.check(N.load().zk_r1cs_products_dev(self.cid, *self.args(), log_x, d_z, d_az, d_bz, d_cz, stream))

    def bind(self, log_x, d_e, coeff_limbs, d_out, stream=None):
        N.check(N.load().zk_r1cs_bind_dev(self.cid, *self.args(), log_x, d_e, N.u64p(coeff_limbs), d_out, stream))

    def free(self):
        for b in (self.ptr, self.idx, self.val, self.long_segs, self.item_ptr, self.items, self.partials):
            if b is not None:
                b.free()


def _pad(coeffs, n):
    coeffs = list(coeffs)
    assert len(coeffs) <= n
    return coeffs + [0] * (n - len(coeffs))


def _horner(coeffs, x, p):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


def eq_point(a, b, p):
    """eq(a, b) for two points of the same length"""
    out = 1
    for x, y in zip(a, b):
        out = out * ((x * y + (1 - x) * (1 - y)) % p) % p
    return out


def public_mle(public, point, p):
    """the multilinear extension of (public, 0, ..) at `point`: O(len(public) * len(point)) on the host"""
    total = 0
    for j, v in enumerate(public):
        e = v % p
        for t, x in enumerate(point):
            e = e * (x if (j >> t) & 1 else 1 - x) % p
        total += e
    return total % p


class Spartan:
    """Spartan(r1cs): the curve is the R1CS's.  The constructor compiles the instance once (sizes, column permutation, both
    merged CSRs on the device, the instance digest); `setup(tau=None)` is the universal multilinear KZG setup over h variables;
    `prove(public_witness, private_witness)` -> SpartanProof; `verify(proof, public_witness)` -> bool."""

    def __init__(self, r1cs):
        r1cs.compile()
        self.r1cs = r1cs
        self.curve = r1cs.curve
        self.E = EllipticCurve(self.curve)
        self.order = self.E.order
        self._ops = FrOps(self.order)
        self.n_row, self.n_col, self.n_public = r1cs.A.n_row, r1cs.A.n_col, int(r1cs.n_public)
        self.s_x, self.h, self.s = sizes(self.n_row, self.n_col, self.n_public)
        self.mkzg = MultilinearKZG(self.h, self.curve)
        rows_m, cols_m = [], []
        for mat in (r1cs.A, r1cs.B, r1cs.C):
            if (mat.n_row, mat.n_col) != (self.n_row, self.n_col):
                raise ValueError("A, B and C must have the same shape")
            row_ptr, cols, vals = mat.to_csr()           # validates the indices: the kernels gather unchecked
            rows = np.repeat(np.arange(self.n_row, dtype=np.int64), np.diff(row_ptr.astype(np.int64)))
            new_cols = self.column(cols.astype(np.int64))
            rows_m.append((rows, new_cols, vals))
            cols_m.append((new_cols, rows, vals))
        ptr, idx, val = merged_csr(self.s_x, rows_m)
        self.digest = hashlib.blake2b(b"".join(int(v).to_bytes(8, "little") for v in (self.n_row, self.n_col, self.n_public, self.s_x, self.s))
                                      + ptr.tobytes() + idx.tobytes() + val.tobytes()).digest()
        N.ensure_gpu()
        self._rows = DeviceR1csCsr(self._ops.cid, self.s_x, ptr, idx, val)
        self._cols = DeviceR1csCsr(self._ops.cid, self.s, *merged_csr(self.s, cols_m))

    def column(self, j):
        """where wire j sits in z (an int or an integer array)"""
        return np.where(j >= self.n_public, j - self.n_public, (1 << self.h) + j) if isinstance(j, np.ndarray) else \
            (j - self.n_public if j >= self.n_public else (1 << self.h) + j)

    # -- the SRS: nothing here depends on the circuit --
    def setup(self, tau=None):
        self.mkzg.setup(tau)

    @property
    def G2_tau(self):
        return self.mkzg.G2_tau

    @G2_tau.setter
    def G2_tau(self, value):
        self.mkzg.G2_tau = value

    def release(self):
        """free the device-resident matrices and the SRS; the object cannot be used afterwards"""
        for csr in (self._rows, self._cols):
            if csr is not None:
                csr.free()
        self._rows = self._cols = None
        self.mkzg.release()

    def _live(self):
        if self._rows is None:
            raise RuntimeError("this Spartan instance has been released")

    # -- the transcript --
    def _start(self, transcript, public, commitment):
        transcript = transcript or FiatShamirTranscript(b"spartan", field=self.order)
        transcript.append(self.digest)
        transcript.append(list(public))
        transcript.append(commitment)
        return transcript

    def challenges(self, proof, public_witness, transcript=None):
        """Replay the transcript of a well-formed proof: (tau, rx, (rA, rB, rC), ry)."""
        p = self.order
        tr = self._start(transcript, [int(v) % p for v in public_witness], proof.commitment)
        tau = [tr.get_challenge_scalar() for _ in range(self.s_x)]
        rx, ry = [], []
        for coeffs in proof.outer:
            tr.append(list(coeffs))
            rx.append(tr.get_challenge_scalar())
        tr.append(list(proof.evals))
        r_abc = tuple(tr.get_challenge_scalar() for _ in range(3))
        for coeffs in proof.inner:
            tr.append(list(coeffs))
            ry.append(tr.get_challenge_scalar())
        tr.append(proof.v_w)
        return tau, rx, r_abc, ry

    def _public(self, public_witness):
        public = [int(v) % self.order for v in public_witness]
        if len(public) != self.n_public:
            raise ValueError(f"{self.n_public} public values expected (the constant 1 first), got {len(public)}")
        return public

    def _rounds(self, poly, count, width, tr):
        """drive `count` sumcheck rounds of a ProductPolynomial: ([coefficients zero padded to `width`], challenges)"""
        rounds, r = [], []
        for _ in range(count):
            coeffs = _pad(poly.round_function(list(r)).coeffs(), width)
            tr.append(coeffs)
            rounds.append(coeffs)
            r.append(tr.get_challenge_scalar())
        return rounds, r

    def _bind(self, rx, r_abc):
        """the table M_r of 2^s entries on the device"""
        ex = eq_table(self._ops, rx)
        m_r = DevVec(1 << self.s, zero=False)
        self._cols.bind(self.s_x, ex.ptr(), self._ops.limbs(list(r_abc)), m_r.ptr())
        return m_r

    def prove(self, public_witness, private_witness, transcript=None, timings=None):
        """`timings`: a dict that receives the wall-clock milliseconds of every phase (tools/spartan_bench.py); the device is
        synchronised at the phase boundaries then, and only then"""
        self._live()
        self.mkzg._need_setup()
        ops, p, lib = self._ops, self.order, N.ensure_gpu()
        clock = [time.perf_counter()]

        def mark(phase):
            if timings is not None:
                N.check(lib.zk_dev_synchronize())
                now = time.perf_counter()
                timings[phase] = timings.get(phase, 0.0) + (now - clock[0]) * 1e3
                clock[0] = now

        public = self._public(public_witness)
        n_private = self.n_col - self.n_public
        w = DevVec(1 << self.h)
        if ops.d_load(w, 0, private_witness, n_private) != n_private:
            raise ValueError(f"{n_private} private values expected")
        z = DevVec(1 << self.s)
        ops.d_copy(1 << self.h, w.ptr(), z.ptr())
        z.upload(ops.limbs(public), 1 << self.h)
        mark("host")
        commitment = self.mkzg.commit(w)
        mark("commit")
        tr = self._start(transcript, public, commitment)
        tau = [tr.get_challenge_scalar() for _ in range(self.s_x)]
        n = 1 << self.s_x
        e = eq_table(ops, tau)
        az, bz, cz = DevVec(n, zero=False), DevVec(n, zero=False), DevVec(n, zero=False)
        mark("host")
        self._rows.products(self.s, z.ptr(), az.ptr(), bz.ptr(), cz.ptr())
        mark("products")
        t = DevVec(n, zero=False)
        ops.d_mul(n, az.ptr(), bz.ptr(), t.ptr())
        ops.d_op(2, n, t.ptr(), cz.ptr(), t.ptr())
        if not ops.d_is_zero(n, t.ptr()):
            raise ValueError("witness does not satisfy the R1CS")
        mark("host")
        cls = MLE_OBJECT[p]
        tables = [cls._wrap(self.s_x, v) for v in (e, az, bz, cz)]
        outer, rx = self._rounds(ProductPolynomial(tables, [(1, (0, 1, 2)), (p - 1, (0, 3))], p), self.s_x, 4, tr)
        evals = tuple(m.evaluate(rx) for m in tables[1:])
        tr.append(list(evals))
        r_abc = tuple(tr.get_challenge_scalar() for _ in range(3))
        mark("outer")
        m_r = self._bind(rx, r_abc)
        mark("bind")
        inner, ry = self._rounds(ProductPolynomial([cls._wrap(self.s, m_r), cls._wrap(self.s, z)], [(1, (0, 1))], p), self.s, 3, tr)
        mark("inner")
        opening, v_w = self.mkzg.open(w, ry[:self.h])
        tr.append(v_w)
        mark("open")
        return SpartanProof(commitment, outer, evals, inner, v_w, opening, self.curve)

    def _well_formed(self, proof):
        p, G1 = self.order, self.E.curve.PointG1
        scalar = lambda v: isinstance(v, int) and not isinstance(v, bool) and 0 <= v < p  # noqa: E731
        rows = lambda rs, count, width: (isinstance(rs, (list, tuple)) and len(rs) == count and  # noqa: E731
                                         all(isinstance(c, (list, tuple)) and len(c) == width and all(scalar(v) for v in c) for c in rs))
        return (isinstance(proof, SpartanProof) and isinstance(proof.commitment, G1) and rows(proof.outer, self.s_x, 4)
                and rows(proof.inner, self.s, 3) and isinstance(proof.evals, (list, tuple)) and len(proof.evals) == 3
                and all(scalar(v) for v in proof.evals) and scalar(proof.v_w) and isinstance(proof.opening, (list, tuple))
                and len(proof.opening) == self.h and all(isinstance(q, G1) for q in proof.opening))

    def verify(self, proof, public_witness, transcript=None):
        self._live()
        p, ops = self.order, self._ops
        try:
            public = [int(v) % p for v in public_witness]
        except (TypeError, ValueError):
            return False
        if len(public) != self.n_public or not self._well_formed(proof):
            return False
        tau, rx, r_abc, ry = self.challenges(proof, public, transcript)
        claim = 0
        for coeffs, r in zip(proof.outer, rx):          # four coefficients: degree <= 3
            if (2 * coeffs[0] + sum(coeffs[1:])) % p != claim:
                return False
            claim = _horner(coeffs, r, p)
        va, vb, vc = proof.evals
        if eq_point(tau, rx, p) * (va * vb - vc) % p != claim:
            return False
        claim = sum(r * v for r, v in zip(r_abc, proof.evals)) % p
        for coeffs, r in zip(proof.inner, ry):          # three coefficients: degree <= 2
            if (2 * coeffs[0] + sum(coeffs[1:])) % p != claim:
                return False
            claim = _horner(coeffs, r, p)
        v_z = ((1 - ry[self.h]) * proof.v_w + ry[self.h] * public_mle(public, ry[:self.h], p)) % p
        N.ensure_gpu()
        m_r = self._bind(rx, r_abc)
        out = np.zeros(4, dtype=np.uint64)
        work = DevVec(1 << (max(self.s - TILE_LOG, 0) + 1), zero=False)
        N.check(N.load().zk_mle_eval_dev(ops.cid, self.s, m_r.ptr(), N.u64p(ops.limbs(ry)), N.u64p(out), work.ptr(), None))
        if int.from_bytes(out.tobytes(), "little") * v_z % p != claim:
            return False
        return bool(self.mkzg.verify(proof.commitment, list(proof.opening), ry[:self.h], proof.v_w))
