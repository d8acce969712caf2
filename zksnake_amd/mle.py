"""
Multilinear polynomials on the GPU: the reference's `MultilinearPolynomial` pyclass (src/bn254/mle.rs:25-143,
src/bls12_381/mle.rs) over ark-poly's SparseMultilinearExtension, here a DENSE table of 2^num_vars canonical Fr elements
in HBM (a `DevVec`) behind the kernels of csrc/mle.hip.

Variable 0 is the least significant bit of the table index (ark-poly's order): `partial_evaluate([r0, r1])` fixes
variables 0 and 1 and leaves a polynomial whose variable 0 is the old variable 2.  Python integers appear only for
challenges and for what the caller asks to see (`to_evaluations`, `to_coefficients`, `evaluate`).
"""

import ctypes

import numpy as np

from . import _native as N
from .constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from .frvec import DevVec, FrOps

TILE_LOG = N.MLE_TILE_LOG  # variables folded per launch and tile (ZK_MLE_TILE_LOG in include/zkmi.h)


def _scalars(ops, values):
    """list of ints -> (k, 4) limbs, reduced mod r (at least one row, so that the pointer is valid)"""
    values = list(values)
    return ops.limbs(values) if values else np.zeros((1, 4), dtype=np.uint64)


class MultilinearPolynomial:
    """MultilinearPolynomial(num_vars, [(index, value), ...]) over the field `p` of the subclass (MLE_OBJECT[p]).

    An index >= 2^num_vars raises ValueError.  Values >= p are reduced, as Fr::from(BigUint) does.  For a repeated index the
    last value wins -- what collecting the pairs into ark-poly's map does; the crate is not vendored beside the reference, so
    this is PARITY UNPINNED.  Beyond the reference: `from_evaluations(values_or_limbs, p)` takes the dense table."""

    p = None

    def __init__(self, num_vars, evaluations=()):
        num_vars = int(num_vars)
        if num_vars < 0 or num_vars > 40:
            raise ValueError("num_vars must be in 0 .. 40")
        ops = FrOps(self.p)
        n = 1 << num_vars
        index, values = [], []
        for i, v in evaluations:
            if not 0 <= i < n:
                raise ValueError(f"evaluation index {i} is outside the hypercube of {num_vars} variables")
            index.append(i)
            values.append(v)
        table = np.zeros((n, 4), dtype=np.uint64)
        if index:
            table[np.asarray(index, dtype=np.int64)] = ops.limbs(values)   # in order: the last of a repeated index stays
        self._set(num_vars, ops.d_from(table))

    def _set(self, num_vars, vec):
        self._num_vars = num_vars
        self._vec = vec
        self._ops = FrOps(self.p)

    @classmethod
    def _wrap(cls, num_vars, vec):
        out = cls.__new__(cls)
        out._set(num_vars, vec)
        return out

    @staticmethod
    def from_evaluations(values, p):
        """dense input: a list of 2^k ints (reduced mod p) or a (2^k, 4) uint64 limb array (reduced on the device)"""
        cls = MLE_OBJECT[p]
        ops = FrOps(p)
        limbs = ops.limbs(values)
        n = limbs.shape[0]
        if n == 0 or n & (n - 1):
            raise ValueError("the number of evaluations must be a power of two")
        vec = ops.d_from(limbs)
        if isinstance(values, np.ndarray):
            N.check(N.load().zk_vec_canon_dev(ops.cid, n, vec.ptr(), None))
        return cls._wrap(n.bit_length() - 1, vec)

    @classmethod
    def zero(cls):
        return cls(0, [])

    # -- the pyclass surface --
    @property
    def num_vars(self):
        return self._num_vars

    def __len__(self):
        return 1 << self._num_vars

    def device_ptr(self):
        return self._vec.ptr()

    def evaluate(self, points):
        points = list(points)
        if len(points) != self._num_vars:
            raise ValueError("Evaluation requires points to be in the same size as the number of variables")
        ops = self._ops
        out = np.zeros(4, dtype=np.uint64)
        work = DevVec(1 << (max(self._num_vars - TILE_LOG, 0) + 1), zero=False)
        N.check(N.load().zk_mle_eval_dev(ops.cid, self._num_vars, self._vec.ptr(), N.u64p(_scalars(ops, points)), N.u64p(out), work.ptr(), None))
        return int.from_bytes(out.tobytes(), "little")

    def partial_evaluate(self, points):
        """fix variables 0 .. len(points)-1; the result has num_vars - len(points) variables (one evaluation when none is left)"""
        points = list(points)
        k = len(points)
        if k > self._num_vars:
            raise ValueError("invalid size of partial point")
        ops = self._ops
        out = DevVec(1 << (self._num_vars - k), zero=False)
        N.check(N.load().zk_mle_fix_dev(ops.cid, self._num_vars, self._vec.ptr(), k, N.u64p(_scalars(ops, points)), out.ptr(), None))
        return self._wrap(self._num_vars - k, out)

    def to_limbs(self):
        """the table as a (2^num_vars, 4) uint64 array"""
        return self._vec.download(len(self))

    def to_evaluations(self):
        return self._ops.ints(self.to_limbs())

    def to_coefficients(self):
        """entry i is the coefficient of prod_{b set in i} x_b"""
        ops = self._ops
        out = DevVec(len(self), zero=False)
        N.check(N.load().zk_mle_coeffs_dev(ops.cid, self._num_vars, self._vec.ptr(), out.ptr(), None))
        return ops.ints(out.download(len(self)))

    def sum(self):
        """sum of the table (the claim of a sumcheck)"""
        out = np.zeros(4, dtype=np.uint64)
        N.check(N.load().zk_mle_sum_dev(self._ops.cid, len(self), self._vec.ptr(), N.u64p(out), None))
        return int.from_bytes(out.tobytes(), "little")

    def _permuted(self, perm):
        out = DevVec(len(self), zero=False)
        arr = np.asarray(perm if len(perm) else [0], dtype=np.uint8)
        N.check(N.load().zk_mle_permute_dev(self._ops.cid, self._num_vars, self._vec.ptr(), N.u8p(arr), out.ptr(), None))
        return self._wrap(self._num_vars, out)

    def permute_evaluations(self, permutation):
        """value at index i moves to the index whose bit t is bit permutation[t] of i"""
        perm = [int(x) for x in permutation]
        if len(perm) != self._num_vars or sorted(perm) != list(range(self._num_vars)):
            raise ValueError("permutation must be a permutation of 0 .. num_vars-1")
        return self._permuted(perm)

    def swap(self, a, b, k):
        """exchange variables a .. a+k-1 with b .. b+k-1 (ark-poly's relabel)"""
        a, b, k = int(a), int(b), int(k)
        lo, hi = min(a, b), max(a, b)
        if k < 0 or lo < 0 or hi + k > self._num_vars:
            raise ValueError("invalid relabel argument")
        if lo != hi and lo + k > hi:
            raise ValueError("overlapped swap window is not allowed")
        perm = list(range(self._num_vars))
        if lo != hi:
            for i in range(k):
                perm[a + i], perm[b + i] = b + i, a + i
        return self._permuted(perm)

    def _is_the_zero(self):
        return self._num_vars == 0 and self._ops.d_is_zero(1, self._vec.ptr())

    def _combine(self, other, op):
        if not isinstance(other, MultilinearPolynomial) or other.p != self.p:
            return NotImplemented
        if self._num_vars != other._num_vars:
            # ark-poly: the zero polynomial (no variables) combines with anything, other sizes do not
            if other._is_the_zero():
                return self._wrap(self._num_vars, self._copy())
            if self._is_the_zero():
                zeros = DevVec(len(other))
                out = DevVec(len(other), zero=False)
                self._ops.d_op(op, len(other), zeros.ptr(), other._vec.ptr(), out.ptr())
                return self._wrap(other._num_vars, out)
            raise ValueError("trying to add non-zero polynomial with different number of variables")
        out = DevVec(len(self), zero=False)
        self._ops.d_op(op, len(self), self._vec.ptr(), other._vec.ptr(), out.ptr())
        return self._wrap(self._num_vars, out)

    def _copy(self):
        out = DevVec(len(self), zero=False)
        self._ops.d_copy(len(self), self._vec.ptr(), out.ptr())
        return out

    def __add__(self, other):
        return self._combine(other, 1)

    __radd__ = __add__

    def __sub__(self, other):
        return self._combine(other, 2)

    def __eq__(self, other):
        if not isinstance(other, MultilinearPolynomial):
            return NotImplemented
        if other.p != self.p or other._num_vars != self._num_vars:
            return False
        diff = DevVec(len(self), zero=False)
        self._ops.d_op(2, len(self), self._vec.ptr(), other._vec.ptr(), diff.ptr())
        return self._ops.d_is_zero(len(self), diff.ptr())

    __hash__ = None

    def __str__(self):
        return f"SparseMLPolynomial(num_vars={self._num_vars}, evaluations={self.to_evaluations()})"

    __repr__ = __str__


class _Bn254(MultilinearPolynomial):
    p = BN254_SCALAR_FIELD


class _Bls12_381(MultilinearPolynomial):
    p = BLS12_381_SCALAR_FIELD


_Bn254.__name__ = _Bn254.__qualname__ = _Bls12_381.__name__ = _Bls12_381.__qualname__ = "MultilinearPolynomial"
MLE_OBJECT = {BN254_SCALAR_FIELD: _Bn254, BLS12_381_SCALAR_FIELD: _Bls12_381}


def sumcheck_round(ops, log_n, tables, terms, r=None, out=None):
    """One call of zk_sumcheck_round_dev.  tables: device pointers of 2^log_n elements; terms: [(coeff, (table index, ..)), ..];
    r given: `out` (device pointers of 2^(log_n-1) elements) receives the tables with variable 0 fixed to r and the result is
    s(.) of those.  Returns [s(0), s(1), s(2), s(3)] as ints."""
    n_tables, n_terms = len(tables), len(terms)
    arr = N._vp * n_tables
    deg = (N._i * n_terms)(*[len(t[1]) for t in terms])
    idx = (N._i * (3 * n_terms))()
    for t, (_, which) in enumerate(terms):
        for j, tb in enumerate(which[:3]):
            idx[3 * t + j] = tb
    coeff = _scalars(ops, [c for c, _ in terms])
    s = np.zeros((4, 4), dtype=np.uint64)
    N.check(N.load().zk_sumcheck_round_dev(ops.cid, log_n, n_tables, arr(*tables), n_terms, N.u64p(coeff), deg, idx,
                                           None if r is None else N.u64p(ops.one(r)), None if out is None else arr(*out),
                                           N.u64p(s), None))
    return ops.ints(s)
