"""Poseidon over Fr of BN254 / BLS12-381: S-box x^5, widths 3, 4 and 5, R_F = 8, circomlib's partial
rounds.  `hash(x_1..x_k)` is circomlib's Poseidon(k); width 4 is pinned by the reference's circom fixture.

One hash, one sponge or one permutation runs on the host in Python integers (`permute`, `hash`, `sponge`): a verifier needs no
GPU.  Many of them run on the GPU, one permutation per lane (`permute_many`, `hash_many`, `sponge_many`, csrc/poseidon.hip).
Both sides use the constants the library generates (`zk_poseidon_params`, host arithmetic).

The GPU calls take rows as
  * an (n, k, 4) uint64 limb array (canonical, little-endian),
  * a sequence of n rows of k ints each, or
  * a `DevVec` of n * k elements together with k,
and return a `DevVec`.  An integer outside [0, r) is a ValueError -- a hash must not alias inputs mod r -- and so is a row of the
wrong length; both are raised before any device call.  Elements already in device memory are not checked: like every other
vector of the library they are canonical.
"""

import ctypes
import operator

import numpy as np

from .. import _native as N
from ..constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from ..frvec import DevVec

WIDTHS = (3, 4, 5)
MAX_ITEMS = 1 << N.POSEIDON_MAX_LOG
_MODULUS = {N.CURVE_BN254: BN254_SCALAR_FIELD, N.CURVE_BLS12_381: BLS12_381_SCALAR_FIELD}


def _below(limbs, r):
    """True where the (.., 4) limb array holds a value below r, without a Python-level loop"""
    top = [(r >> (64 * i)) & (2**64 - 1) for i in range(4)]
    less = np.zeros(limbs.shape[:-1], dtype=bool)
    equal = np.ones(limbs.shape[:-1], dtype=bool)
    for i in (3, 2, 1, 0):
        word = limbs[..., i]
        less |= equal & (word < np.uint64(top[i]))
        equal &= word == np.uint64(top[i])
    return less


class Poseidon:

    def __init__(self, curve="BN254"):
        self.curve = curve
        self.cid = N.curve_id(curve)
        self.p = _MODULUS[self.cid]
        self._params = {}

    # ---- parameters -----------------------------------------------------------------------------------------------------
    def params(self, t):
        """(R_F, R_P, round constants [round][i], matrix [i][j]) of width t as ints, from the library's generator (no GPU)"""
        if t not in WIDTHS:
            raise ValueError(f"the state has 3, 4 or 5 elements, not {t!r}")
        if t not in self._params:
            lib = N.load()
            rf, rp = ctypes.c_int(0), ctypes.c_int(0)
            N.check(lib.zk_poseidon_params(self.cid, t, ctypes.byref(rf), ctypes.byref(rp), None))
            rounds = rf.value + rp.value
            out = np.zeros((rounds * t + t * t, 4), dtype=np.uint64)
            N.check(lib.zk_poseidon_params(self.cid, t, None, None, N.u64p(out)))
            flat = N.limbs_to_ints(out)
            rc = [flat[k * t:(k + 1) * t] for k in range(rounds)]
            mds = [flat[rounds * t + i * t:rounds * t + (i + 1) * t] for i in range(t)]
            self._params[t] = (rf.value, rp.value, rc, mds)
        return self._params[t]

    # ---- host ---------------------------------------------------------------------------------------------------------------
    def _element(self, x):
        x = operator.index(x)
        if not 0 <= x < self.p:
            raise ValueError("a Poseidon input is an integer in [0, r)")
        return x

    def permute(self, state):
        """perm_t of a state of t = 3, 4 or 5 ints, as a list"""
        s = [self._element(x) for x in state]
        rf, rp, rc, mds = self.params(len(s))
        p = self.p
        for k in range(rf + rp):
            s = [x + c for x, c in zip(s, rc[k])]
            if k < rf // 2 or k >= rf // 2 + rp:
                s = [pow(x, 5, p) for x in s]
            else:
                s[0] = pow(s[0], 5, p)
            s = [sum(m * x for m, x in zip(row, s)) % p for row in mds]
        return s

    def hash(self, inputs):
        """circomlib's Poseidon(k) of k = 2, 3 or 4 ints"""
        inputs = list(inputs)
        if not 2 <= len(inputs) <= 4:
            raise ValueError(f"hash takes 2, 3 or 4 elements, not {len(inputs)}")
        return self.permute([0] + inputs)[0]

    def sponge(self, row):
        """the digest of a row of L >= 1 ints: width 3, rate 2, the length in the capacity element"""
        row = [self._element(x) for x in row]
        if not 1 <= len(row) <= N.POSEIDON_MAX_ROW:
            raise ValueError("a sponge row has 1 to 2^20 elements")
        s = [len(row), 0, 0]
        for i in range(0, len(row), 2):
            s[1] = (s[1] + row[i]) % self.p
            if i + 1 < len(row):
                s[2] = (s[2] + row[i + 1]) % self.p
            s = self.permute(s)
        return s[1]

    # ---- GPU ----------------------------------------------------------------------------------------------------------------
    def rows_in(self, rows, k, widths, what):
        """(n, k, source) of the rows of a GPU call, checked on the host: source is a DevVec (the caller's) or an (n * k, 4)
        limb array still to upload.  No device call."""
        if isinstance(rows, DevVec):
            if k is None:
                raise ValueError(f"{what}: a DevVec needs the number of elements per row")
            k = operator.index(k)
            if k not in widths:
                raise ValueError(f"{what}: a row has {widths.start} to {widths.stop - 1} elements, not {k}")
            if rows.n == 0 or rows.n % k:
                raise ValueError(f"{what}: {rows.n} elements are not whole rows of {k}")
            n, src = rows.n // k, rows
        elif isinstance(rows, np.ndarray):
            if rows.ndim != 3 or rows.shape[2] != 4 or rows.dtype != np.uint64:
                raise ValueError(f"{what}: an array of rows is (n, k, 4) uint64")
            if k is not None and rows.shape[1] != k:
                raise ValueError(f"{what}: a row has {k} elements, not {rows.shape[1]}")
            n, k = rows.shape[0], rows.shape[1]
            if k not in widths:
                raise ValueError(f"{what}: a row has {widths.start} to {widths.stop - 1} elements, not {k}")
            if not _below(rows, self.p).all():
                raise ValueError("a Poseidon input is an integer in [0, r)")
            src = np.ascontiguousarray(rows).reshape(n * k, 4)
        else:
            rows = [list(row) for row in rows]
            lens = {len(row) for row in rows}
            if k is not None and lens - {k}:
                raise ValueError(f"{what}: every row has {k} elements")
            if len(lens) > 1:
                raise ValueError(f"{what}: rows of different lengths")
            n, k = len(rows), (lens.pop() if lens else k)
            if n and k not in widths:
                raise ValueError(f"{what}: a row has {widths.start} to {widths.stop - 1} elements, not {k}")
            flat = [self._element(x) for row in rows for x in row]
            src = N.ints_to_limbs(flat, 4)
        if n == 0:
            raise ValueError(f"{what}: no rows")
        if n > MAX_ITEMS:
            raise ValueError(f"{what}: at most 2^{N.POSEIDON_MAX_LOG} rows a call")
        return n, k, src

    @staticmethod
    def on_device(src):
        """the rows in device memory: the caller's DevVec, or a new one filled from the limb array"""
        if isinstance(src, DevVec):
            return src
        vec = DevVec(src.shape[0], zero=False)
        vec.upload(src)
        return vec

    def permute_many(self, states, t=None):
        """perm_t of n states -> DevVec of n * t elements"""
        n, t, src = self.rows_in(states, t, range(3, 6), "permute_many")
        lib = N.ensure_gpu()
        vec, out = self.on_device(src), DevVec(n * t, zero=False)
        N.check(lib.zk_poseidon_perm_dev(self.cid, t, n, vec.ptr(), out.ptr(), None))
        return out

    def hash_many(self, rows, k=None):
        """hash of n rows of k = 2, 3 or 4 elements -> DevVec of n elements"""
        n, k, src = self.rows_in(rows, k, range(2, 5), "hash_many")
        lib = N.ensure_gpu()
        vec, out = self.on_device(src), DevVec(n, zero=False)
        N.check(lib.zk_poseidon_hash_dev(self.cid, k, n, vec.ptr(), out.ptr(), None))
        return out

    def sponge_many(self, rows, row_elems=None):
        """sponge of n rows of L >= 1 elements each -> DevVec of n digests"""
        n, k, src = self.rows_in(rows, row_elems, range(1, N.POSEIDON_MAX_ROW + 1), "sponge_many")
        lib = N.ensure_gpu()
        vec, out = self.on_device(src), DevVec(n, zero=False)
        N.check(lib.zk_poseidon_sponge_rows_dev(self.cid, n, vec.ptr(), k, out.ptr(), None))
        return out
