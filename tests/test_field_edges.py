"""Field primitives at the ends of their ranges: tests/native/field_edges.hip runs the primitives of csrc/field.hip.h, the lazy NTT
steps of csrc/ntt_lazy.hip.h and the relaxed bucket step of csrc/curve.hip.h on raw register-form limbs.  The host build (g++, and
g++ with UBSan) runs in the CPU suite; the device build (the library's own hipcc pipeline, gfx950) must give the host's output limb
for limb (`-m gpu`).  Every record is checked against plain integers: the exact identity of the primitive (Montgomery products
as (s + m p) / R with m = -s p^-1 mod R, lazy forms as e.g. a - b + K p), the output range promised at its definition and, where
promised, a canonical result.  Operands are generated per documented precondition ("value < K p, limbs < 2^B"): the edges 0, 1, 2,
j p - 1, j p, j p + 1, K p - 2^i, the largest value whose top limb is one below that of K p, all non-top limbs at 2^29 - 1, values
just below a top-limb step, then seeded random values, 30 % of them within 2^20 of the top of the range.  Products take pairs on
their documented bound (a b <= R p) and the operand shapes the kernels create.

Contracts checked here (p the field's modulus, R = 2^(29 N), "norm" = every limb but the top one below 2^29):

  primitive                 input contract                                 promised output                         test
  fp_add / fp_sub           a, b < 2p, norm                                a +- b, selected into [0, 2p), norm      test_host_field_ops
  fp_reduce_full            a < 2p                                         a mod p, canonical                       test_host_field_ops
  fp_reduce_2p              a < 4p                                         [0, 2p)                                  test_host_field_ops
  fp_is_zero / _limbs / eq  a, b < 2p                                      p is zero for fp_is_zero, not for _limbs test_host_field_ops
  fp_mul / fp_sqr           a b <= R p, norm                               (a b + m p) / R < 2p, norm               test_host_field_ops
  fp_mul2                   a b + c d <= R p, one lazy operand per product (a b + c d + m p) / R < 2p, norm         test_host_field_ops
  fp_mul4 (N = 9)           four products <= R p, c and e lazy (< 2^30)    < 2p, norm                               test_host_field_ops
  fp_inv                    a < 2p                                         a^-1 (Montgomery), < 2p                  test_host_field_ops
  fp_sub_lazy               a, b < 2p                                      a - b + 4p exactly, limbs < 2^31, < 6p   test_host_field_ops
  fp_sub_k<2|4|8>           a < 2p, b < K p                                a - b + K p, norm, in (0, (K+2) p)      test_host_field_ops
  fp_sub_twice_sel4         t < 4p, q < 2p                                 t - 2q selected into [0, 4p), norm       test_host_field_ops
  fp_sub_lazy8              a < 2p, b < 4p or b_top < top(8p)              a - b + 8p exactly, limbs < 3 2^29       test_host_field_ops,
                                                                                                                    test_sub_lazy8_outside_its_contract
  fp_neg_lazy               b < 2p                                         4p - b exactly, limbs < 2^30             test_host_field_ops
  fp_neg_lazy_k<4|8>        b < (K-1) p                                    K p - b exactly, limbs < 2^30            test_host_field_ops
  fp_add_nosel / dbl_lazy   a, b < 6p, norm                                a + b norm / 2a limb-wise (< 2^30)       test_host_field_ops
  fp_from_canonical         any 32 W-bit integer                           x R mod p, < 2p                          test_host_field_ops
  fp_to_canonical           a < 2p                                         a / R mod p as W words                   test_host_field_ops
  fp2_mul / sqr / inv       components < 2p                                exact Montgomery forms, < 2p             test_host_field_ops
  fp2_mul_relaxed<K>        a1 < (K-1) p, a0 b0 + K p b1 <= R p, ..        < 2p                                     test_host_field_ops
  fp2_sqr_relaxed<KD>       a1 < KD p, (a0 + a1)(a0 - a1 + KD p) <= R p    < 2p                                     test_host_field_ops
  lz_sub<18,29> / <36,30>   b limbs < 2^BITS, b <= K p / 2                 a - b + K p, limbs < 3 / 5 2^29          test_host_field_ops
  lz_norm                   limbs < 2^31                                   same value, norm                         test_host_field_ops
  lz_reduce<8|2>            limbs < 2^31, value < 4.5 U p                  a - k U p, norm, < 1.09 U p              test_host_field_ops
  lz_canonical              norm, < 9p                                     a mod p, canonical                       test_host_field_ops
  G2 relaxed step           X < 4p, Y, ZZ, ZZZ, base < 2p (per component)  madd-2008-s, X < 4p, rest < 2p           test_host_g2_relaxed_step
  G1 / G2 step (device)     the same                                       the same                                 test_device_bucket_step
  all of the above (device) inside the contract                            limb-equal to the host build             test_device_field_ops
"""

import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "field_edges.hip")
B = 29
MASK = (1 << B) - 1

(ADD, SUB, REDUCE_FULL, REDUCE_2P, IS_ZERO, IS_ZERO_LIMBS, EQ, MUL, MUL2, MUL4, SQR, INV, SUB_LAZY, SUB_K2, SUB_K4, SUB_K8,
 SUB_TWICE_SEL4, SUB_LAZY8, NEG_LAZY, NEG_LAZY_K4, NEG_LAZY_K8, ADD_NOSEL, DBL_LAZY, FROM_CANONICAL, TO_CANONICAL, FP2_MUL,
 FP2_SQR, FP2_INV, FP2_MUL_REL4, FP2_MUL_REL8, FP2_SQR_REL4, FP2_SQR_REL8, LZ_SUB_18_29, LZ_SUB_36_30, LZ_NORM, LZ_REDUCE8,
 LZ_REDUCE2, LZ_CANONICAL, G1_STEP, G2_STEP) = range(40)
OP_NAMES = ["add", "sub", "reduce_full", "reduce_2p", "is_zero", "is_zero_limbs", "eq", "mul", "mul2", "mul4", "sqr", "inv",
            "sub_lazy", "sub_k2", "sub_k4", "sub_k8", "sub_twice_sel4", "sub_lazy8", "neg_lazy", "neg_lazy_k4", "neg_lazy_k8",
            "add_nosel", "dbl_lazy", "from_canonical", "to_canonical", "fp2_mul", "fp2_sqr", "fp2_inv", "fp2_mul_rel4",
            "fp2_mul_rel8", "fp2_sqr_rel4", "fp2_sqr_rel8", "lz_sub_18_29", "lz_sub_36_30", "lz_norm", "lz_reduce8", "lz_reduce2",
            "lz_canonical", "g1_step", "g2_step"]


class Field:
    def __init__(self, fid, name, p, n, w):
        self.fid, self.name, self.p, self.N, self.W = fid, name, p, n, w
        self.R = 1 << (B * n)
        self.Rinv = pow(self.R, -1, p)
        self.pinv = pow(p, -1, self.R)
        self.TOP = B * (n - 1)   # bit position of the top limb

    def __repr__(self):
        return self.name

    def limbs(self, v):
        assert 0 <= v < 1 << (self.TOP + 32), v
        return [(v >> (B * i)) & MASK for i in range(self.N - 1)] + [v >> self.TOP]

    def top(self, v):
        return v >> self.TOP

    def mont(self, s):
        """the value of a Montgomery reduction of s: (s + m p) / R with m = -s p^-1 mod R"""
        m = (-s * self.pinv) % self.R
        t = s + m * self.p
        assert t % self.R == 0
        return t // self.R

    def kp_limbs(self, k):
        return self.limbs(k * self.p)


FIELDS = [Field(0, "BN254 Fq", pyref.BN254_P, 9, 8), Field(1, "BN254 Fr", pyref.BN254_R, 9, 8),
          Field(2, "BLS12-381 Fq", pyref.BLS_P, 14, 12), Field(3, "BLS12-381 Fr", pyref.BLS_R, 9, 8)]
FQ = [FIELDS[0], FIELDS[2]]
FR = [FIELDS[1], FIELDS[3]]


def val(ls):
    return sum(int(x) << (B * i) for i, x in enumerate(ls))


def is_norm(ls):
    return all(int(x) <= MASK for x in ls[:-1])


# ---- operand generator ----------------------------------------------------------------------------------------------------
def edges(f, k):
    """edge values of the precondition "value < k p, normalised limbs" """
    p, hi = f.p, k * f.p
    vs = {0, 1, 2, hi - 1}
    for j in range(1, k + 1):
        vs |= {j * p - 1, j * p, j * p + 1}
    for i in list(range(0, hi.bit_length(), 23)) + [hi.bit_length() - 2, hi.bit_length() - 1]:
        vs.add(hi - (1 << i))
    low = (1 << f.TOP) - 1
    t = f.top(hi)
    vs |= {((t - 1) << f.TOP) | low, low, (1 << f.TOP) | low}   # top limb one below that of k p; all non-top limbs at 2^29 - 1
    for s in {1, max(1, t // 2), t}:
        vs |= {(s << f.TOP) - 1, (s << f.TOP) - 2}                # just below a top-limb step
    return sorted(v for v in vs if 0 <= v < hi)


def rand_below(rnd, hi):
    """seeded random value below hi, 30 % of them within 2^20 of the top"""
    if rnd.random() < 0.3:
        return hi - 1 - rnd.randrange(min(hi, 1 << 20))
    return rnd.randrange(hi)


def tuples(f, bounds, seed, n_random=2000, max_edges=None):
    """edge cross product for the given per-operand bounds (values), plus seeded random tuples"""
    import itertools
    rnd = random.Random(seed)
    lists = []
    for hi in bounds:
        k = -(-hi // f.p)
        e = [v for v in edges(f, k) if v < hi] + [hi - 1]
        if max_edges and len(e) > max_edges:
            e = sorted(set(rnd.sample(e, max_edges) + [0, hi - 1]))
        lists.append(sorted(set(e)))
    out = list(itertools.product(*lists))
    out += [tuple(rand_below(rnd, hi) for hi in bounds) for _ in range(n_random)]
    return out


# ---- records ----------------------------------------------------------------------------------------------------------------
def pack(f, rows):
    """rows: per record a list of limb lists (operands in register form) -> (count, 16 N) uint32"""
    arr = np.zeros((len(rows), 16 * f.N), dtype=np.uint32)
    for r, ops in enumerate(rows):
        flat = [x for op in ops for x in op]
        arr[r, :len(flat)] = flat
    return arr


class Harness:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.fe_run.restype = ctypes.c_int
        self.lib.fe_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]

    def run(self, f, op, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint32)
        out = np.zeros((arr.shape[0], 8 * f.N), dtype=np.uint32)
        rc = self.lib.fe_run(f.fid, op, arr.shape[0], arr.ctypes.data, out.ctypes.data)
        assert rc == 0, f"fe_run({f}, {OP_NAMES[op]}) returned {rc}"
        return out


# ---- lazy forms as the kernels create them (limb lists) --------------------------------------------------------------------
def borrow_proof(f, k, bits=B):
    """k p with every limb but the top one borrowing 2^bits from the limb above (the lazy constants of field.hip.h / ntt_lazy.hip.h)"""
    kp = f.kp_limbs(k)
    return [kp[i] + ((1 << bits) if i < f.N - 1 else 0) - ((1 << (bits - B)) if i > 0 else 0) for i in range(f.N)]


def lazy_sub(f, a, b, k, bits=B):
    c = borrow_proof(f, k, bits)
    return [(x + y - z) & 0xFFFFFFFF for x, y, z in zip(f.limbs(a) if isinstance(a, int) else a, c, f.limbs(b) if isinstance(b, int) else b)]


def limbwise_add(*xs):
    return [sum(t) for t in zip(*xs)]


# ---- cases: (operand limb lists per record, checker(record operands, output words) -> None) -------------------------------
def field_cases(f, op, seed):
    """list of records (operand limb lists) and the per-record check; only operands inside the primitive's contract"""
    p, L = f.p, f.limbs
    N = f.N
    recs, chk = [], None
    lt = lambda hi: (lambda v: 0 <= v < hi)  # noqa: E731

    def one(bounds, **kw):
        return [[L(v) for v in t] for t in tuples(f, bounds, seed, **kw)]

    def norm_val(o, hi, exact=None):
        assert is_norm(o), o
        v = val(o)
        assert v < hi, (v, hi)
        if exact is not None:
            assert v == exact, (v, exact)
        return v

    if op in (ADD, SUB):
        recs = one([2 * p, 2 * p])

        def chk(ins, o):
            a, b = val(ins[0]), val(ins[1])
            s = a + b if op == ADD else a - b
            e = s - 2 * p if s >= 2 * p else (s + 2 * p if s < 0 else s)
            norm_val(o[:N], 2 * p, e)
    elif op == REDUCE_FULL:
        recs = one([2 * p])
        chk = lambda ins, o: norm_val(o[:N], p, val(ins[0]) % p)  # noqa: E731
    elif op == REDUCE_2P:
        recs = one([4 * p])

        def chk(ins, o):
            a = val(ins[0])
            norm_val(o[:N], 2 * p, a - 2 * p if a >= 2 * p else a)
    elif op in (IS_ZERO, IS_ZERO_LIMBS):
        recs = one([2 * p])

        def chk(ins, o):
            a = val(ins[0])
            assert int(o[0]) == int(a in (0, p) if op == IS_ZERO else a == 0), a
    elif op == EQ:
        recs = one([2 * p, 2 * p], max_edges=24)
        chk = lambda ins, o: (int(o[0]) == int((val(ins[0]) - val(ins[1])) % p == 0)) or pytest.fail(str(ins))  # noqa: E731
    elif op in (MUL, SQR):
        from math import isqrt
        rp = f.R * p
        rnd = random.Random(seed)
        if op == SQR:
            sq = edges(f, 2) + [rand_below(rnd, 2 * p) for _ in range(2000)] + [isqrt(rp), isqrt(rp) - 1] + \
                [k * p - 1 for k in (4, 6, 8, 12) if (k * p - 1) ** 2 <= rp]
            recs = [[L(a)] for a in sq]
        else:
            pairs = tuples(f, [2 * p, 2 * p], seed)
            # on the documented bound a b <= R p: the largest partner of values at the ends of the kernels' operand ranges
            for ka in (1, 2, 4, 6, 8, 10, 12, 27, 54):
                for a in (ka * p - 1, ka * p - 1 - (1 << 20)):
                    if a * p <= rp:
                        pairs += [(a, rp // a), (rp // a, a)]
            recs = [[L(a), L(b)] for a, b in pairs]
            for _ in range(500):
                x, y = rand_below(rnd, 2 * p), rand_below(rnd, 2 * p)
                recs.append([lazy_sub(f, x, y, 4), L(rand_below(rnd, 2 * p))])          # fp_sub_lazy (< 6p) against < 2p
                if f.fid in (1, 3):
                    x9 = [rand_below(rnd, 9 * p) for _ in range(4)]
                    a0, b0 = limbwise_add(L(x9[0]), L(x9[1])), limbwise_add(L(x9[2]), L(x9[3]))
                    tw = L(rand_below(rnd, p))
                    recs.append([lazy_sub(f, a0, b0, 36, 30), tw])                         # 54p operand, limbs < 5 2^29
                    recs.append([lazy_sub(f, x9[0], x9[1], 18), tw])                       # 27p against p
            if f.fid in (1, 3):   # the extremes of the two lazy NTT operands against the largest canonical twiddle
                top18 = limbwise_add(L(9 * p - 1), L(9 * p - 1))
                recs += [[lazy_sub(f, top18, [0] * N, 36, 30), L(p - 1)], [lazy_sub(f, 9 * p - 1, 0, 18), L(p - 1)],
                         [lazy_sub(f, [0] * N, top18, 36, 30), L(p - 1)], [lazy_sub(f, 0, 9 * p - 1, 18), L(p - 1)]]

        def chk(ins, o):
            a = val(ins[0])
            b = a if op == SQR else val(ins[1])
            assert a * b <= f.R * p
            norm_val(o[:N], 2 * p, f.mont(a * b))
    elif op in (MUL2, MUL4):
        rnd = random.Random(seed)
        k = 2 if op == MUL2 else 4
        for _ in range(1500):
            recs.append([L(rand_below(rnd, 2 * p)) for _ in range(2 * k)])
        e = edges(f, 2)
        for i in range(0, len(e), 2):
            recs.append([L(e[i])] * (2 * k))
            recs.append([L(e[-1 - i])] * (2 * k))
        if op == MUL2:
            for _ in range(600):
                a0, a1, b0, b1 = (rand_below(rnd, 2 * p) for _ in range(4))
                recs.append([L(a0), L(b0), lazy_sub(f, 0, a1, 4), L(b1)])                 # fp2_mul: a0 b0 + (4p - a1) b1
                if f.N <= 10:
                    r, q, x3, y, ppp = rand_below(rnd, 4 * p), rand_below(rnd, 2 * p), rand_below(rnd, 4 * p), rand_below(rnd, 2 * p), rand_below(rnd, 2 * p)
                    recs.append([L(r), lazy_sub(f, q, x3, 8), lazy_sub(f, 0, y, 4), L(ppp)])  # Y3 of the G1 step
        elif f.fid == 0:
            for _ in range(800):   # Y3 of the BN254 G2 step: R0 < 4p, D < 6p, 8p - R1, 4p - Y0, PPP, Y1 < 2p
                R0, R1, D0, D1 = rand_below(rnd, 4 * p), rand_below(rnd, 4 * p), rand_below(rnd, 6 * p), rand_below(rnd, 6 * p)
                Y0, Y1, P0, P1 = (rand_below(rnd, 2 * p) for _ in range(4))
                recs.append([L(R0), L(D0), lazy_sub(f, 0, R1, 8), L(D1), lazy_sub(f, 0, Y0, 4), L(P0), L(Y1), L(P1)])

        def chk(ins, o):
            s = sum(val(ins[2 * i]) * val(ins[2 * i + 1]) for i in range(k))
            assert s <= f.R * p
            norm_val(o[:N], 2 * p, f.mont(s))
    elif op == INV:
        recs = one([2 * p])

        def chk(ins, o):
            a = val(ins[0]) % p
            e = 0 if a == 0 else pow(a * f.Rinv % p, -1, p) * f.R % p
            assert val(o[:N]) % p == e and norm_val(o[:N], 2 * p) is not None
    elif op == SUB_LAZY:
        recs = one([2 * p, 2 * p])

        def chk(ins, o):
            assert all(int(x) < 1 << 31 for x in o[:N])
            assert val(o[:N]) == val(ins[0]) - val(ins[1]) + 4 * p < 6 * p
    elif op in (SUB_K2, SUB_K4, SUB_K8):
        k = {SUB_K2: 2, SUB_K4: 4, SUB_K8: 8}[op]
        recs = one([2 * p, k * p])

        def chk(ins, o):
            e = val(ins[0]) - val(ins[1]) + k * p
            assert 0 < e
            norm_val(o[:N], (k + 2) * p, e)
    elif op == SUB_TWICE_SEL4:
        recs = one([4 * p, 2 * p])

        def chk(ins, o):
            x = val(ins[0]) - 2 * val(ins[1])
            norm_val(o[:N], 4 * p, x + 4 * p if x < 0 else x)
    elif op == SUB_LAZY8:
        recs = one([2 * p, 4 * p])
        t8 = f.top(8 * p)
        recs += [[L(a), L(((t8 - 1) << f.TOP) | low)] for a in (0, 1, 2 * p - 1) for low in (0, (1 << f.TOP) - 1)]   # b_top < top(8p)

        def chk(ins, o):
            assert all(int(x) < 3 << B for x in o[:N])
            assert val(o[:N]) == val(ins[0]) - val(ins[1]) + 8 * p
    elif op in (NEG_LAZY, NEG_LAZY_K4, NEG_LAZY_K8):
        k = {NEG_LAZY: 4, NEG_LAZY_K4: 4, NEG_LAZY_K8: 8}[op]
        recs = one([2 * p if op == NEG_LAZY else (k - 1) * p])

        def chk(ins, o):
            assert all(int(x) < 1 << 30 for x in o[:N])
            assert val(o[:N]) == k * p - val(ins[0])
    elif op == ADD_NOSEL:
        recs = one([6 * p, 6 * p], max_edges=30)
        chk = lambda ins, o: norm_val(o[:N], 12 * p, val(ins[0]) + val(ins[1]))  # noqa: E731
    elif op == DBL_LAZY:
        recs = one([6 * p])

        def chk(ins, o):
            assert [int(x) for x in o[:N]] == [2 * int(x) for x in ins[0]] and all(int(x) < 1 << 30 for x in o[:N])
    elif op == FROM_CANONICAL:
        top = 1 << (32 * f.W)
        rnd = random.Random(seed)
        xs = sorted({0, 1, p - 1, p, p + 1, 2 * p, top - 1, top - p, top - 2, (top // p) * p, (top // p) * p - 1}) + \
            [rand_below(rnd, top) for _ in range(2000)]
        words = lambda x: [(x >> (32 * i)) & 0xFFFFFFFF for i in range(f.W)]  # noqa: E731
        recs = [[words(x)] for x in xs]

        def chk(ins, o):
            x = sum(int(w) << (32 * i) for i, w in enumerate(ins[0]))
            norm_val(o[:N], 2 * p, f.mont(val(L(x % (1 << (32 * f.W)))) * (f.R * f.R % p)))
    elif op == TO_CANONICAL:
        recs = one([2 * p])

        def chk(ins, o):
            got = sum(int(w) << (32 * i) for i, w in enumerate(o[:f.W]))
            assert got == val(ins[0]) * f.Rinv % p
    elif op in (FP2_MUL, FP2_SQR, FP2_INV, FP2_MUL_REL4, FP2_MUL_REL8, FP2_SQR_REL4, FP2_SQR_REL8):
        rnd = random.Random(seed)
        e = edges(f, 2)
        comp = {FP2_MUL: (2, 2, 2, 2), FP2_SQR: (2, 2), FP2_INV: (2, 2), FP2_MUL_REL4: (2, 2, 2, 2), FP2_MUL_REL8: (6, 6, 2, 2),
                FP2_SQR_REL4: (4, 4), FP2_SQR_REL8: (6, 6)}[op]
        tup = [tuple(rand_below(rnd, k * p) for k in comp) for _ in range(2000)]
        sub = e[:: max(1, len(e) // 6)] + [2 * p - 1]
        import itertools
        if len(comp) == 2:
            tup += list(itertools.product(*[[v for v in edges(f, k)] for k in comp]))
        else:
            tup += list(itertools.product(sub, sub, sub, sub))
            tup += [tuple(k * p - 1 for k in comp), tuple(k * p - 1 - rnd.randrange(1 << 20) for k in comp)]

        def fits(t):
            if op == FP2_MUL_REL4 or op == FP2_MUL_REL8:
                k = 4 if op == FP2_MUL_REL4 else 8
                a0, a1, b0, b1 = t
                return a1 < (k - 1) * p and a0 * b0 + k * p * b1 <= f.R * p and a0 * b1 + a1 * b0 <= f.R * p
            if op in (FP2_SQR_REL4, FP2_SQR_REL8):
                kd = 4 if op == FP2_SQR_REL4 else 8
                a0, a1 = t
                return a1 < kd * p and (a0 + a1) * (a0 - a1 + kd * p) <= f.R * p and 2 * a0 * a1 <= f.R * p
            return True
        recs = [[L(v) for v in t] for t in tup if fits(t)]

        def add2(a, b):
            s = a + b
            return s - 2 * p if s >= 2 * p else s

        def sub2(a, b):
            s = a - b
            return s + 2 * p if s < 0 else s

        def chk(ins, o):
            a0, a1 = val(ins[0]), val(ins[1])
            c0, c1 = norm_val(o[:N], 2 * p), norm_val(o[N:2 * N], 2 * p)
            if op in (FP2_MUL, FP2_MUL_REL4, FP2_MUL_REL8):
                k = {FP2_MUL: 4, FP2_MUL_REL4: 4, FP2_MUL_REL8: 8}[op]
                b0, b1 = val(ins[2]), val(ins[3])
                assert (c0, c1) == (f.mont(a0 * b0 + (k * p - a1) * b1), f.mont(a0 * b1 + a1 * b0))
            elif op == FP2_SQR:
                t1 = f.mont(a0 * a1)
                assert (c0, c1) == (f.mont(add2(a0, a1) * sub2(a0, a1)), add2(t1, t1))
            elif op == FP2_INV:
                x0, x1 = a0 * f.Rinv % p, a1 * f.Rinv % p
                d = (x0 * x0 + x1 * x1) % p
                e0, e1 = (0, 0) if d == 0 else (x0 * pow(d, -1, p) % p, -x1 * pow(d, -1, p) % p)
                assert (c0 % p, c1 % p) == (e0 * f.R % p, e1 * f.R % p)
            else:
                kd = 4 if op == FP2_SQR_REL4 else 8
                assert (c0, c1) == (f.mont((a0 + a1) * (a0 - a1 + kd * p)), f.mont(2 * a0 * a1))
    elif op in (LZ_SUB_18_29, LZ_SUB_36_30):
        rnd = random.Random(seed)
        if op == LZ_SUB_18_29:
            recs = [[L(a), L(b)] for a, b in tuples(f, [9 * p, 9 * p], seed, max_edges=30)]
        else:   # operands are limb-wise sums of two normalised values below 9p (limbs < 2^30, value < 18p)
            e = edges(f, 9)
            sums = [limbwise_add(L(x), L(y)) for x, y in zip(e, reversed(e))] + [limbwise_add(L(9 * p - 1), L(9 * p - 1))]
            sums += [limbwise_add(L(rand_below(rnd, 9 * p)), L(rand_below(rnd, 9 * p))) for _ in range(60)]
            recs = [[a, b] for a in sums for b in sums]
        k, bits, lim = (18, 29, 3 << B) if op == LZ_SUB_18_29 else (36, 30, 5 << B)

        def chk(ins, o):
            assert all(int(x) < lim for x in o[:N])
            assert val(o[:N]) == val(ins[0]) - val(ins[1]) + k * p < (k * 3 // 2) * p
    elif op == LZ_NORM:
        rnd = random.Random(seed)
        recs = [[[rnd.randrange(1 << 31) for _ in range(N - 1)] + [rnd.randrange(1 << 28)]] for _ in range(2000)]
        recs += [[[(1 << 31) - 1] * (N - 1) + [0]], [[(1 << 31) - 1] * N], [[0] * N]]
        prods = [rand_below(rnd, 2 * p) for _ in range(400)]   # the kernel's use: a sum of two products (< 2p each)
        recs += [[limbwise_add(L(x), L(y))] for x, y in zip(prods, reversed(prods))] + [[limbwise_add(L(2 * p - 1), L(2 * p - 1))]]
        chk = lambda ins, o: norm_val(o[:N], 1 << (f.TOP + 32), val(ins[0]))  # noqa: E731
    elif op in (LZ_REDUCE8, LZ_REDUCE2, LZ_CANONICAL):
        rnd = random.Random(seed)
        u = 8 if op == LZ_REDUCE8 else 2
        if op == LZ_REDUCE8:   # limb-wise sums of up to four normalised values below 9p: limbs < 2^31, value < 36p
            e = edges(f, 9)
            recs = [[limbwise_add(*[L(x) for x in t])] for t in zip(e, reversed(e), e[1:] + e[:1], e[2:] + e[:2])]
            recs += [[limbwise_add(L(x), L(y))] for x, y in zip(e, reversed(e))]
            recs += [[limbwise_add(*[L(rand_below(rnd, 9 * p)) for _ in range(4)])] for _ in range(2000)]
            recs += [[limbwise_add(*[L(9 * p - 1)] * 4)], [limbwise_add(*[L(9 * p - 1 - rnd.randrange(1 << 20))] * 4)]]
        else:
            recs = [[L(v)] for v in edges(f, 9)] + [[L(rand_below(rnd, 9 * p))] for _ in range(2000)]

        def chk(ins, o):
            a = val(ins[0])
            if op == LZ_CANONICAL:
                norm_val(o[:N], p, a % p)
            else:
                v = norm_val(o[:N], (109 * u * p) // 100)
                assert (a - v) % (u * p) == 0 and 0 <= (a - v) // (u * p) <= 4, (a, v)
    else:
        raise AssertionError(op)
    return recs, chk


def host_ops(f):
    ops = [op for op in range(G1_STEP) if not (op == MUL4 and f.N > 9)]
    if f.fid in (0, 2):
        ops = [op for op in ops if not LZ_SUB_18_29 <= op <= LZ_CANONICAL]
    else:
        ops = [op for op in ops if not FP2_MUL <= op <= FP2_SQR_REL8]
    return ops


FIELD_OPS = [(f, op) for f in FIELDS for op in host_ops(f)]


def check_records(f, op, recs, out, chk):
    for i, ins in enumerate(recs):
        try:
            chk(ins, out[i])
        except AssertionError as e:
            raise AssertionError(f"{f} {OP_NAMES[op]} record {i}: in {[hex(val(x)) for x in ins]} out {[hex(int(x)) for x in out[i][:2 * f.N]]}: {e}") from None


# ---- builds ---------------------------------------------------------------------------------------------------------------------
def build_host(dst, ubsan=False):
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-x", "c++", "-o", str(dst), SRC]
    if ubsan:
        cmd[1:1] = ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(cmd, check=True, timeout=600)
    return str(dst)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return Harness(build_host(tmp_path_factory.mktemp("fe_host") / "field_edges_host.so"))


@pytest.mark.parametrize("f,op", FIELD_OPS, ids=[f"{f.name.replace(' ', '_')}-{OP_NAMES[op]}" for f, op in FIELD_OPS])
def test_host_field_ops(host, f, op):
    recs, chk = field_cases(f, op, 1000 + 50 * f.fid + op)
    out = host.run(f, op, pack(f, recs))
    check_records(f, op, recs, out, chk)


def test_sub_lazy8_outside_its_contract(host):
    """fp_sub_lazy8 is exact for b_top < top(8p) only: the top limb of 8p does not borrow, so a = 0 against a b < 8p whose top
    limb equals top(8p) wraps the result's top limb (host build only: never sent to the device)"""
    for f in FIELDS:
        t8 = f.top(8 * f.p)
        b = t8 << f.TOP
        assert b < 8 * f.p
        out = host.run(f, SUB_LAZY8, pack(f, [[f.limbs(0), f.limbs(b)]]))[0]
        assert int(out[f.N - 1]) >= 1 << 31, "expected the top limb to wrap"
        assert val(out[:f.N]) != 8 * f.p - b
        # one step inside the corrected contract is exact
        b -= 1
        out = host.run(f, SUB_LAZY8, pack(f, [[f.limbs(0), f.limbs(b)]]))[0]
        assert val(out[:f.N]) == 8 * f.p - b


_UBSAN_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import test_field_edges as T
h = T.Harness({lib!r})
for f, op in T.FIELD_OPS:
    recs, chk = T.field_cases(f, op, 1000 + 50 * f.fid + op)
    T.check_records(f, op, recs, h.run(f, op, T.pack(f, recs)), chk)
for f in T.FQ:
    T.run_step_cases(h, f, T.G2_STEP, 2)
print("ubsan-clean")
"""


def test_host_build_under_ubsan_is_clean(tmp_path):
    """the same records through a -fsanitize=undefined build in a child process: signed carry chains at the edges must not
    overflow (the child aborts on the first report)"""
    lib = build_host(tmp_path / "field_edges_ubsan.so", ubsan=True)
    code = _UBSAN_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), lib=lib)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=1200, env=env)
    assert res.returncode == 0 and "ubsan-clean" in res.stdout and "runtime error" not in res.stderr, res.stderr[-4000:]


# ---- the relaxed bucket step ----------------------------------------------------------------------------------------------------
class StepRef:
    """madd-2008-s / mdbl-2008-s-1 on Montgomery representatives (every product carries 1/R), for Fp (d = 1) and Fp2 (d = 2)"""

    def __init__(self, f, d):
        self.f, self.p, self.d = f, f.p, d

    def mul(self, a, b):
        p, ri = self.p, self.f.Rinv
        if self.d == 1:
            return (a[0] * b[0] * ri % p,)
        return ((a[0] * b[0] - a[1] * b[1]) * ri % p, (a[0] * b[1] + a[1] * b[0]) * ri % p)

    def sub(self, a, b):
        return tuple((x - y) % self.p for x, y in zip(a, b))

    def add(self, a, b):
        return tuple((x + y) % self.p for x, y in zip(a, b))

    def zero(self, a):
        return all(x % self.p == 0 for x in a)

    def dbl_affine(self, x, y):
        if self.zero(y):
            return None
        U = self.add(y, y)
        V = self.mul(U, U)
        W = self.mul(U, V)
        S = self.mul(x, V)
        xx = self.mul(x, x)
        M = self.add(self.add(xx, xx), xx)
        X3 = self.sub(self.mul(M, M), self.add(S, S))
        Y3 = self.sub(self.mul(M, self.sub(S, X3)), self.mul(W, y))
        return X3, Y3, V, W

    def step(self, acc, x, y, neg):
        """expected (X, Y, ZZ, ZZZ) mod p, or None for infinity, or "same" for the sentinel / "init" for an empty accumulator"""
        X, Y, ZZ, ZZZ = acc
        if neg:
            y = tuple((-c) % self.p for c in y)
        U2, S2 = self.mul(x, ZZ), self.mul(y, ZZZ)
        P, Rr = self.sub(U2, X), self.sub(S2, Y)
        if self.zero(P):
            return self.dbl_affine(x, y) if self.zero(Rr) else None
        PP = self.mul(P, P)
        PPP = self.mul(P, PP)
        Q = self.mul(X, PP)
        X3 = self.sub(self.sub(self.mul(Rr, Rr), PPP), self.add(Q, Q))
        Y3 = self.sub(self.mul(Rr, self.sub(Q, X3)), self.mul(Y, PPP))
        return X3, Y3, self.mul(ZZ, PP), self.mul(ZZZ, PPP)


def step_record(f, d, acc, x, y, neg):
    """acc: 4 coordinates of d component ints (register form); x, y: d component ints (memory form)"""
    rec = np.zeros(16 * f.N, dtype=np.uint32)
    words = []
    for c in tuple(x) + tuple(y):
        words += [(c >> (32 * i)) & 0xFFFFFFFF for i in range(f.W)]
    rec[:len(words)] = words
    regs = [l for coord in acc for c in coord for l in f.limbs(c)]
    rec[4 * f.N:4 * f.N + len(regs)] = regs
    rec[12 * f.N] = 1 if neg else 0
    return rec


def unpack_acc(f, d, o):
    return tuple(tuple(val(o[(k * d + j) * f.N:(k * d + j + 1) * f.N]) for j in range(d)) for k in range(4))


def check_step(f, d, rec_in, o):
    acc, x, y, neg = rec_in
    got = unpack_acc(f, d, o)
    for k in range(4):
        for j in range(d):
            base = (k * d + j) * f.N
            assert is_norm(o[base:base + f.N])
            assert got[k][j] < (4 if k == 0 else 2) * f.p, (k, j, hex(got[k][j]))
    ref = StepRef(f, d)
    p = f.p
    if all(c == 0 for c in x + y):
        assert got == acc, "the (0, 0) sentinel must leave the accumulator alone"
        return got
    if all(c == 0 for c in acc[2]):
        ny = tuple(0 if c == 0 else 2 * p - c for c in y) if neg else tuple(y)
        one = tuple([f.R % p] + [0] * (d - 1))
        assert got == (tuple(x), ny, one, one), "empty accumulator"
        return got
    e = ref.step(acc, x, y, neg)
    if e is None:
        assert all(c == 0 for coord in got for c in coord), "infinity is written as zeros"
    else:
        assert tuple(tuple(c % p for c in coord) for coord in got) == e
    return got


def step_inputs(f, d, seed, n=600):
    """accumulator states and bases at the ends of the relaxed ranges, with the special branches"""
    rnd = random.Random(seed)
    p = f.p
    ref = StepRef(f, d)
    e4, e2 = edges(f, 4), edges(f, 2)

    def rv(k):
        m = rnd.random()
        if m < 0.2:
            return rnd.choice(e4 if k == 4 else e2)
        return rand_below(rnd, k * p)

    def comp(k):
        return tuple(rv(k) for _ in range(d))

    cases = []
    for i in range(n):
        acc = (comp(4), comp(2), comp(2), comp(2))
        x, y = comp(2), comp(2)
        neg = rnd.random() < 0.5
        kind = i % 10
        if kind == 1:
            x, y = (0,) * d, (0,) * d                                   # the (0, 0) sentinel
        elif kind == 2:
            acc = (acc[0], acc[1], (0,) * d, acc[3])                     # an empty accumulator
        elif kind in (3, 4, 5):                                          # same x: P + P / P - P, PP as 0 or p
            U2 = ref.mul(x, acc[2])
            acc = (tuple(c + rnd.choice([j for j in range(4) if c + j * p < 4 * p]) * p for c in U2),) + acc[1:]
            yy = tuple((-c) % p for c in y) if neg else y
            S2 = ref.mul(yy, acc[3])
            if kind != 5:
                acc = (acc[0], tuple(c + rnd.choice((0, p)) if c + p < 2 * p else c for c in S2), acc[2], acc[3])
        elif kind == 6:                                                  # a coordinate equal to p as the representative of zero
            j = rnd.randrange(4)
            acc = tuple(tuple(p for _ in range(d)) if k == j else acc[k] for k in range(4))
        cases.append((acc, x, y, neg))
    return cases


def run_step_cases(h, f, op, seed, n=600):
    d = 1 if op == G1_STEP else 2
    cases = step_inputs(f, d, seed, n)
    out = h.run(f, op, np.stack([step_record(f, d, *c) for c in cases]))
    for i, c in enumerate(cases):
        try:
            check_step(f, d, c, out[i])
        except AssertionError as e:
            raise AssertionError(f"{f} {OP_NAMES[op]} case {i} ({c}): {e}") from None
    # chains of 24 steps, each output fed back in
    rnd = random.Random(seed + 7)
    chains = 64
    accs = [((0,) * d,) * 4 for _ in range(chains)]
    last = [None] * chains
    for step in range(24):
        recs, ins = [], []
        for c in range(chains):
            x, y = tuple(rand_below(rnd, 2 * f.p) for _ in range(d)), tuple(rand_below(rnd, 2 * f.p) for _ in range(d))
            if step == 7:
                x, y = (0,) * d, (0,) * d
            if step in (11, 17) and last[c] is not None:
                x, y = last[c]
            neg = rnd.random() < 0.5
            last[c] = (x, y)
            ins.append((accs[c], x, y, neg))
            recs.append(step_record(f, d, accs[c], x, y, neg))
        out = h.run(f, op, np.stack(recs))
        for c in range(chains):
            accs[c] = check_step(f, d, ins[c], out[c])
    return out


def test_host_g2_relaxed_step(host):
    for f in FQ:
        run_step_cases(host, f, G2_STEP, 11 + f.fid)


# ---- device build --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device(tmp_path_factory, gpu):
    from helpers import build_device_harness
    return Harness(build_device_harness(SRC, tmp_path_factory.mktemp("fe_dev"), timeout=900))


@pytest.mark.gpu
@pytest.mark.parametrize("f", FIELDS, ids=[f.name.replace(" ", "_") for f in FIELDS])
def test_device_field_ops(host, device, f):
    """every field op on the device, limb for limb equal to the host build, inside each op's contract"""
    for op in host_ops(f):
        recs, chk = field_cases(f, op, 1000 + 50 * f.fid + op)
        arr = pack(f, recs)
        want, got = host.run(f, op, arr), device.run(f, op, arr)
        bad = np.flatnonzero((want != got).any(axis=1))
        assert bad.size == 0, f"{f} {OP_NAMES[op]}: device differs from host at records {bad[:8]}"
        check_records(f, op, recs, got, chk)


@pytest.mark.gpu
@pytest.mark.parametrize("f", FQ, ids=[f.name.replace(" ", "_") for f in FQ])
def test_device_bucket_step(host, device, f):
    """the relaxed bucket step of the MSM inner loop (xyzz_add_affine_mem): G1 (the F::RELAXED branch) against madd-2008-s on
    Montgomery representatives, G2 (relaxed2) likewise and limb-equal to the host build"""
    run_step_cases(device, f, G1_STEP, 21 + f.fid)
    dev = run_step_cases(device, f, G2_STEP, 31 + f.fid, n=300)
    hst = run_step_cases(host, f, G2_STEP, 31 + f.fid, n=300)
    assert (dev == hst).all()
