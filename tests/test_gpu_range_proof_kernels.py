"""GPU: the four entry points of csrc/rangeproof.hip and zk_ipa_round_seeded_dev (csrc/ipa.hip) against the integer contracts of
tests/range_proof_model.py, by ==.

Shapes (log_bits, log_N): one position; one value of one bit, two values of one bit, one value of two bits; 8 and 16 positions;
one and two workgroups with small and large values, 512 one-bit values, n = 128 (two limbs per value) with one and two values;
and one call of each entry point at (6, 19): the grid is capped at 1024 workgroups of 256 threads, so 2^19 is the first N at
which a thread takes a second item and steps its powers.  Every shape runs with every value pattern (0, 2^n - 1, alternating
bits, bits set above n, and at n = 128 bits 63, 64, 127) and with the challenges 1, r - 1, a value >= r and random ones, y = 1
among them; s_L, s_R hold 0 and r - 1."""

import itertools
import random

import numpy as np
import pytest

import range_proof_model as M
from zksnake_amd import _native as N
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from zksnake_amd.frvec import DevVec, FrOps

pytestmark = pytest.mark.gpu

FIELDS = (("BN254", BN254_SCALAR_FIELD), ("BLS12_381", BLS12_381_SCALAR_FIELD))
IDS = [f[0] for f in FIELDS]
SHAPES = [(0, 0), (0, 1), (1, 1), (3, 3), (2, 4), (3, 8), (6, 9), (0, 9), (7, 7), (7, 8)]
SECOND_ITEM = (6, 19)      # 1024 workgroups x 256 threads = 2^18 threads
MASK128 = (1 << 128) - 1
_CACHE = {}


def patterns(n):
    full = (1 << n) - 1
    alt = int("10" * 64, 2) & full
    above = (0b1011 << n) & MASK128            # bits at and above n: ignored
    out = [0, full, alt, (full ^ alt) | above, above, 1 | above, (1 << (n - 1)) | above]
    if n == 128:
        out += [1 << 63, 1 << 64, 1 << 127, (1 << 63) | (1 << 64) | (1 << 127), full ^ (1 << 64)]
    return out


def value_sets(log_bits, log_N):
    """lists of m values that between them put every pattern somewhere, at least four of them; then random values"""
    n, m = 1 << log_bits, 1 << (log_N - log_bits)
    pats = patterns(n)
    rnd = random.Random(1000 * log_bits + log_N)
    sets = []
    for p in range(max(4, -(-len(pats) // m))):
        sets.append([pats[p * m + j] if p * m + j < len(pats) else rnd.getrandbits(128) for j in range(m)])
    return sets


def challenge_sets(p, seed):
    """(y, z, x) as handed in: 1, r - 1 and a value >= r in every position once, then random"""
    rnd = random.Random(seed)
    return [(1, p - 1, p + 5), (p - 1, p + 2, 1), (p + 5, 1, p - 1), tuple(rnd.randrange(2, p) for _ in range(3))]


def s_table(p, count, seed):
    """s_L || s_R with 0 and r - 1 in both halves (shared, never modified)"""
    key = (p, count, seed)
    if key not in _CACHE:
        rnd = random.Random(7 * count + seed + (p & 0xFF))
        t = [rnd.randrange(p) for _ in range(count)]
        t[0], t[-1] = p - 1, 0
        if count >= 4:
            t[count // 2 - 1], t[count // 2] = 0, p - 1
        _CACHE[key] = t
    return _CACHE[key]


def geometric(p, n, g, first):
    return list(itertools.accumulate(itertools.repeat(g, n - 1), lambda x, y: x * y % p, initial=first % p))


def raw(values):
    return N.ints_to_limbs(list(values), 4)


def one(value):
    return N.u64p(raw([value]))


def upload(values):
    vec = DevVec(len(values), zero=False)
    vec.upload(raw(values))
    return vec


def upload_values(values):
    """m x 2 limbs; the buffer is a whole number of 32-byte elements"""
    vec = DevVec((len(values) + 1) // 2, zero=False)
    vec.buf.upload(N.ints_to_limbs([v & MASK128 for v in values], 2))
    return vec


def ints(vec, count=None):
    return N.limbs_to_ints(vec.download(count))


def poisoned(gpu, n):
    vec = DevVec(n, zero=False)
    N.check(gpu.zk_dev_memset(vec.ptr(), 0xA5, 32 * n))
    return vec


def big_case(p):
    """(values, s) at the size where a thread takes a second item: patterns, then a cheap spread of 64-bit values"""
    lb, ln = SECOND_ITEM
    key = ("big", p)
    if key not in _CACHE:
        m, size = 1 << (ln - lb), 1 << ln
        pats = patterns(1 << lb)
        values = pats + [(0x9E3779B97F4A7C15 * j) & MASK128 for j in range(len(pats), m)]
        s = geometric(p, 2 * size, 3, 5)
        s[1], s[size], s[-1] = 0, p - 1, 0
        _CACHE[key] = (values, s, upload_values(values), upload(s))
    return _CACHE[key]


# ---- zk_rp_bits_dev ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_bits,log_N", SHAPES)
@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_bits(gpu, name, p, log_bits, log_N):
    ops, size = FrOps(p), 1 << log_N
    for values in value_sets(log_bits, log_N):
        d_values, out = upload_values(values), poisoned(gpu, 2 * size)
        N.check(gpu.zk_rp_bits_dev(ops.cid, log_bits, log_N, d_values.ptr(), out.ptr(), None))
        assert ints(out) == M.bits_contract(log_bits, log_N, values, p)


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_bits_where_a_thread_takes_a_second_item(gpu, name, p):
    lb, ln = SECOND_ITEM
    values, _, d_values, _ = big_case(p)
    out = poisoned(gpu, 2 << ln)
    N.check(gpu.zk_rp_bits_dev(FrOps(p).cid, lb, ln, d_values.ptr(), out.ptr(), None))
    assert (out.download() == raw(M.bits_contract(lb, ln, values, p))).all()


# ---- zk_rp_poly_dev ------------------------------------------------------------------------------------------------------------
def call_poly(gpu, cid, lb, ln, d_values, d_s, y, z):
    t = np.full((3, 4), 0x77, dtype=np.uint64)
    N.check(gpu.zk_rp_poly_dev(cid, lb, ln, d_values.ptr(), d_s.ptr(), one(y), one(z), N.u64p(t), None))
    return tuple(N.limbs_to_ints(t))


@pytest.mark.parametrize("log_bits,log_N", SHAPES)
@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_poly(gpu, name, p, log_bits, log_N):
    ops, size = FrOps(p), 1 << log_N
    s = s_table(p, 2 * size, 1)
    d_s = upload(s)
    for i, values in enumerate(value_sets(log_bits, log_N)):
        y, z, _ = challenge_sets(p, log_N)[(i + log_N) % 4]
        got = call_poly(gpu, ops.cid, log_bits, log_N, upload_values(values), d_s, y, z)
        assert got == M.poly_contract(log_bits, log_N, values, s, y, z, p), (i, y, z)
    assert ints(d_s) == s, "s_L || s_R is read only"
    # twice the same: fixed-order sums
    assert call_poly(gpu, ops.cid, log_bits, log_N, upload_values(values), d_s, y, z) == got


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_poly_where_a_thread_takes_a_second_item(gpu, name, p):
    lb, ln = SECOND_ITEM
    values, s, d_values, d_s = big_case(p)
    y, z = 0x1234567890ABCDEF1234567890ABCDEF % p, p + 3
    assert call_poly(gpu, FrOps(p).cid, lb, ln, d_values, d_s, y, z) == M.poly_contract(lb, ln, values, s, y, z, p)


@pytest.mark.parametrize("log_bits,log_N", [(3, 3), (3, 9)])
@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_poly_with_every_term_at_the_top_of_the_range(gpu, name, p, log_bits, log_N):
    """every bit set, s_L = s_R = r - 1 everywhere, y = z = r - 1.  N is a power of two, so no size is "two workgroups and one
    element"; two sizes stand in for it: 512 positions (two full workgroups, and the combine reads two of the 256 partial triples
    it can take) and 8 (a workgroup that sums with 248 idle lanes).  With y = z = -1: l0 = 2, l1 = -1, r0[k] = -(-1)^k + (-1)^j 2^i,
    r1[k] = -(-1)^k, and over an even N the alternating sums vanish: t0 = 2 S, t1 = -S, t2 = 0 with S = (2^n - 1) (m mod 2)."""
    n, m = 1 << log_bits, 1 << (log_N - log_bits)
    values, s = [MASK128] * m, [p - 1] * (2 << log_N)
    got = call_poly(gpu, FrOps(p).cid, log_bits, log_N, upload_values(values), upload(s), p - 1, p - 1)
    assert got == M.poly_contract(log_bits, log_N, values, s, p - 1, p - 1, p)
    total = ((1 << n) - 1) * (m % 2)
    assert (n * m) % 2 == 0 and got == (2 * total % p, -total % p, 0)


# ---- zk_rp_eval_dev ------------------------------------------------------------------------------------------------------------
def call_eval(gpu, cid, lb, ln, d_values, d_s, y, y_inv, z, x, d_ab, d_w):
    return gpu.zk_rp_eval_dev(cid, lb, ln, d_values.ptr(), d_s.ptr(), one(y), one(y_inv), one(z), one(x), d_ab.ptr(), d_w.ptr(), None)


@pytest.mark.parametrize("log_bits,log_N", SHAPES)
@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_eval(gpu, name, p, log_bits, log_N):
    ops, size = FrOps(p), 1 << log_N
    s = s_table(p, 2 * size, 2)
    d_s = upload(s)
    for i, values in enumerate(value_sets(log_bits, log_N)):
        y, z, x = challenge_sets(p, 10 + log_N)[(i + log_N) % 4]
        y_inv = pow(y, -1, p) + (p if i % 2 else 0)      # reduced on entry like every host scalar
        d_ab, d_w = poisoned(gpu, 2 * size), poisoned(gpu, size)
        N.check(call_eval(gpu, ops.cid, log_bits, log_N, upload_values(values), d_s, y, y_inv, z, x, d_ab, d_w))
        want_ab, want_w = M.eval_contract(log_bits, log_N, values, s, y, y_inv, z, x, p)
        assert ints(d_ab) == want_ab, (i, y, z, x)
        assert ints(d_w) == want_w, (i, y)
        # l || r at x are consistent with the coefficients of t(X)
        t0, t1, t2 = M.poly_contract(log_bits, log_N, values, s, y, z, p)
        assert sum(a * b for a, b in zip(want_ab[:size], want_ab[size:])) % p == (t0 + t1 * x + t2 * x * x) % p
    assert ints(d_s) == s
    # y * y_inv = 1 is not checked: the weights are the powers of what was handed in
    N.check(call_eval(gpu, ops.cid, log_bits, log_N, upload_values(values), d_s, y, 3, z, x, d_ab, d_w))
    assert ints(d_w) == M.powers(3, size, p) and ints(d_ab) == want_ab


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_eval_where_a_thread_takes_a_second_item(gpu, name, p):
    lb, ln = SECOND_ITEM
    values, s, d_values, d_s = big_case(p)
    y, z, x = p - 2, 0xFEDCBA9876543210FEDCBA9876543210 % p, p + 9
    y_inv = pow(y, -1, p)
    d_ab, d_w = poisoned(gpu, 2 << ln), poisoned(gpu, 1 << ln)
    N.check(call_eval(gpu, FrOps(p).cid, lb, ln, d_values, d_s, y, y_inv, z, x, d_ab, d_w))
    want_ab, want_w = M.eval_contract(lb, ln, values, s, y, y_inv, z, x, p)
    assert (d_ab.download() == raw(want_ab)).all() and (d_w.download() == raw(want_w)).all()


# ---- zk_rp_verify_scalars_dev --------------------------------------------------------------------------------------------------
def round_challenges(p, count, seed):
    rnd = random.Random(seed)
    special = [1, p - 1, p + 5]
    return [special[i] if i < len(special) else rnd.randrange(1, p) for i in range(count)]


def call_verify_scalars(gpu, cid, lb, ln, us, a, b, y_inv, z, out, p):
    u_l = raw(us) if us else None
    ui_l = raw([pow(u, -1, p) for u in us]) if us else None
    return gpu.zk_rp_verify_scalars_dev(cid, lb, ln, N.u64p(u_l) if us else None, N.u64p(ui_l) if us else None, one(a), one(b), one(y_inv), one(z),
                                        out.ptr(), None)


@pytest.mark.parametrize("log_bits,log_N", SHAPES + [SECOND_ITEM])
@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_verify_scalars(gpu, name, p, log_bits, log_N):
    ops, size = FrOps(p), 1 << log_N
    us = round_challenges(p, log_N, seed=30 + log_N)
    sets = challenge_sets(p, 20 + log_N) if log_N <= 9 else challenge_sets(p, 20 + log_N)[3:]
    for i, (y_inv, z, _) in enumerate(sets):
        a, b = ((p - 1, p + 3), (0x1F2E3D4C5B6A79880102030405060708090A0B0C0D0E0F % p, (1 << 256) - 1), (0, 1), (1, 0))[(i + log_N) % 4]
        out = poisoned(gpu, 2 * size)
        N.check(call_verify_scalars(gpu, ops.cid, log_bits, log_N, us, a, b, y_inv, z, out, p))
        want = M.verify_scalars_contract(log_bits, log_N, us, a, b, y_inv, z, p)
        assert (out.download() == raw(want)).all(), (i, y_inv, z, a, b)


# ---- zk_ipa_round_seeded_dev ---------------------------------------------------------------------------------------------------
def call_round(gpu, fn, cid, log_n, k, a, b, s, s_inv, weight, u, scal_l, scal_r, p):
    """one round through zk_ipa_round_seeded_dev (weight: a DevVec, None for NULL) or zk_ipa_round_dev (fn = the plain entry
    point, which has no weight argument)"""
    cross = np.zeros((2, 4), dtype=np.uint64)
    u_l = None if u is None else raw([u])
    ui_l = None if u is None else raw([pow(u, -1, p)])
    args = [cid, log_n, k, a.ptr(), b.ptr(), s.ptr(), s_inv.ptr()]
    if fn is gpu.zk_ipa_round_seeded_dev:
        args.append(None if weight is None else weight.ptr())
    args += [None if u is None else N.u64p(u_l), None if u is None else N.u64p(ui_l), scal_l.ptr(), scal_r.ptr(), N.u64p(cross), None]
    return fn(*args), tuple(N.limbs_to_ints(cross))


@pytest.mark.parametrize("log_n", [1, 3, 9, 19])
@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_seeded_round(gpu, name, p, log_n):
    ops, n = FrOps(p), 1 << log_n
    y_inv = pow(0xABCDEF0123456789 % p, -1, p)
    weight = geometric(p, n, y_inv, 1)
    a, b = geometric(p, n, 3, 5), geometric(p, n, 7, p - 1)
    a[n - 1], b[1] = 0, p - 1
    s, s_inv = [None] * n, [None] * n
    d_a, d_b, d_w = upload(a), upload(b), upload(weight)
    d_s, d_si = poisoned(gpu, n), poisoned(gpu, n)
    for k, u in ((0, None), (1, (p + 5) if log_n == 3 else 0x1234567890ABCDEF1234567890ABCDEF % p)):
        if k > log_n:
            break
        want = M.seeded_round_contract(log_n, k, a, b, s, s_inv, weight if k == 0 else None, None if u is None else u % p,
                                       None if u is None else pow(u, -1, p), p)
        d_l, d_r = poisoned(gpu, 2 * n), poisoned(gpu, 2 * n)
        st, cross = call_round(gpu, gpu.zk_ipa_round_seeded_dev, ops.cid, log_n, k, d_a, d_b, d_s, d_si, d_w if k == 0 else None, u, d_l, d_r, p)
        N.check(st)
        assert (d_a.download() == raw(a)).all() and (d_b.download() == raw(b)).all()
        assert (d_s.download() == raw(s)).all() and (d_si.download() == raw(s_inv)).all()
        if want is None:
            continue
        assert cross == want[2]
        assert (d_l.download() == raw(want[0])).all() and (d_r.download() == raw(want[1])).all()
    assert (d_w.download() == raw(weight)).all(), "the weights are read only"


@pytest.mark.parametrize("log_n", [1, 3, 9])
@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_seeded_round_without_weights_is_the_plain_round(gpu, name, p, log_n):
    ops, n = FrOps(p), 1 << log_n
    a, b = s_table(p, n, 3), s_table(p, n, 4)
    state = []
    for fn in (gpu.zk_ipa_round_seeded_dev, gpu.zk_ipa_round_dev):
        d_a, d_b, d_s, d_si = upload(a), upload(b), poisoned(gpu, n), poisoned(gpu, n)
        got = []
        for k, u in ((0, None), (1, p - 1)):
            d_l, d_r = poisoned(gpu, 2 * n), poisoned(gpu, 2 * n)
            st, cross = call_round(gpu, fn, ops.cid, log_n, k, d_a, d_b, d_s, d_si, None, u, d_l, d_r, p)
            N.check(st)
            got.append([cross] + [ints(v) for v in (d_a, d_b, d_s, d_si, d_l, d_r)])
        state.append(got)
    assert state[0] == state[1]


# ---- arguments -----------------------------------------------------------------------------------------------------------------
class Arena:
    """one device block cut into named parts, every byte known, so that 'nothing was written' is one comparison"""

    def __init__(self, gpu, sizes):
        self.total = sum(sizes.values())
        self.vec = DevVec(self.total, zero=False)
        N.check(gpu.zk_dev_memset(self.vec.ptr(), 0x5A, 32 * self.total))
        self.at, offset = {}, 0
        for key, count in sizes.items():
            self.at[key] = offset
            offset += count
        self.before = None

    def ptr(self, key, plus=0):
        return self.vec.ptr(self.at[key]) + 32 * plus

    def put(self, key, limbs):
        self.vec.buf.upload(limbs, 32 * self.at[key])

    def freeze(self):
        self.before = self.vec.download()

    def untouched(self):
        return (self.vec.download() == self.before).all()


def arena(gpu, p, lb, ln):
    size, m = 1 << ln, 1 << (ln - lb)
    ar = Arena(gpu, {"values": (m + 1) // 2, "s": 2 * size, "out": 2 * size, "w": size})
    ar.put("values", N.ints_to_limbs([5] * m, 2))
    ar.put("s", raw(s_table(p, 2 * size, 5)))
    ar.freeze()
    return ar


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_bits_bad_arguments(gpu, name, p):
    cid, lb, ln = FrOps(p).cid, 2, 4
    ar = arena(gpu, p, lb, ln)
    V, O = ar.ptr("values"), ar.ptr("out")
    for what, args in {
        "null values": (lb, ln, None, O), "null out": (lb, ln, V, None), "log_bits < 0": (-1, ln, V, O), "log_bits > 7": (8, 8, V, O),
        "log_N < log_bits": (3, 2, V, O), "log_N > 22": (lb, N.IPA_MAX_LOG + 1, V, O), "out over values": (lb, ln, V, V),
        "values inside out": (lb, ln, O + 32 * 5, O),
    }.items():
        assert gpu.zk_rp_bits_dev(cid, *args, None) == N.ZK_ERR_ARG, what
        assert ar.untouched(), what
    assert gpu.zk_rp_bits_dev(9, lb, ln, V, O, None) == N.ZK_ERR_ARG, "unknown curve"
    assert ar.untouched()
    assert gpu.zk_rp_bits_dev(cid, lb, ln, V, O, None) == N.ZK_OK


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_poly_bad_arguments(gpu, name, p):
    cid, lb, ln = FrOps(p).cid, 2, 4
    ar = arena(gpu, p, lb, ln)
    V, S = ar.ptr("values"), ar.ptr("s")
    t = np.full((3, 4), 0x77, dtype=np.uint64)
    Y, Z, T = one(5), one(7), N.u64p(t)
    for what, args in {
        "null values": (lb, ln, None, S, Y, Z, T), "null s": (lb, ln, V, None, Y, Z, T), "null y": (lb, ln, V, S, None, Z, T),
        "null z": (lb, ln, V, S, Y, None, T), "null t_out": (lb, ln, V, S, Y, Z, None), "log_bits < 0": (-1, ln, V, S, Y, Z, T),
        "log_bits > 7": (8, 8, V, S, Y, Z, T), "log_N < log_bits": (3, 2, V, S, Y, Z, T), "log_N > 22": (lb, N.IPA_MAX_LOG + 1, V, S, Y, Z, T),
    }.items():
        assert gpu.zk_rp_poly_dev(cid, *args, None) == N.ZK_ERR_ARG, what
        assert ar.untouched() and (t == 0x77).all(), what
    assert gpu.zk_rp_poly_dev(9, lb, ln, V, S, Y, Z, T, None) == N.ZK_ERR_ARG, "unknown curve"
    assert (t == 0x77).all()
    assert gpu.zk_rp_poly_dev(cid, lb, ln, V, S, Y, Z, T, None) == N.ZK_OK
    assert ar.untouched(), "every device buffer of the call is read only"


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_eval_bad_arguments(gpu, name, p):
    cid, lb, ln = FrOps(p).cid, 2, 4
    size = 1 << ln
    ar = arena(gpu, p, lb, ln)
    V, S, O, W = ar.ptr("values"), ar.ptr("s"), ar.ptr("out"), ar.ptr("w")
    Y, YI, Z, X = one(5), one(pow(5, -1, p)), one(7), one(9)
    for what, args in {
        "null values": (lb, ln, None, S, Y, YI, Z, X, O, W), "null s": (lb, ln, V, None, Y, YI, Z, X, O, W),
        "null y": (lb, ln, V, S, None, YI, Z, X, O, W), "null y_inv": (lb, ln, V, S, Y, None, Z, X, O, W),
        "null z": (lb, ln, V, S, Y, YI, None, X, O, W), "null x": (lb, ln, V, S, Y, YI, Z, None, O, W),
        "null ab": (lb, ln, V, S, Y, YI, Z, X, None, W), "null h_weight": (lb, ln, V, S, Y, YI, Z, X, O, None),
        "log_bits < 0": (-1, ln, V, S, Y, YI, Z, X, O, W), "log_bits > 7": (8, 8, V, S, Y, YI, Z, X, O, W),
        "log_N < log_bits": (3, 2, V, S, Y, YI, Z, X, O, W), "log_N > 22": (lb, N.IPA_MAX_LOG + 1, V, S, Y, YI, Z, X, O, W),
        "ab over s": (lb, ln, V, S, Y, YI, Z, X, S, W), "h_weight inside ab": (lb, ln, V, S, Y, YI, Z, X, O, O + 32 * (2 * size - 1)),
        "h_weight over s": (lb, ln, V, S, Y, YI, Z, X, O, S + 32 * size), "ab over values": (lb, ln, V, S, Y, YI, Z, X, V, W),
        "h_weight over values": (lb, ln, V, S, Y, YI, Z, X, O, V),
    }.items():
        assert gpu.zk_rp_eval_dev(cid, *args, None) == N.ZK_ERR_ARG, what
        assert ar.untouched(), what
    assert gpu.zk_rp_eval_dev(9, lb, ln, V, S, Y, YI, Z, X, O, W, None) == N.ZK_ERR_ARG, "unknown curve"
    assert ar.untouched()
    assert gpu.zk_rp_eval_dev(cid, lb, ln, V, S, Y, YI, Z, X, O, W, None) == N.ZK_OK


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_verify_scalars_bad_arguments(gpu, name, p):
    cid, lb, ln = FrOps(p).cid, 2, 4
    ar = arena(gpu, p, lb, ln)
    O = ar.ptr("out")
    us = raw([3, 5, 7, 11])
    uis = raw([pow(u, -1, p) for u in (3, 5, 7, 11)])
    U, UI, A, B, YI, Z = N.u64p(us), N.u64p(uis), one(2), one(3), one(4), one(5)
    for what, args in {
        "null u": (lb, ln, None, UI, A, B, YI, Z, O), "null u_inv": (lb, ln, U, None, A, B, YI, Z, O), "null a": (lb, ln, U, UI, None, B, YI, Z, O),
        "null b": (lb, ln, U, UI, A, None, YI, Z, O), "null y_inv": (lb, ln, U, UI, A, B, None, Z, O), "null z": (lb, ln, U, UI, A, B, YI, None, O),
        "null out": (lb, ln, U, UI, A, B, YI, Z, None), "log_bits < 0": (-1, ln, U, UI, A, B, YI, Z, O), "log_bits > 7": (8, 8, U, UI, A, B, YI, Z, O),
        "log_N < log_bits": (3, 2, U, UI, A, B, YI, Z, O), "log_N > 22": (lb, N.IPA_MAX_LOG + 1, U, UI, A, B, YI, Z, O),
    }.items():
        assert gpu.zk_rp_verify_scalars_dev(cid, *args, None) == N.ZK_ERR_ARG, what
        assert ar.untouched(), what
    assert gpu.zk_rp_verify_scalars_dev(9, lb, ln, U, UI, A, B, YI, Z, O, None) == N.ZK_ERR_ARG, "unknown curve"
    assert ar.untouched()
    assert gpu.zk_rp_verify_scalars_dev(cid, lb, ln, U, UI, A, B, YI, Z, O, None) == N.ZK_OK
    # no rounds, no challenges
    assert gpu.zk_rp_verify_scalars_dev(cid, 0, 0, None, None, A, B, YI, Z, O, None) == N.ZK_OK
    assert N.limbs_to_ints(ar.vec.download(2, ar.at["out"])) == M.verify_scalars_contract(0, 0, [], 2, 3, 4, 5, p)


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_seeded_round_bad_arguments(gpu, name, p):
    cid, log_n, n = FrOps(p).cid, 3, 8
    ar = Arena(gpu, {"a": n, "b": n, "s": n, "s_inv": n, "l": 2 * n, "r": 2 * n, "w": n})
    ar.put("a", raw(s_table(p, n, 6)))
    ar.put("b", raw(s_table(p, n, 7)))
    ar.put("w", raw(geometric(p, n, 9, 1)))
    ar.freeze()
    pa, pb, ps, psi, pl, pr, pw = (ar.ptr(k) for k in ("a", "b", "s", "s_inv", "l", "r", "w"))
    cross = np.full((2, 4), 0x77, dtype=np.uint64)
    U, UI, C = one(5), one(pow(5, -1, p)), N.u64p(cross)
    for what, (k, *rest) in {
        "a weight at k = 1": (1, pa, pb, ps, psi, pw, U, UI, pl, pr, C),
        "a weight at k = log_n": (log_n, pa, pb, ps, psi, pw, U, UI, None, None, None),
        "the weights over a": (0, pa, pb, ps, psi, pa, None, None, pl, pr, C),
        "the weights inside s_inv": (0, pa, pb, ps, psi, psi + 32 * (n - 1), None, None, pl, pr, C),
        "the weights inside scal_L": (0, pa, pb, ps, psi, pl + 32 * (2 * n - 1), None, None, pl, pr, C),
        "scal_R over the weights": (0, pa, pb, ps, psi, pw, None, None, pl, pw, C),
        "u at k = 0": (0, pa, pb, ps, psi, pw, U, UI, pl, pr, C),
        "null a": (0, None, pb, ps, psi, pw, None, None, pl, pr, C),
        "null cross": (0, pa, pb, ps, psi, pw, None, None, pl, pr, None),
    }.items():
        assert gpu.zk_ipa_round_seeded_dev(cid, log_n, k, *rest, None) == N.ZK_ERR_ARG, what
        assert ar.untouched() and (cross == 0x77).all(), what
    assert gpu.zk_ipa_round_seeded_dev(9, log_n, 0, pa, pb, ps, psi, pw, None, None, pl, pr, C, None) == N.ZK_ERR_ARG, "unknown curve"
    assert ar.untouched()
    assert gpu.zk_ipa_round_seeded_dev(cid, log_n, 0, pa, pb, ps, psi, pw, None, None, pl, pr, C, None) == N.ZK_OK
    assert gpu.zk_ipa_round_seeded_dev(cid, log_n, 1, pa, pb, ps, psi, None, U, UI, pl, pr, C, None) == N.ZK_OK
