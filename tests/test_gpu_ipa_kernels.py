"""GPU: zk_ipa_round_dev and zk_ipa_verify_scalars_dev (csrc/ipa.hip) against the integer contracts of tests/ipa_model.py, by ==.

Sizes: log_n 1, 2, 3 (every index pattern of a short proof), 8 and 9 (one and two workgroups), each chained through every k of
a proof, and one call pair (k = 0, k = 1) at log_n = 19: the grid is capped at 1024 workgroups of 256 threads, so 2^19 is the
first n at which a thread of the pass over i < n (the s vectors and the MSM scalars, and the verifier's scalars) takes a second
item.  The fold (n >> k items) and the cross products (half of that) take a second item first at n = 2^20; one (k = 0, k = 1)
pair there checks a, b and the cross products."""

import itertools
import random

import numpy as np
import pytest

import ipa_model as M
from zksnake_amd import _native as N
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from zksnake_amd.frvec import DevVec, FrOps

pytestmark = pytest.mark.gpu

FIELDS = (("BN254", BN254_SCALAR_FIELD), ("BLS12_381", BLS12_381_SCALAR_FIELD))
IDS = [f[0] for f in FIELDS]
SIZES = (1, 2, 3, 8, 9)
SECOND_ITEM_LOG = 19      # 1024 workgroups x 256 threads = 2^18 threads
FOLD_SECOND_ITEM_LOG = 20
_TABLES = {}


def table(p, log_n, seed):
    """random table with the entries 0 and r-1 (shared by the tests, never modified)"""
    key = (p, log_n, seed)
    if key not in _TABLES:
        rnd = random.Random(100 * log_n + seed + (p & 0xFF))
        t = [rnd.randrange(p) for _ in range(1 << log_n)]
        t[-1] = p - 1
        t[0] = 0 if seed else p - 1
        if log_n > 2:
            t[3], t[len(t) // 2] = p - 1, 0
        _TABLES[key] = t
    return _TABLES[key]


def geometric(p, n, g, first):
    """first * g^j: 2^20 elements in a fraction of a second, and no two alike"""
    return list(itertools.accumulate(itertools.repeat(g, n - 1), lambda x, y: x * y % p, initial=first % p))


def challenges(p, count, seed):
    """(u as handed in, u mod r): 1, r-1, a value >= r, then random ones"""
    rnd = random.Random(seed)
    special = [1, p - 1, p + 5]
    raw = [special[i] if i < len(special) else rnd.randrange(1, p) for i in range(count)]
    return raw


def raw(values):
    return N.ints_to_limbs(list(values), 4)


def upload(values):
    vec = DevVec(len(values), zero=False)
    vec.upload(raw(values))
    return vec


def ints(vec, count=None):
    return N.limbs_to_ints(vec.download(count))


def poisoned(gpu, n):
    vec = DevVec(n, zero=False)
    N.check(gpu.zk_dev_memset(vec.ptr(), 0xA5, 32 * n))
    return vec


def call_round(gpu, ops, log_n, k, a, b, s, s_inv, u, scal_l, scal_r, p, want_cross=True):
    """one zk_ipa_round_dev; u: the challenge as handed in (None at k = 0).  Returns the status and the cross products."""
    cross = np.zeros((2, 4), dtype=np.uint64)
    u_l = None if u is None else raw([u])
    ui_l = None if u is None else raw([pow(u, -1, p)])
    st = gpu.zk_ipa_round_dev(ops.cid, log_n, k, a.ptr(), b.ptr(), s.ptr(), s_inv.ptr(), None if u is None else N.u64p(u_l),
                              None if u is None else N.u64p(ui_l), scal_l.ptr() if scal_l else None, scal_r.ptr() if scal_r else None,
                              N.u64p(cross) if want_cross else None, None)
    return st, tuple(N.limbs_to_ints(cross))


@pytest.mark.parametrize("log_n", SIZES)
@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_round_chained_through_a_proof(gpu, name, p, log_n):
    ops, n = FrOps(p), 1 << log_n
    a, b = list(table(p, log_n, 0)), list(table(p, log_n, 1))
    s, s_inv = [None] * n, [None] * n
    d_a, d_b = upload(a), upload(b)
    d_s, d_si = poisoned(gpu, n), poisoned(gpu, n)
    us = challenges(p, log_n, seed=log_n)
    u = None
    for k in range(log_n + 1):
        want = M.round_step(log_n, k, a, b, s, s_inv, None if u is None else u % p, None if u is None else pow(u, -1, p), p)
        if k == log_n:
            st, _ = call_round(gpu, ops, log_n, k, d_a, d_b, d_s, d_si, u, None, None, p, want_cross=False)
            N.check(st)
        else:
            d_l, d_r = poisoned(gpu, 2 * n), poisoned(gpu, 2 * n)   # the zero halves must really be written
            st, cross = call_round(gpu, ops, log_n, k, d_a, d_b, d_s, d_si, u, d_l, d_r, p)
            N.check(st)
            assert ints(d_l) == want[0], f"scal_L, round {k}"
            assert ints(d_r) == want[1], f"scal_R, round {k}"
            assert cross == want[2], f"cross products, round {k}"
            u = us[k]
        assert ints(d_a) == a and ints(d_b) == b, f"a, b after round {k}"
        assert ints(d_s) == s and ints(d_si) == s_inv, f"s, s_inv after round {k}"
    # the end of the chain: the proof's scalars, and the verifier's s vector
    assert s == M.s_vector([x % p for x in us], log_n, p)


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_round_where_a_thread_takes_a_second_item(gpu, name, p):
    log_n = SECOND_ITEM_LOG
    ops, n = FrOps(p), 1 << log_n
    a, b = geometric(p, n, 3, 5), geometric(p, n, 7, p - 1)
    a[n - 1], b[1] = 0, 0
    s, s_inv = [None] * n, [None] * n
    d_a, d_b = upload(a), upload(b)
    d_s, d_si = poisoned(gpu, n), poisoned(gpu, n)
    for k, u in ((0, None), (1, 0x1234567890ABCDEF1234567890ABCDEF % p)):
        want = M.round_step(log_n, k, a, b, s, s_inv, u, None if u is None else pow(u, -1, p), p)
        d_l, d_r = poisoned(gpu, 2 * n), poisoned(gpu, 2 * n)
        st, cross = call_round(gpu, ops, log_n, k, d_a, d_b, d_s, d_si, u, d_l, d_r, p)
        N.check(st)
        assert cross == want[2]
        assert (d_l.download() == raw(want[0])).all() and (d_r.download() == raw(want[1])).all()
        assert (d_a.download() == raw(a)).all() and (d_b.download() == raw(b)).all()
        assert (d_s.download() == raw(s)).all() and (d_si.download() == raw(s_inv)).all()


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_fold_and_cross_where_a_thread_takes_a_second_item(gpu, name, p):
    log_n = FOLD_SECOND_ITEM_LOG
    ops, n = FrOps(p), 1 << log_n
    h = n // 2
    ga, gb = 3, 7
    a, b = geometric(p, n, ga, 5), geometric(p, n, gb, 11)
    d_a, d_b = upload(a), upload(b)
    d_s, d_si = DevVec(n, zero=False), DevVec(n, zero=False)
    d_l, d_r = DevVec(2 * n, zero=False), DevVec(2 * n, zero=False)
    # k = 0: sum_{j<h} 5 ga^j * 11 gb^(j+h) is a geometric series in ga gb
    st, cross = call_round(gpu, ops, log_n, 0, d_a, d_b, d_s, d_si, None, d_l, d_r, p)
    N.check(st)
    q = ga * gb % p
    series = (pow(q, h, p) - 1) * pow(q - 1, -1, p) % p
    assert cross == (55 * pow(gb, h, p) * series % p, 55 * pow(ga, h, p) * series % p)
    # k = 1: the folded halves, element by element, and their cross products
    u = 0xFEDCBA9876543210FEDCBA9876543210 % p
    ui = pow(u, -1, p)
    st, cross = call_round(gpu, ops, log_n, 1, d_a, d_b, d_s, d_si, u, d_l, d_r, p)
    N.check(st)
    a[:h] = [(u * x + ui * y) % p for x, y in zip(a[:h], a[h:])]
    b[:h] = [(ui * x + u * y) % p for x, y in zip(b[:h], b[h:])]
    assert (d_a.download() == raw(a)).all() and (d_b.download() == raw(b)).all()
    q4 = h // 2
    assert cross == (sum(x * y for x, y in zip(a[:q4], b[q4:h])) % p, sum(x * y for x, y in zip(a[q4:h], b[:q4])) % p)


@pytest.mark.parametrize("log_n", [3, 10])
@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_cross_products_with_every_term_at_the_top_of_the_range(gpu, name, p, log_n):
    """a = b = r - 1 everywhere and u = u^-1 = r - 1, through k = 0, 1, 2.  The vectors of this entry point are powers of two long,
    so no size is "two workgroups and one element"; two sizes stand in for it.  At log_n = 10 the first cross products run two
    full workgroups and the combine reads two of the 256 partial pairs it can take; from then on, and at log_n = 3 from the
    start, a workgroup sums with most of its lanes idle.  Every product is +-1 times a power of two, so the cross products are
    also counts: (n 2^k) / 2 in round k."""
    ops, n = FrOps(p), 1 << log_n
    a, b = [p - 1] * n, [p - 1] * n
    s, s_inv = [None] * n, [None] * n
    d_a, d_b = upload(a), upload(b)
    d_s, d_si = poisoned(gpu, n), poisoned(gpu, n)
    for k in range(3):
        u = None if k == 0 else p - 1
        want = M.round_step(log_n, k, a, b, s, s_inv, u, u, p)
        d_l, d_r = poisoned(gpu, 2 * n), poisoned(gpu, 2 * n)
        st, cross = call_round(gpu, ops, log_n, k, d_a, d_b, d_s, d_si, u, d_l, d_r, p)
        N.check(st)
        assert cross == want[2], f"round {k}"
        assert cross == (((n << k) >> 1) % p,) * 2, f"round {k}: the count"
        assert ints(d_l) == want[0] and ints(d_r) == want[1], f"the scalars of round {k}"
        assert ints(d_a) == a and ints(d_b) == b and ints(d_s) == s and ints(d_si) == s_inv, f"the vectors after round {k}"


@pytest.mark.parametrize("log_n", (0,) + SIZES + (SECOND_ITEM_LOG,))
@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_verify_scalars(gpu, name, p, log_n):
    ops, n = FrOps(p), 1 << log_n
    us = challenges(p, log_n, seed=50 + log_n)
    a, b = (p - 1, p + 3) if log_n % 2 else (0x1F2E3D4C5B6A79880102030405060708090A0B0C0D0E0F % p, (1 << 256) - 1)
    out = poisoned(gpu, 2 * n)
    u_l = raw(us) if us else None
    ui_l = raw([pow(u, -1, p) for u in us]) if us else None
    N.check(gpu.zk_ipa_verify_scalars_dev(ops.cid, log_n, N.u64p(u_l) if us else None, N.u64p(ui_l) if us else None, N.u64p(raw([a])),
                                          N.u64p(raw([b])), out.ptr(), None))
    want = M.verify_scalars(log_n, [u % p for u in us], a, b, p)
    assert (out.download() == raw(want)).all()
    if log_n <= 9:
        sv = M.s_vector([u % p for u in us], log_n, p)
        assert want == [a * x % p for x in sv] + [b * pow(x, -1, p) % p for x in sv]


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_bad_arguments_leave_everything_untouched(gpu, name, p):
    log_n = 3
    ops, n = FrOps(p), 8
    a, b = table(p, log_n, 0), table(p, log_n, 1)
    big = DevVec(8 * n, zero=False)                 # a | b | s | s_inv | scal_L (2n) | scal_R (2n), every part poisoned or known
    N.check(gpu.zk_dev_memset(big.ptr(), 0x5A, 32 * 8 * n))
    big.upload(raw(a), 0)
    big.upload(raw(b), n)
    before = big.download()
    pa, pb, ps, psi, pl, pr = (big.ptr(x * n) for x in (0, 1, 2, 3, 4, 6))
    u = raw([5])
    ui = raw([pow(5, -1, p)])
    cross = np.full((2, 4), 0x77, dtype=np.uint64)
    U, UI, C = N.u64p(u), N.u64p(ui), N.u64p(cross)
    cases = {
        "null a": (log_n, 1, None, pb, ps, psi, U, UI, pl, pr, C),
        "null b": (log_n, 1, pa, None, ps, psi, U, UI, pl, pr, C),
        "null s": (log_n, 1, pa, pb, None, psi, U, UI, pl, pr, C),
        "null s_inv": (log_n, 1, pa, pb, ps, None, U, UI, pl, pr, C),
        "null scal_L": (log_n, 1, pa, pb, ps, psi, U, UI, None, pr, C),
        "null scal_R": (log_n, 0, pa, pb, ps, psi, None, None, pl, None, C),
        "null cross": (log_n, 2, pa, pb, ps, psi, U, UI, pl, pr, None),
        "k < 0": (log_n, -1, pa, pb, ps, psi, None, None, pl, pr, C),
        "k > log_n": (log_n, log_n + 1, pa, pb, ps, psi, U, UI, pl, pr, C),
        "log_n < 0": (-1, 0, pa, pb, ps, psi, None, None, pl, pr, C),
        "log_n > 22": (N.IPA_MAX_LOG + 1, 1, pa, pb, ps, psi, U, UI, pl, pr, C),
        "u at k = 0": (log_n, 0, pa, pb, ps, psi, U, UI, pl, pr, C),
        "u_inv alone at k = 0": (log_n, 0, pa, pb, ps, psi, None, UI, pl, pr, C),
        "no u at k = 1": (log_n, 1, pa, pb, ps, psi, None, UI, pl, pr, C),
        "no u_inv at k = log_n": (log_n, log_n, pa, pb, ps, psi, U, None, None, None, None),
        "b inside a": (log_n, 1, pa, pa + 32 * (n - 1), ps, psi, U, UI, pl, pr, C),
        "s is s_inv": (log_n, 1, pa, pb, ps, ps, U, UI, pl, pr, C),
        "scal_R inside scal_L": (log_n, 1, pa, pb, ps, psi, U, UI, pl, pl + 32 * (2 * n - 1), C),
        "scal_L over s_inv": (log_n, 0, pa, pb, ps, psi, None, None, psi + 32 * (n - 1), pr, C),
    }
    for what, (ln, k, *rest) in cases.items():
        assert gpu.zk_ipa_round_dev(ops.cid, ln, k, *rest, None) == N.ZK_ERR_ARG, what
        assert (big.download() == before).all() and (cross == 0x77).all(), what
    assert gpu.zk_ipa_round_dev(7, log_n, 0, pa, pb, ps, psi, None, None, pl, pr, C, None) == N.ZK_ERR_ARG, "unknown curve"
    out = big.ptr(4 * n)
    one = N.u64p(raw([1]))
    for what, args in {
        "null a": (log_n, U, UI, None, one, out),
        "null b": (log_n, U, UI, one, None, out),
        "null out": (log_n, U, UI, one, one, None),
        "no u": (log_n, None, UI, one, one, out),
        "no u_inv": (log_n, U, None, one, one, out),
        "log_n < 0": (-1, U, UI, one, one, out),
        "log_n > 22": (N.IPA_MAX_LOG + 1, U, UI, one, one, out),
    }.items():
        assert gpu.zk_ipa_verify_scalars_dev(ops.cid, *args, None) == N.ZK_ERR_ARG, what
    assert (big.download() == before).all()
    # the same buffers do work: nothing above failed for a reason other than the one named
    assert gpu.zk_ipa_round_dev(ops.cid, log_n, 0, pa, pb, ps, psi, None, None, pl, pr, C, None) == N.ZK_OK
    # overlap is judged on what a call touches: with k == log_n the scalar buffers are not looked at
    assert gpu.zk_ipa_round_dev(ops.cid, log_n, log_n, pa, pb, ps, psi, U, UI, None, None, None, None) == N.ZK_OK
