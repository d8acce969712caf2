"""GPU: zk_pcs_round_dev and zk_pcs_verify_scalars_dev (csrc/pcs.hip) against the integer contracts of tests/pcs_model.py, by ==:
every output element and both sums.

Sizes log_n = 0, 1, 2, 3, 5 and 9, each chained through every k of an opening (so k = 0, 1, log_n - 1 and log_n among them), on
both curves, with the opening point z in {0, 1, r - 1, a random value handed in unreduced}, 0 and r - 1 scattered through c, a
challenge >= r, and once behind a parked stream.  The grid is capped at 1024 workgroups of 256 threads: the pass over i < n takes a
second item per thread first at n = 2^19, the fold and the sums first at n = 2^20.  At those two sizes k = 0, 1, 2 run on a
geometric table c_i = a g^i against closed forms: the fold stays geometric, s_i is a product over the top bits of i, and the two
sums are geometric series."""

import ctypes
import itertools
import random

import numpy as np
import pytest

import pcs_model as M
from zksnake_amd import _native as N
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from zksnake_amd.frvec import DevVec, FrOps

pytestmark = pytest.mark.gpu

FIELDS = (("BN254", BN254_SCALAR_FIELD), ("BLS12_381", BLS12_381_SCALAR_FIELD))
IDS = [f[0] for f in FIELDS]
SIZES = (0, 1, 2, 3, 5, 9)
POINTS = ("zero", "one", "minus_one", "random")
_TABLES = {}


def table(p, log_n):
    """random table with 0 and r-1 scattered through it (shared by the tests, never modified)"""
    if (p, log_n) not in _TABLES:
        rnd = random.Random(100 * log_n + (p & 0xFF))
        t = [rnd.randrange(p) for _ in range(1 << log_n)]
        for i in range(0, len(t), 5):
            t[i] = 0 if i % 2 else p - 1
        t[-1] = p - 1
        _TABLES[(p, log_n)] = t
    return _TABLES[(p, log_n)]


def point(p, kind):
    """the opening point as handed in; the random one is not reduced"""
    return {"zero": 0, "one": 1, "minus_one": p - 1, "random": random.Random(p & 0xFFFF).randrange(p) + p}[kind]


def challenges(p, count, seed):
    """as handed in: 1, r-1, a value >= r, then random ones"""
    rnd = random.Random(seed)
    special = [1, p - 1, p + 5]
    return [special[i] if i < len(special) else rnd.randrange(1, p) for i in range(count)]


def geometric(p, n, g, first):
    return list(itertools.accumulate(itertools.repeat(g, n - 1), lambda x, y: x * y % p, initial=first % p))


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


def call_round(gpu, ops, log_n, k, c, s, u, z, scal_l, scal_r, p, stream=None):
    """one zk_pcs_round_dev; u, z: as handed in (u None at k = 0).  Returns the two sums."""
    evals = np.zeros((2, 4), dtype=np.uint64)
    last = k == log_n
    u_l = None if u is None else raw([u])
    ui_l = None if u is None else raw([pow(u, -1, p)])
    z_l = None if z is None else raw([z])
    N.check(gpu.zk_pcs_round_dev(ops.cid, log_n, k, c.ptr(), s.ptr(), None if u is None else N.u64p(u_l), None if u is None else N.u64p(ui_l),
                                 None if z is None else N.u64p(z_l), None if last else scal_l.ptr(), None if last else scal_r.ptr(),
                                 None if last else N.u64p(evals), stream))
    return tuple(N.limbs_to_ints(evals))


def run_chain(gpu, p, log_n, kind, stream=None):
    ops, n = FrOps(p), 1 << log_n
    c, s = list(table(p, log_n)), [None] * n
    d_c, d_s = upload(c), poisoned(gpu, n)
    us, z = challenges(p, log_n, seed=log_n), point(p, kind)
    u = None
    for k in range(log_n + 1):
        want = M.round_step(log_n, k, c, s, u, None if u is None else pow(u, -1, p), z, p)
        d_l, d_r = poisoned(gpu, n), poisoned(gpu, n)        # the zero halves must really be written
        if stream is not None:
            N.check(gpu.zk_dev_synchronize())                # the stream does not wait for the default stream's fills
            N.check(gpu.zk_debug_spin_dev(stream, 2000))     # the call queues up behind work already on its stream
        if k == log_n:
            call_round(gpu, ops, log_n, k, d_c, d_s, u, None, None, None, p, stream)
            if stream is not None:
                N.check(gpu.zk_stream_synchronize(stream))
        else:
            evals = call_round(gpu, ops, log_n, k, d_c, d_s, u, z, d_l, d_r, p, stream)
            assert evals == want[2], f"sums, round {k}"
            assert ints(d_l) == want[0], f"scal_L, round {k}"
            assert ints(d_r) == want[1], f"scal_R, round {k}"
            u = us[k]
        m = n >> k
        assert ints(d_c)[:m] == c[:m], f"c after round {k}"
        assert ints(d_s) == s, f"s after round {k}"
    assert s == M.verify_scalars(log_n, us, 1, p)


@pytest.mark.parametrize("kind", POINTS)
@pytest.mark.parametrize("log_n", SIZES)
@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_round_chained_through_an_opening(gpu, name, p, log_n, kind):
    run_chain(gpu, p, log_n, kind)


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_round_and_verify_scalars_on_a_busy_stream(gpu, name, p):
    stream = ctypes.c_void_p()
    N.check(gpu.zk_stream_create(0, ctypes.byref(stream)))
    try:
        run_chain(gpu, p, 9, "random", stream)
        ops, log_n = FrOps(p), 9
        us = challenges(p, log_n, seed=7)
        out = poisoned(gpu, 1 << log_n)
        N.check(gpu.zk_dev_synchronize())
        N.check(gpu.zk_debug_spin_dev(stream, 2000))
        N.check(gpu.zk_pcs_verify_scalars_dev(ops.cid, log_n, N.u64p(raw(us)), N.u64p(raw([p + 3])), out.ptr(), stream))
        N.check(gpu.zk_stream_synchronize(stream))
        assert ints(out) == M.verify_scalars(log_n, us, 3, p)
    finally:
        N.check(gpu.zk_stream_destroy(stream))


@pytest.mark.parametrize("log_n", SIZES + (19,))
@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_verify_scalars(gpu, name, p, log_n):
    ops, n = FrOps(p), 1 << log_n
    us = challenges(p, log_n, seed=50 + log_n)
    c = (p - 1, p + 3, (1 << 256) - 1, 0)[log_n % 4]
    out = poisoned(gpu, n)
    u_l = raw(us) if us else None
    N.check(gpu.zk_pcs_verify_scalars_dev(ops.cid, log_n, N.u64p(u_l) if us else None, N.u64p(raw([c])), out.ptr(), None))
    want = M.verify_scalars(log_n, us, c, p)
    assert (out.download() == raw(want)).all()
    if log_n <= 9:     # s_i is the product of the challenges whose bit is set in i
        for i in (0, n - 1, n // 2, 5 % n):
            prod = c % p
            for t in range(log_n):
                if (i >> (log_n - 1 - t)) & 1:
                    prod = prod * us[t] % p
            assert want[i] == prod


@pytest.mark.parametrize("log_n", [19, 20])
@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_rounds_where_a_thread_takes_a_second_item(gpu, name, p, log_n):
    """k = 0, 1, 2 on c_i = a g^i.  After k folds c_j = a_k g^j for j < m with a_k = a prod_{t<k} (1 + u_t^-1 g^(n >> (t+1))); s is
    constant on each of the 2^k blocks of m indices; with q = g z the sums are a_k g^h (q^h - 1)/(q - 1) and a_k (q^h - 1)/(q - 1)."""
    ops, n = FrOps(p), 1 << log_n
    a, g = 5, 3
    z = 0x0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF % p
    q = g * z % p
    d_c, d_s = upload(geometric(p, n, g, a)), poisoned(gpu, n)
    d_l, d_r = poisoned(gpu, n), poisoned(gpu, n)
    us = [0x1234567890ABCDEF1234567890ABCDEF % p, p - 2]
    block_s = [1]                      # s on the blocks of m indices, in index order
    for k in range(3):
        m = n >> k
        h = m // 2
        u = None
        if k:
            u = us[k - 1]
            a = a * (1 + pow(u, -1, p) * pow(g, m, p)) % p
            block_s = [x * f % p for x in block_s for f in (1, u)]
        evals = call_round(gpu, ops, log_n, k, d_c, d_s, u, z, d_l, d_r, p)
        series = (pow(q, h, p) - 1) * pow(q - 1, -1, p) % p
        assert evals == (a * pow(g, h, p) * series % p, a * series % p), f"sums, round {k}"
        assert (d_c.download(m) == raw(geometric(p, m, g, a))).all(), f"c after round {k}"
        assert (d_s.download() == np.repeat(raw(block_s), m, axis=0)).all(), f"s after round {k}"
        want_l, want_r = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
        for b, sb in enumerate(block_s):
            want_l[b * m:b * m + h] = raw(geometric(p, h, g, sb * a * pow(g, h, p)))    # c[j+h] s[i], j < h
            want_r[b * m + h:(b + 1) * m] = raw(geometric(p, h, g, sb * a))             # c[j-h] s[i], j >= h
        assert (d_l.download() == want_l).all(), f"scal_L, round {k}"
        assert (d_r.download() == want_r).all(), f"scal_R, round {k}"


@pytest.mark.parametrize("name,p", FIELDS, ids=IDS)
def test_bad_arguments_leave_everything_untouched(gpu, name, p):
    log_n, n = 3, 8
    ops = FrOps(p)
    big = DevVec(4 * n, zero=False)                 # c | s | scal_L | scal_R
    N.check(gpu.zk_dev_memset(big.ptr(), 0x5A, 32 * 4 * n))
    big.upload(raw(table(p, log_n)), 0)
    before = big.download()
    pc, ps, pl, pr = (big.ptr(x * n) for x in range(4))
    u, ui, z = raw([5]), raw([pow(5, -1, p)]), raw([9])
    evals = np.full((2, 4), 0x77, dtype=np.uint64)
    U, UI, Z, E = N.u64p(u), N.u64p(ui), N.u64p(z), N.u64p(evals)
    cases = {
        "null c": (log_n, 1, None, ps, U, UI, Z, pl, pr, E),
        "null s": (log_n, 1, pc, None, U, UI, Z, pl, pr, E),
        "null z": (log_n, 1, pc, ps, U, UI, None, pl, pr, E),
        "null scal_L": (log_n, 1, pc, ps, U, UI, Z, None, pr, E),
        "null scal_R": (log_n, 0, pc, ps, None, None, Z, pl, None, E),
        "null evals": (log_n, 2, pc, ps, U, UI, Z, pl, pr, None),
        "k < 0": (log_n, -1, pc, ps, None, None, Z, pl, pr, E),
        "k > log_n": (log_n, log_n + 1, pc, ps, U, UI, Z, pl, pr, E),
        "log_n < 0": (-1, 0, pc, ps, None, None, Z, pl, pr, E),
        "log_n > 21": (N.PCS_MAX_LOG + 1, 1, pc, ps, U, UI, Z, pl, pr, E),
        "u at k = 0": (log_n, 0, pc, ps, U, UI, Z, pl, pr, E),
        "no u at k = 1": (log_n, 1, pc, ps, None, UI, Z, pl, pr, E),
        "no u_inv at k = log_n": (log_n, log_n, pc, ps, U, None, None, None, None, None),
        "s inside c": (log_n, 1, pc, pc + 32 * (n - 1), U, UI, Z, pl, pr, E),
        "scal_L is s": (log_n, 1, pc, ps, U, UI, Z, ps, pr, E),
        "scal_R inside scal_L": (log_n, 1, pc, ps, U, UI, Z, pl, pl + 32 * (n - 1), E),
    }
    for what, args in cases.items():
        assert gpu.zk_pcs_round_dev(ops.cid, *args, None) == N.ZK_ERR_ARG, what
        assert (big.download() == before).all() and (evals == 0x77).all(), what
    assert gpu.zk_pcs_round_dev(7, log_n, 0, pc, ps, None, None, Z, pl, pr, E, None) == N.ZK_ERR_ARG, "unknown curve"
    one = N.u64p(raw([1]))
    for what, args in {"null c": (log_n, U, None, pl), "null out": (log_n, U, one, None), "no u": (log_n, None, one, pl),
                       "log_n < 0": (-1, U, one, pl), "log_n > 21": (N.PCS_MAX_LOG + 1, U, one, pl)}.items():
        assert gpu.zk_pcs_verify_scalars_dev(ops.cid, *args, None) == N.ZK_ERR_ARG, what
    assert (big.download() == before).all()
    # the same buffers do work: nothing above failed for a reason other than the one named
    assert gpu.zk_pcs_round_dev(ops.cid, log_n, 0, pc, ps, None, None, Z, pl, pr, E, None) == N.ZK_OK
    assert gpu.zk_pcs_round_dev(ops.cid, log_n, log_n, pc, ps, U, UI, None, None, None, None, None) == N.ZK_OK
