"""GPU: zk_mlpcs_quotients_dev (csrc/mlpcs.hip) against the integer model (tests/mlpcs_model.py), by ==: every quotient entry and
the evaluation.

With T = ZK_MLE_TILE_LOG the sizes are the smallest at which the chain changes path: no variable, one, two; T-1, T and T+1 (a
partial tile, one whole tile in one pass, the first chain of two passes); 2T (two whole passes) and 2T+1 (2^17 elements, the
first chain of three passes).  The grid is not capped (one workgroup per tile at every size up to the cap of 24 variables, 2^16
workgroups), so there is no second-tile path to place a size on."""

import random

import numpy as np
import pytest

import mlpcs_model as M
from stream_state_child import behind_spin, settle, staged
from zksnake_amd import _native as N
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from zksnake_amd.frvec import DevVec, FrOps

pytestmark = pytest.mark.gpu

T = N.MLE_TILE_LOG
FIELDS = (("BN254", BN254_SCALAR_FIELD), ("BLS12_381", BLS12_381_SCALAR_FIELD))
SIZES = sorted({0, 1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1})
GUARD = 0x5A5A5A5A5A5A5A5A
_CASES = {}


def table(p, log_n, seed=0):
    rnd = random.Random(4000 * log_n + seed + (p & 0xFF))
    t = [rnd.randrange(p) for _ in range(1 << log_n)]
    t[-1] = p - 1
    if log_n:
        t[0] = 0
    if log_n > 2:
        t[3], t[len(t) // 2], t[len(t) // 2 + 1] = p - 1, 0, p - 1
    return t


def point(p, k, seed=0):
    """k coordinates as the caller hands them in (not reduced): 0, 1, r-1 and values >= r first AND last, random ones between"""
    rnd = random.Random(91 + seed)
    special = [0, 1, p - 1, p + 5, (1 << 256) - 1, p]
    out = [rnd.randrange(p) for _ in range(k)]
    for i, s in enumerate(special[:k]):
        out[i] = s
    for i, s in enumerate(special[:max(k - len(special), 0)]):
        out[k - 1 - i] = s
    return out


def case(p, log_n):
    """(table, point, expected flat quotients, expected evaluation), computed once and shared"""
    key = (p, log_n)
    if key not in _CASES:
        t, z = table(p, log_n), point(p, log_n, seed=log_n)
        _CASES[key] = (t, z) + M.flat_quotients(t, [x % p for x in z], p)
    return _CASES[key]


def raw_limbs(values):
    return N.ints_to_limbs(values, 4) if values else np.zeros((1, 4), dtype=np.uint64)


def run(gpu, ops, log_n, d_f, z, work=None, stream=None):
    """one call; returns (the 2^log_n - 1 quotient entries, the evaluation); asserts the guard element behind d_q"""
    n = 1 << log_n
    d_q = DevVec(n, zero=False)                    # n - 1 entries and one guard element
    d_q.upload(np.full((n, 4), GUARD, dtype=np.uint64))
    out = np.zeros(4, dtype=np.uint64)
    N.check(gpu.zk_mlpcs_quotients_dev(ops.cid, log_n, d_f, N.u64p(raw_limbs(z)) if log_n else None, d_q.ptr(), N.u64p(out),
                                       work.ptr() if work else None, stream))
    got = d_q.download(n)
    assert (got[n - 1] == GUARD).all(), "the element behind the last quotient was written"
    return N.limbs_to_ints(got[:n - 1]) if n > 1 else [], N.limbs_to_ints(out.reshape(1, 4))[0]


@pytest.mark.parametrize("log_n", SIZES)
@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_quotients_and_evaluation(gpu, name, p, log_n):
    ops = FrOps(p)
    t, z, want_q, want_v = case(p, log_n)
    d_f = ops.d_from(N.ints_to_limbs(t, 4))
    for work in (DevVec(1 << (max(log_n - T, 0) + 1), zero=False), None):
        got_q, got_v = run(gpu, ops, log_n, d_f.ptr(), z, work)
        assert got_v == want_v
        assert got_q == want_q
    assert N.limbs_to_ints(d_f.download()) == t, "d_f was modified"


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_all_r_minus_one_and_the_ends_of_the_range(gpu, name, p):
    ops = FrOps(p)
    log_n = T + 1
    n = 1 << log_n
    d_f = ops.d_from(N.ints_to_limbs([p - 1] * n, 4))
    z = ([0, 1, p - 1] * log_n)[:log_n]
    got_q, got_v = run(gpu, ops, log_n, d_f.ptr(), z)
    assert got_q == [0] * (n - 1) and got_v == p - 1
    # alternating 0 / r-1: the first level is all r-1 or all 1, every later one zero
    for pair in ((0, p - 1), (p - 1, 0)):
        t = list(pair) * (n // 2)
        d_t = ops.d_from(N.ints_to_limbs(t, 4))
        got_q, got_v = run(gpu, ops, log_n, d_t.ptr(), z[::-1])
        assert (got_q, got_v) == M.flat_quotients(t, z[::-1], p)
        assert got_q[:n // 2] == [(pair[1] - pair[0]) % p] * (n // 2) and not any(got_q[n // 2:])


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_on_a_busy_stream(gpu, name, p):
    """the table arrives from page-locked memory behind a spin on a fresh stream; the call on that stream must see it (the two
    passes, the quotient stores and the copy of the evaluation all ordered there) and return the bytes of a default-stream call"""
    ops = FrOps(p)
    log_n = T + 1
    t, z, want_q, want_v = case(p, log_n)
    stale = table(p, log_n, seed=5)
    f = staged(stale, t)
    got = behind_spin(gpu, [f], lambda st: run(gpu, ops, log_n, f.ptr, z, None, st))
    settle(got, (want_q, want_v), M.flat_quotients(stale, [x % p for x in z], p))
    assert got == run(gpu, ops, log_n, f.ptr, z)


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_bad_arguments_are_refused_and_write_nothing(gpu, name, p):
    ops = FrOps(p)
    log_n = 4
    n = 1 << log_n
    t = table(p, log_n + 2)
    buf = ops.d_from(N.ints_to_limbs(t, 4))        # 4n elements: f at 0, outputs placed inside, across or beside it
    z = N.u64p(raw_limbs(point(p, log_n)))
    out = np.zeros(4, dtype=np.uint64)
    call = lambda log, f, q, w: gpu.zk_mlpcs_quotients_dev(ops.cid, log, f, z, q, N.u64p(out), w, None)   # noqa: E731
    for off in (0, 1, n - 1):
        assert call(log_n, buf.ptr(0), buf.ptr(off), buf.ptr(3 * n)) == N.ZK_ERR_ARG            # d_q over d_f
        assert call(log_n, buf.ptr(0), buf.ptr(n), buf.ptr(off)) == N.ZK_ERR_ARG                # d_work over d_f
    assert call(log_n, buf.ptr(n), buf.ptr(2), buf.ptr(3 * n)) == N.ZK_ERR_ARG                  # the end of d_q over the start of d_f
    assert call(log_n, buf.ptr(0), buf.ptr(n), buf.ptr(n)) == N.ZK_ERR_ARG                      # d_work over d_q
    assert call(log_n, buf.ptr(0), buf.ptr(n), buf.ptr(2 * n - 2)) == N.ZK_ERR_ARG
    assert call(-1, buf.ptr(0), buf.ptr(n), None) == N.ZK_ERR_ARG
    assert call(N.MLPCS_MAX_LOG + 1, buf.ptr(0), buf.ptr(n), None) == N.ZK_ERR_ARG
    assert call(log_n, None, buf.ptr(n), None) == N.ZK_ERR_ARG and call(log_n, buf.ptr(0), None, None) == N.ZK_ERR_ARG
    assert gpu.zk_mlpcs_quotients_dev(ops.cid, log_n, buf.ptr(0), None, buf.ptr(n), N.u64p(out), None, None) == N.ZK_ERR_ARG
    assert gpu.zk_mlpcs_quotients_dev(ops.cid, log_n, buf.ptr(0), z, buf.ptr(n), None, None, None) == N.ZK_ERR_ARG
    assert gpu.zk_mlpcs_quotients_dev(2, log_n, buf.ptr(0), z, buf.ptr(n), N.u64p(out), None, None) == N.ZK_ERR_ARG
    assert N.limbs_to_ints(buf.download()) == t and not out.any()
    # d_q directly behind d_f and d_work directly behind d_q are fine
    N.check(call(log_n, buf.ptr(0), buf.ptr(n), buf.ptr(2 * n - 1)))
    want_q, want_v = M.flat_quotients(t[:n], [x % p for x in point(p, log_n)], p)
    assert N.limbs_to_ints(buf.download(n - 1, n)) == want_q and N.limbs_to_ints(out.reshape(1, 4))[0] == want_v
    assert N.limbs_to_ints(buf.download(n)) == t[:n] and N.limbs_to_ints(buf.download(2 * n, 2 * n)) == t[2 * n:]
