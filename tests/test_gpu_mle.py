"""GPU: the multilinear kernels (csrc/mle.hip) and MultilinearPolynomial (mle.py) against the integer model, by ==.

With T = ZK_MLE_TILE_LOG the sizes are the smallest at which each kernel changes path: log_n below, at and above one tile,
2T+1 (three fix passes; coefficient passes of 8, 6 and 3 bits), 2^16 (several workgroups, second-level reduce) and, for the
sum alone, 2^19 (the smallest table at which a workgroup of the capped grid takes a second stride)."""

import random

import numpy as np
import pytest

import mle_model as M
from zksnake_amd import _native as N
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from zksnake_amd.frvec import DevVec, FrOps
from zksnake_amd.mle import MLE_OBJECT
from zksnake_amd.polynomial import MultilinearPolynomial

pytestmark = pytest.mark.gpu

T = N.MLE_TILE_LOG
FIELDS = (("BN254", BN254_SCALAR_FIELD), ("BLS12_381", BLS12_381_SCALAR_FIELD))
SIZES = sorted({0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 16})
_TABLES = {}


def table(p, log_n, seed=0):
    """random table with the entries 0 and r-1 (shared by the tests, never modified)"""
    key = (p, log_n, seed)
    if key not in _TABLES:
        rnd = random.Random(1000 * log_n + seed + (p & 0xFF))
        t = [rnd.randrange(p) for _ in range(1 << log_n)]
        t[-1] = p - 1
        if log_n:
            t[0] = 0
        if log_n > 2:
            t[3], t[len(t) // 2] = p - 1, 0
        _TABLES[key] = t
    return _TABLES[key]


def challenges(p, k, seed=0):
    """k scalars as the caller hands them in (not reduced): 0, 1, r-1, values >= r, then random ones"""
    rnd = random.Random(77 + seed)
    special = [0, 1, p - 1, p + 5, (1 << 256) - 1, p]
    return [special[i] if i < len(special) else rnd.randrange(p) for i in range(k)]


def raw_limbs(values):
    return N.ints_to_limbs(values, 4) if values else np.zeros((1, 4), dtype=np.uint64)


def upload(ops, values):
    return ops.d_from(N.ints_to_limbs(values, 4))


def ints(vec, count):
    return N.limbs_to_ints(vec.download(count))


@pytest.mark.parametrize("log_n", SIZES)
@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_fix_eval_sum_coeffs(gpu, name, p, log_n):
    ops = FrOps(p)
    t = table(p, log_n)
    n = 1 << log_n
    d_in = upload(ops, t)
    for k in sorted({0, 1, T, T + 1, log_n}):
        if k > log_n:
            continue
        rs = challenges(p, k, seed=k)
        if k == log_n and k > 1:
            rs = rs[::-1]   # the special values also on the last variables
        d_out = DevVec(n >> k, zero=False)
        N.check(gpu.zk_mle_fix_dev(ops.cid, log_n, d_in.ptr(), k, N.u64p(raw_limbs(rs)), d_out.ptr(), None))
        assert ints(d_out, n >> k) == M.fix(t, [r % p for r in rs], p), f"fix k={k}"
    point = challenges(p, log_n, seed=9)
    want = M.evaluate(t, [r % p for r in point], p)
    for work in (DevVec(1 << (max(log_n - T, 0) + 1), zero=False), None):
        out = np.zeros(4, dtype=np.uint64)
        N.check(gpu.zk_mle_eval_dev(ops.cid, log_n, d_in.ptr(), N.u64p(raw_limbs(point)), N.u64p(out), work.ptr() if work else None, None))
        assert N.limbs_to_ints(out.reshape(1, 4))[0] == want
    out = np.zeros(4, dtype=np.uint64)
    N.check(gpu.zk_mle_sum_dev(ops.cid, n, d_in.ptr(), N.u64p(out), None))
    assert N.limbs_to_ints(out.reshape(1, 4))[0] == M.total(t, p)
    want_c = M.coefficients(t, p)
    d_c = DevVec(n, zero=False)
    N.check(gpu.zk_mle_coeffs_dev(ops.cid, log_n, d_in.ptr(), d_c.ptr(), None))
    assert ints(d_c, n) == want_c
    assert ints(d_in, n) == t, "an input table was modified"
    N.check(gpu.zk_mle_coeffs_dev(ops.cid, log_n, d_in.ptr(), d_in.ptr(), None))   # in place
    assert ints(d_in, n) == want_c


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_sum_where_the_capped_grid_strides(gpu, name, p):
    ops = FrOps(p)
    t = table(p, 19)
    out = np.zeros(4, dtype=np.uint64)
    d_x = upload(ops, t)
    N.check(gpu.zk_mle_sum_dev(ops.cid, len(t), d_x.ptr(), N.u64p(out), None))
    assert N.limbs_to_ints(out.reshape(1, 4))[0] == M.total(t, p)


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_all_zero_table(gpu, name, p):
    ops = FrOps(p)
    log_n = T + 1
    n = 1 << log_n
    d_in, d_out = DevVec(n), DevVec(n, zero=False)
    rs = challenges(p, log_n)
    for k in (1, T, log_n):
        N.check(gpu.zk_mle_fix_dev(ops.cid, log_n, d_in.ptr(), k, N.u64p(raw_limbs(rs[:k])), d_out.ptr(), None))
        assert not d_out.download(n >> k).any()
    out = np.ones(4, dtype=np.uint64)
    N.check(gpu.zk_mle_eval_dev(ops.cid, log_n, d_in.ptr(), N.u64p(raw_limbs(rs)), N.u64p(out), None, None))
    assert not out.any()
    out = np.ones(4, dtype=np.uint64)
    N.check(gpu.zk_mle_sum_dev(ops.cid, n, d_in.ptr(), N.u64p(out), None))
    assert not out.any()
    N.check(gpu.zk_mle_coeffs_dev(ops.cid, log_n, d_in.ptr(), d_out.ptr(), None))
    assert not d_out.download(n).any()


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_overlapping_and_bad_arguments_are_refused_and_write_nothing(gpu, name, p):
    ops = FrOps(p)
    log_n = 4
    n = 1 << log_n
    t = table(p, log_n + 1)
    buf = upload(ops, t)   # 2n elements: input at 0, outputs placed inside or across it
    rs = raw_limbs(challenges(p, log_n))
    perm = np.arange(log_n, dtype=np.uint8)
    for off in (0, 1, n // 2, n - 1):
        assert gpu.zk_mle_fix_dev(ops.cid, log_n, buf.ptr(0), 1, N.u64p(rs), buf.ptr(off), None) == N.ZK_ERR_ARG
        assert gpu.zk_mle_permute_dev(ops.cid, log_n, buf.ptr(0), N.u8p(perm), buf.ptr(off), None) == N.ZK_ERR_ARG
        if off:
            assert gpu.zk_mle_coeffs_dev(ops.cid, log_n, buf.ptr(0), buf.ptr(off), None) == N.ZK_ERR_ARG
    assert gpu.zk_mle_fix_dev(ops.cid, log_n, buf.ptr(n), 0, None, buf.ptr(n - 1), None) == N.ZK_ERR_ARG   # the copy too
    out = np.zeros(4, dtype=np.uint64)
    assert gpu.zk_mle_eval_dev(ops.cid, log_n, buf.ptr(0), N.u64p(rs), N.u64p(out), buf.ptr(n - 1), None) == N.ZK_ERR_ARG
    assert gpu.zk_mle_fix_dev(ops.cid, log_n, buf.ptr(0), log_n + 1, N.u64p(rs), buf.ptr(n), None) == N.ZK_ERR_ARG
    assert gpu.zk_mle_fix_dev(ops.cid, -1, buf.ptr(0), 0, N.u64p(rs), buf.ptr(n), None) == N.ZK_ERR_ARG
    for bad in ([0, 1, 1, 3], [0, 1, 2, 4]):
        assert gpu.zk_mle_permute_dev(ops.cid, log_n, buf.ptr(0), N.u8p(np.array(bad, dtype=np.uint8)), buf.ptr(n), None) == N.ZK_ERR_ARG
    assert ints(buf, 2 * n) == t


@pytest.mark.parametrize("log_n", [5, T + 2])
@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_permute_and_swap(gpu, name, p, log_n):
    ops = FrOps(p)
    t = table(p, log_n)
    n = 1 << log_n
    d_in, d_out = upload(ops, t), DevVec(n, zero=False)
    rnd = random.Random(log_n)
    shuffled = list(range(log_n))
    rnd.shuffle(shuffled)
    perms = [list(range(log_n)), list(range(log_n))[::-1], shuffled,
             M.swap_perm(log_n, 0, 2, 2),             # adjacent blocks
             M.swap_perm(log_n, 1, 2, 1),
             M.swap_perm(log_n, 0, log_n - 2, 2)]     # distant blocks
    for perm in perms:
        N.check(gpu.zk_mle_permute_dev(ops.cid, log_n, d_in.ptr(), N.u8p(np.array(perm, dtype=np.uint8)), d_out.ptr(), None))
        assert ints(d_out, n) == M.permute(t, perm), perm
    assert ints(d_in, n) == t


# ---- the Python class ----

@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_multilinear_polynomial_against_the_model(gpu, name, p):
    rnd = random.Random(5)
    nv = T + 1
    t = table(p, nv)
    dense = MLE_OBJECT[p].from_evaluations(t, p)
    sparse = MultilinearPolynomial(nv, [(i, v) for i, v in enumerate(t) if v], p)
    assert sparse == dense and sparse.num_vars == nv and type(sparse) is MLE_OBJECT[p]
    assert dense.to_evaluations() == t
    limbs = N.ints_to_limbs([v + p if v < 5 else v for v in t], 4)      # a limb table with entries >= p is reduced
    assert MLE_OBJECT[p].from_evaluations(limbs, p) == dense
    pt = challenges(p, nv)
    assert dense.evaluate(pt) == M.evaluate(t, [x % p for x in pt], p)
    for k in (0, 1, T, nv):
        part = dense.partial_evaluate(pt[:k])
        assert part.num_vars == nv - k and part.to_evaluations() == M.fix(t, [x % p for x in pt[:k]], p)
    assert len(dense.partial_evaluate(pt).to_evaluations()) == 1
    assert dense.to_coefficients() == M.coefficients(t, p)
    assert dense.sum() == M.total(t, p)
    perm = list(range(nv))
    rnd.shuffle(perm)
    assert dense.permute_evaluations(perm).to_evaluations() == M.permute(t, perm)
    assert dense.swap(0, 3, 2).to_evaluations() == M.permute(t, M.swap_perm(nv, 0, 3, 2))
    assert dense.swap(0, 3, 2).swap(3, 0, 2) == dense
    assert dense.to_evaluations() == t, "a method modified its polynomial"
    other = MLE_OBJECT[p].from_evaluations(table(p, nv, seed=1), p)
    assert (dense + other).to_evaluations() == [(a + b) % p for a, b in zip(t, table(p, nv, seed=1))]
    assert (dense - other).to_evaluations() == [(a - b) % p for a, b in zip(t, table(p, nv, seed=1))]
    assert dense + other - other == dense and dense != other


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_multilinear_polynomial_constructor_and_errors(gpu, name, p):
    cls = MLE_OBJECT[p]
    g = MultilinearPolynomial(4, [(5, 1), (6, 1), (7, 1)], p)
    assert g.to_evaluations() == [0] * 5 + [1, 1, 1] + [0] * 8
    assert str(g) == repr(g) == "SparseMLPolynomial(num_vars=4, evaluations=[0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0])"
    assert MultilinearPolynomial(2, [(1, p + 3), (1, 2 * p + 7), (3, p - 1)], p).to_evaluations() == [0, 7, 0, p - 1]   # reduced; last wins
    zero = MultilinearPolynomial(0, [(0, 9)], p)          # the reference's rule: no variables -> zero()
    assert zero == cls.zero() and zero.num_vars == 0 and zero.to_evaluations() == [0] and zero.evaluate([]) == 0
    assert g + zero == g and zero + g == g and g - zero == g
    assert (zero - g).to_evaluations() == [(-v) % p for v in g.to_evaluations()]
    with pytest.raises(ValueError):
        MultilinearPolynomial(2, [(4, 1)], p)
    with pytest.raises(ValueError, match="Evaluation requires points to be in the same size as the number of variables"):
        g.evaluate([1, 2, 3])
    with pytest.raises(ValueError):
        g.partial_evaluate([1] * 5)
    with pytest.raises(ValueError):
        g.permute_evaluations([0, 1, 1, 3])
    with pytest.raises(ValueError):
        g.swap(0, 1, 2)
    with pytest.raises(ValueError):
        g + MultilinearPolynomial(3, [(1, 1)], p)
    with pytest.raises(ValueError):
        cls.from_evaluations([1, 2, 3], p)
    assert g != MultilinearPolynomial(3, [(5, 1)], p)
