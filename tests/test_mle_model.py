"""CPU: pins the integer model the GPU tests compare with (tests/mle_model.py), the new C entry points' behaviour without a
GPU, and the host-only sumcheck verifier."""

import ctypes
import random

import numpy as np
import pytest

import mle_model as M
from zksnake_amd import _native as N
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD

FIELDS = (("BN254", BN254_SCALAR_FIELD), ("BLS12_381", BLS12_381_SCALAR_FIELD))
NEW_SYMBOLS = ("zk_mle_fix_dev", "zk_mle_sum_dev", "zk_mle_eval_dev", "zk_mle_coeffs_dev", "zk_mle_permute_dev", "zk_sumcheck_round_dev")
GKR_TERMS = [(1, (0, 1)), (1, (0, 2)), (1, (3, 1, 2))]   # A B + A C + M B C


def _table(rnd, n, p):
    t = [rnd.randrange(p) for _ in range(1 << n)]
    t[0], t[-1] = 0, p - 1
    return t


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_evaluate_at_boolean_points_returns_the_table(name, p):
    rnd = random.Random(1)
    for n in (0, 1, 3, 5):
        t = _table(rnd, n, p)
        for i in range(1 << n):
            assert M.evaluate(t, [(i >> b) & 1 for b in range(n)], p) == t[i]


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_coefficients_expand_to_the_polynomial(name, p):
    rnd = random.Random(2)
    for n in (0, 1, 2, 4, 6):
        t = _table(rnd, n, p)
        c = M.coefficients(t, p)
        assert len(c) == len(t)
        for _ in range(4):
            pt = [rnd.randrange(p) for _ in range(n)]
            assert M.expand(c, pt, p) == M.evaluate(t, pt, p)


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_fix_then_evaluate_is_evaluate(name, p):
    rnd = random.Random(3)
    n = 6
    t = _table(rnd, n, p)
    pt = [0, 1, p - 1] + [rnd.randrange(p) for _ in range(n - 3)]
    for k in range(n + 1):
        rest = M.fix(t, pt[:k], p)
        assert len(rest) == 1 << (n - k)
        assert M.evaluate(rest, pt[k:], p) == M.evaluate(t, pt, p)
    assert M.total(t, p) == sum(t) % p


def test_permute_and_swap():
    t = list(range(32))
    assert M.permute(t, [0, 1, 2, 3, 4]) == t
    rev = M.permute(t, [4, 3, 2, 1, 0])
    assert rev[0b00001] == t[0b10000] and rev[0b00110] == t[0b01100]
    for a, b, k in ((0, 1, 1), (0, 2, 2), (0, 3, 2), (1, 4, 1)):
        perm = M.swap_perm(5, a, b, k)
        once = M.permute(t, perm)
        assert once != t
        assert M.permute(once, perm) == t   # an involution
    # swapping variables 0 and 1 of f(x0, x1) = table: f'(x0, x1) = f(x1, x0)
    assert M.permute([10, 11, 12, 13], M.swap_perm(2, 0, 1, 1)) == [10, 12, 11, 13]


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_round_sums_are_the_partial_sums_of_f(name, p):
    rnd = random.Random(4)
    n = 4
    tables = [_table(rnd, n, p) for _ in range(4)]
    terms = [(p - 1, (0, 0)), (3, (1,))] + GKR_TERMS
    s = M.round_sums(tables, terms, p)
    for x in range(4):
        direct = 0
        for rest in range(1 << (n - 1)):
            direct += M.f_value(tables, terms, [x] + [(rest >> b) & 1 for b in range(n - 1)], p)
        assert s[x] == direct % p
    coeffs = M.interpolate(s, p)
    assert [M.poly_at(coeffs, x, p) for x in range(4)] == s
    assert M.interpolate([0, 0, 0, 0], p) == [] and M.interpolate([7, 7, 7, 7], p) == [7]


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_model_verifier_accepts_its_proof_and_rejects_tampering(name, p):
    rnd = random.Random(5)
    n = 5
    tables = [_table(rnd, n, p) for _ in range(4)]
    for terms, degree in (([(1, (0,))], 1), ([(1, (0, 1))], 2), (GKR_TERMS, 3)):
        claim, rounds, rs = M.prove(tables, terms, p)
        final = lambda pt: M.f_value(tables, terms, pt, p)  # noqa: E731
        assert len(rounds) == n and len(rs) == n
        assert M.verify(n, claim, rounds, degree, p, final=final) == rs
        assert M.verify(n, claim, rounds, degree - 1, p, final=final) is False
        assert M.verify(n, (claim + 1) % p, rounds, degree, p, final=final) is False
        bad = [list(c) for c in rounds]
        bad[2][0] = (bad[2][0] + 1) % p
        assert M.verify(n, claim, bad, degree, p, final=final) is False
        assert M.verify(n, claim, rounds, degree, p, final=lambda pt: (final(pt) + 1) % p) is False


def test_transcript_matches_the_projects():
    from zksnake_amd.transcript import FiatShamirTranscript
    p = BN254_SCALAR_FIELD
    a, b = M.Transcript(b"sumcheck", p), FiatShamirTranscript(b"sumcheck", field=p)
    for item in (0, 5, p - 1, [1, 2, p - 1], 1 << 200):
        a.append(item)
        b.append(item)
        assert a.challenge() == b.get_challenge_scalar()
    with pytest.raises(TypeError):
        a.append([])
    with pytest.raises(TypeError):
        b.append([])


def test_new_symbols_are_exported_and_bound(lib):
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in N.SIGNATURES


def test_new_entry_points_fail_loudly_without_a_gpu(lib):
    if lib.zk_device_count() > 0:
        pytest.skip("a GPU is visible")
    buf = np.zeros((64, 4), dtype=np.uint64)   # stands for device memory: without a device nothing gets as far as reading it
    a, b = buf.ctypes.data, buf.ctypes.data + 32 * 32
    sc = np.ones((4, 4), dtype=np.uint64)
    out = np.zeros((4, 4), dtype=np.uint64)
    perm = np.arange(4, dtype=np.uint8)
    for cid in (0, 1):
        assert lib.zk_mle_fix_dev(cid, 4, a, 2, N.u64p(sc), b, None) == N.ZK_ERR_HIP
        assert lib.zk_mle_fix_dev(cid, 4, a, 0, None, b, None) == N.ZK_ERR_HIP
        assert lib.zk_mle_sum_dev(cid, 16, a, N.u64p(out), None) == N.ZK_ERR_HIP
        assert lib.zk_mle_eval_dev(cid, 4, a, N.u64p(sc), N.u64p(out), b, None) == N.ZK_ERR_HIP
        assert lib.zk_mle_coeffs_dev(cid, 4, a, b, None) == N.ZK_ERR_HIP
        assert lib.zk_mle_permute_dev(cid, 4, a, N.u8p(perm), b, None) == N.ZK_ERR_HIP
        tabs = (ctypes.c_void_p * 1)(a)
        outs = (ctypes.c_void_p * 1)(b)
        deg, idx = (ctypes.c_int * 1)(2), (ctypes.c_int * 3)(0, 0, 0)
        for r, o in ((None, None), (N.u64p(sc), outs)):
            assert lib.zk_sumcheck_round_dev(cid, 4, 1, tabs, 1, N.u64p(sc), deg, idx, r, o, N.u64p(out), None) == N.ZK_ERR_HIP
    # argument errors are found before the device is needed
    assert lib.zk_mle_fix_dev(0, 4, a, 5, N.u64p(sc), b, None) == N.ZK_ERR_ARG
    assert lib.zk_mle_fix_dev(0, 4, a, 1, N.u64p(sc), a + 32, None) == N.ZK_ERR_ARG
    assert lib.zk_mle_permute_dev(0, 4, a, N.u8p(np.array([0, 1, 1, 3], dtype=np.uint8)), b, None) == N.ZK_ERR_ARG
    assert lib.zk_mle_fix_dev(2, 4, a, 1, N.u64p(sc), b, None) == N.ZK_ERR_ARG


def test_header_tile_constant_matches_the_binding():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "zkmi.h")) as f:
        assert int(re.search(r"#define ZK_MLE_TILE_LOG (\d+)", f.read()).group(1)) == N.MLE_TILE_LOG


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_sumcheck_verify_is_host_only_on_a_model_proof(name, p):
    from zksnake_amd.polynomial import Polynomial
    from zksnake_amd.subprotocol.sumcheck import Sumcheck, round_polynomial

    class Final:   # stands for the polynomial in the verifier's last check
        def __init__(self, fn):
            self.evaluate = fn

    rnd = random.Random(6)
    n = 4
    tables = [_table(rnd, n, p) for _ in range(4)]
    claim, rounds, rs = M.prove(tables, GKR_TERMS, p)
    proof = [Polynomial(list(c), p) for c in rounds]
    final = Final(lambda pt: M.f_value(tables, GKR_TERMS, pt, p))
    sc = Sumcheck(n, p)
    assert sc.verify(claim, proof, 3, mlpoly=final) == rs
    assert sc.verify(claim, proof, 3) == rs
    assert sc.verify(claim, proof, 2, mlpoly=final) is False
    assert sc.verify((claim + 1) % p, proof, 3, mlpoly=final) is False
    bad = list(proof)
    bad[1] = Polynomial([(rounds[1][0] + 1) % p] + list(rounds[1][1:]), p)
    assert sc.verify(claim, bad, 3, mlpoly=final) is False
    assert sc.verify(claim, proof, 3, mlpoly=Final(lambda pt: 0)) is False
    # the host interpolation of the prover gives the model's coefficients
    s = M.round_sums(tables, GKR_TERMS, p)
    assert round_polynomial(s, p).coeffs() == M.interpolate(s, p)


# ---- the closed forms on geometric tables (the reference of tests/test_gpu_fr_large.py) against the definitions ----

GEO_SIZES = (0, 1, 2, 5, 9)
GEO_TERMS = {
    "degree 1": [(1, (0,))],
    "degree 2": [(1, (0, 1))],
    "degree 3": [(5, (0, 1, 2))],
    "one table twice": [(-1, (0, 0))],
    "mixed": [(-1, (3, 3, 1)), (3, (2,)), (1, (0, 1)), (0, (1, 2))],
    "gkr": GKR_TERMS,
}


def _root_of_unity_16(p):
    for x in range(2, 50):
        w = pow(x, (p - 1) // 16, p)
        if pow(w, 8, p) != 1:
            return w
    raise AssertionError("no element of order 16 found")


def _geo_ratios(rnd, p):
    """random full-width ratios and the ones at which a series degenerates: g = 1 (a constant table), g = p - 1 (g^2 = 1, and
    1 + X (g - 1) = 0 at X = 1/2), w of order 16 (g^2 becomes 1 after three folds) with w^7 beside it (the product of the two
    squared ratios is 1 at once)"""
    w = _root_of_unity_16(p)
    return {
        "random": [rnd.randrange(2, p) for _ in range(4)],
        "g = 1": [1, rnd.randrange(2, p), 1, 1],
        "g = p - 1": [p - 1, p - 1, rnd.randrange(2, p), p - 1],
        "order 16": [w, pow(w, 7, p), pow(w, 3, p), pow(w, 5, p)],
    }


def _geo_tables(rnd, p, log_n, ratios):
    return [(rnd.randrange(1, p), g, log_n) for g in ratios]


def _terms(terms, p):
    return [(c % p, which) for c, which in terms]


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_geo_sum_is_the_sum(name, p):
    rnd = random.Random(20)
    for ratio in (0, 1, p + 1, p - 1, 2, rnd.randrange(p), _root_of_unity_16(p)):
        first = rnd.randrange(p)
        for count in (1, 2, 5, 16, 33):
            assert M.geo_sum(first, ratio, count, p) == sum(first * pow(ratio, i, p) for i in range(count)) % p


@pytest.mark.parametrize("log_n", GEO_SIZES)
@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_geo_fix_total_coefficients_permute_equal_the_definitions(name, p, log_n):
    rnd = random.Random(21 + log_n)
    for label, ratios in _geo_ratios(rnd, p).items():
        for tab in _geo_tables(rnd, p, log_n, ratios):
            t = M.geo_table(tab, p)
            assert len(t) == 1 << log_n and t[0] == tab[0]
            assert M.geo_total(tab, p) == M.total(t, p), label
            rs = [p - 1, 0, pow(2, -1, p), 1][:log_n] + [rnd.randrange(p) for _ in range(log_n - 4)]
            for k in range(log_n + 1):
                assert M.geo_table(M.geo_fix(tab, rs[:k], p), p) == M.fix(t, rs[:k], p), (label, k)
            assert M.geo_evaluate(tab, rs, p) == M.evaluate(t, rs, p), label
            assert [M.geo_coefficient(tab, i, p) for i in range(1 << log_n)] == M.coefficients(t, p), label
            perm = list(range(log_n))
            rnd.shuffle(perm)
            for pm in (perm, perm[::-1], M.swap_perm(log_n, 0, log_n - 2, 2) if log_n >= 4 else perm):
                assert [M.geo_permuted_at(tab, pm, j, p) for j in range(1 << log_n)] == M.permute(t, pm), (label, pm)


@pytest.mark.parametrize("log_n", GEO_SIZES)
@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_geo_round_sums_equal_the_definition_down_a_chain_of_folds(name, p, log_n):
    """every term shape at every level of a chain of folds from log_n to 0: the closed-form round sums against round_sums on the
    folded lists, and the folded triples against the folded lists"""
    rnd = random.Random(22 + log_n)
    for label, ratios in _geo_ratios(rnd, p).items():
        start = tabs = _geo_tables(rnd, p, log_n, ratios)
        lists = [M.geo_table(t, p) for t in tabs]
        rs = [p - 1, pow(2, -1, p), 0][:log_n] + [rnd.randrange(p) for _ in range(log_n - 3)]
        for level in range(log_n, -1, -1):
            for shape, terms in GEO_TERMS.items():
                terms = _terms(terms, p)
                assert M.geo_round_sums(tabs, terms, p) == M.round_sums(lists, terms, p), (label, shape, level)
            if level:
                r = rs[log_n - level]
                tabs = [M.geo_fix(t, [r], p) for t in tabs]
                lists = [M.fix(t, [r], p) for t in lists]
                assert [M.geo_table(t, p) for t in tabs] == lists, (label, level)
        assert M.geo_f_value(start, GKR_TERMS, rs, p) == M.f_value([M.geo_table(t, p) for t in start], GKR_TERMS, rs, p), label


@pytest.mark.parametrize("shape", ["degree 1", "degree 2", "gkr"])
@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_geo_prove_is_prove(name, p, shape):
    from test_gpu_sumcheck import shapes
    terms = shapes(p)[shape]
    rnd = random.Random(23)
    for log_n in (0, 1, 2, 5, 9):
        for label, ratios in _geo_ratios(rnd, p).items():
            tabs = _geo_tables(rnd, p, log_n, ratios)
            try:
                want = M.prove([M.geo_table(t, p) for t in tabs], terms, p)
            except TypeError:   # one table whose ratio has a small even order: a round polynomial is zero, which no transcript takes
                assert shape == "degree 1" and label in ("g = p - 1", "order 16")
                with pytest.raises(TypeError):
                    M.geo_prove(tabs, terms, p)
                continue
            assert M.geo_prove(tabs, terms, p) == want, (label, log_n)
    tabs = _geo_tables(rnd, p, 5, _geo_ratios(rnd, p)["random"])
    a, b = M.Transcript(b"outer", p), M.Transcript(b"outer", p)
    for tr in (a, b):
        tr.append(99)
    assert M.geo_prove(tabs, terms, p, a) == M.prove([M.geo_table(t, p) for t in tabs], terms, p, b) != M.geo_prove(tabs, terms, p)


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_descending_table_and_its_coefficients(name, p):
    """T[i] = p - 1 - i, built in limbs: the table and its coefficient table (p - 1 at 0, p - 2^b at 2^b, zero elsewhere)"""
    for log_n in (0, 1, 6):
        n = 1 << log_n
        t = N.limbs_to_ints(M.descending_limbs(p, log_n))
        assert t == [p - 1 - i for i in range(n)]
        want = N.limbs_to_ints(M.descending_coefficient_limbs(p, log_n))
        assert want == M.coefficients(t, p)
        assert [i for i, v in enumerate(want) if v] == sorted({0} | {1 << b for b in range(log_n)})
    assert ((p - 1) & ((1 << 64) - 1)) > 1 << 25   # the low limb never borrows at the sizes the GPU tests use
