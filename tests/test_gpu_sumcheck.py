"""GPU: the sumcheck round kernel and the Sumcheck prover against the integer model (tests/mle_model.py), by ==.

Round kernel: every term shape at log_n in {1, 2, T, T+1, 2T+1} (T = ZK_MLE_TILE_LOG), without a challenge and fused with the
fold; the fused form's tables must equal the fix kernel's and its sums the unfused call on those tables.  One more size,
log_n = 20, is the smallest at which a workgroup of the capped grid takes a second stride."""

import ctypes
import random

import numpy as np
import pytest

import mle_model as M
from zksnake_amd import _native as N
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from zksnake_amd.frvec import DevVec, FrOps
from zksnake_amd.mle import MLE_OBJECT, sumcheck_round
from zksnake_amd.polynomial import MultilinearPolynomial
from zksnake_amd.subprotocol import ProductPolynomial, Sumcheck
from zksnake_amd.transcript import FiatShamirTranscript

pytestmark = pytest.mark.gpu

T = N.MLE_TILE_LOG
FIELDS = (("BN254", BN254_SCALAR_FIELD), ("BLS12_381", BLS12_381_SCALAR_FIELD))
_TABLES = {}


def shapes(p):
    return {
        "degree 1": [(1, (0,))],
        "degree 2": [(1, (0, 1))],
        "degree 3": [(1, (0, 1, 2))],
        "one table twice": [(p - 1, (0, 0))],
        "two terms share a table": [(1, (0, 1)), (p - 1, (0, 2))],
        "gkr": [(1, (0, 1)), (1, (0, 2)), (1, (3, 1, 2))],                 # A B + A C + M B C
        "coefficients 0, 1, r-1": [(0, (0, 1)), (1, (2,)), (p - 1, (3, 3, 1))],
    }


def tables(p, log_n):
    """four random tables with the entries 0 and r-1 (shared, never modified)"""
    if (p, log_n) not in _TABLES:
        rnd = random.Random(31 * log_n + (p & 0xFF))
        out = []
        for _ in range(4):
            t = [rnd.randrange(p) for _ in range(1 << log_n)]
            t[0], t[-1] = 0, p - 1
            out.append(t)
        _TABLES[(p, log_n)] = out
    return _TABLES[(p, log_n)]


def upload(ops, values):
    return ops.d_from(N.ints_to_limbs(values, 4))


def ints(vec, count):
    return N.limbs_to_ints(vec.download(count))


@pytest.mark.parametrize("log_n", [1, 2, T, T + 1, 2 * T + 1])
@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_round_kernel(gpu, name, p, log_n):
    ops = FrOps(p)
    host = tables(p, log_n)
    n = 1 << log_n
    dev = [upload(ops, t) for t in host]
    ptrs = [v.ptr() for v in dev]
    plain_cache, folded = {}, {}
    specials = [0, 1, p - 1, p + 5, random.Random(log_n).randrange(p)]
    for i, (label, terms) in enumerate(shapes(p).items()):
        used = 1 + max(tb for _, which in terms for tb in which)
        # r == NULL
        assert sumcheck_round(ops, log_n, ptrs[:used], terms) == M.round_sums(host, terms, p, plain_cache), label
        # fused with the fold of variable 0; one challenge for all shapes at the largest size keeps the model's work shared
        r = specials[3] if log_n > T + 1 else specials[i % len(specials)]
        if r not in folded:
            folded[r] = ([M.fix(t, [r % p], p) for t in host], {})
        want_tables, cache = folded[r]
        out = [DevVec(n // 2, zero=False) for _ in range(used)]
        raw = np.ascontiguousarray(N.ints_to_limbs([r], 4))
        s = np.zeros((4, 4), dtype=np.uint64)
        arr = ctypes.c_void_p * used
        deg = (ctypes.c_int * len(terms))(*[len(w) for _, w in terms])
        idx = (ctypes.c_int * (3 * len(terms)))()
        for t_i, (_, which) in enumerate(terms):
            for j, tb in enumerate(which):
                idx[3 * t_i + j] = tb
        coeff = N.ints_to_limbs([c for c, _ in terms], 4)
        N.check(gpu.zk_sumcheck_round_dev(ops.cid, log_n, used, arr(*ptrs[:used]), len(terms), N.u64p(coeff), deg, idx, N.u64p(raw),
                                          arr(*[v.ptr() for v in out]), N.u64p(s), None))
        fused = N.limbs_to_ints(s)
        assert fused == M.round_sums(want_tables, terms, p, cache), label
        for tb in range(used):
            assert ints(out[tb], n // 2) == want_tables[tb], label
            fixed = DevVec(n // 2, zero=False)
            N.check(gpu.zk_mle_fix_dev(ops.cid, log_n, ptrs[tb], 1, N.u64p(raw), fixed.ptr(), None))
            assert np.array_equal(fixed.download(n // 2), out[tb].download(n // 2)), label
        assert sumcheck_round(ops, log_n - 1, [v.ptr() for v in out], terms) == fused, label
    for tb in range(4):
        assert ints(dev[tb], n) == host[tb], "an input table was modified"


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_round_kernel_where_the_capped_grid_strides(gpu, name, p):
    ops = FrOps(p)
    log_n = 20
    rnd = random.Random(p & 0xFFFF)
    t = [rnd.getrandbits(250) for _ in range(1 << log_n)]
    d = upload(ops, t)
    for terms in ([(1, (0,))], [(p - 1, (0, 0))]):
        assert sumcheck_round(ops, log_n, [d.ptr()], terms) == M.round_sums([t], terms, p)


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_round_kernel_refuses_bad_arguments(gpu, name, p):
    ops = FrOps(p)
    log_n = 3
    buf = upload(ops, tables(p, 4)[0])
    one = N.ints_to_limbs([1], 4)
    s = np.zeros((4, 4), dtype=np.uint64)
    arr = ctypes.c_void_p * 1

    def call(log_n=log_n, n_tables=1, n_terms=1, deg=2, idx=(0, 0, 0), r=None, out=None):
        return gpu.zk_sumcheck_round_dev(ops.cid, log_n, n_tables, arr(buf.ptr(0)), n_terms, N.u64p(one), (ctypes.c_int * 1)(deg),
                                         (ctypes.c_int * 3)(*idx), r, out, N.u64p(s), None)

    assert call() == N.ZK_OK
    assert call(deg=0) == N.ZK_ERR_ARG and call(deg=4) == N.ZK_ERR_ARG
    assert call(idx=(0, 1, 0)) == N.ZK_ERR_ARG
    assert call(n_tables=0) == N.ZK_ERR_ARG and call(n_tables=9) == N.ZK_ERR_ARG
    assert call(n_terms=0) == N.ZK_ERR_ARG and call(n_terms=9) == N.ZK_ERR_ARG
    assert call(log_n=0, r=N.u64p(one), out=arr(buf.ptr(8))) == N.ZK_ERR_ARG
    assert call(r=N.u64p(one), out=None) == N.ZK_ERR_ARG
    for off in (0, 4, 7):   # a folded table inside its input
        assert call(r=N.u64p(one), out=arr(buf.ptr(off))) == N.ZK_ERR_ARG
    assert ints(buf, 16) == tables(p, 4)[0]


# ---- the protocol ----

def _model_proof(host, terms, p, transcript=None):
    return M.prove(host, terms, p, transcript)


def _coeffs(proof):
    return [u.coeffs() for u in proof]


def test_the_references_own_case(gpu):
    p = BN254_SCALAR_FIELD
    g = MultilinearPolynomial(4, [(5, 1), (6, 1), (7, 1)], p)
    sc = Sumcheck(4, p)
    sum_claim, proof, r_evals = sc.prove(g)
    assert sum_claim == 3
    assert sc.verify(sum_claim, proof, 1, mlpoly=g)
    assert sc.verify(sum_claim, proof, 1, mlpoly=g) == r_evals


@pytest.mark.parametrize("n", [1, 2, T + 1, 16])
@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_prove_matches_the_model(gpu, name, p, n):
    host = tables(p, n)
    polys = [MLE_OBJECT[p].from_evaluations(t, p) for t in host]
    sc = Sumcheck(n, p)
    claim, proof, rs = sc.prove(polys[0])
    assert (claim, _coeffs(proof), rs) == _model_proof(host[:1], [(1, (0,))], p)
    assert sc.verify(claim, proof, 1, mlpoly=polys[0]) == rs
    for label in ("degree 2", "gkr") if n < 16 else ("gkr",):
        terms = shapes(p)[label]
        poly = ProductPolynomial(polys, terms, p)
        claim, proof, rs = sc.prove_arbitrary(poly)
        assert (claim, _coeffs(proof), rs) == _model_proof(host, terms, p), label
        assert sc.verify(claim, proof, poly.degree(), mlpoly=poly) == rs
        assert poly.evaluate(rs) == M.f_value(host, terms, rs, p)
    for t, m in zip(host, polys):
        assert m.to_evaluations() == t, "the prover modified an input polynomial"


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_product_polynomial_table_and_sum(gpu, name, p):
    n = 5
    host = tables(p, n)
    polys = [MLE_OBJECT[p].from_evaluations(t, p) for t in host]
    for terms in shapes(p).values():
        poly = ProductPolynomial(polys, terms, p)
        want = []
        for i in range(1 << n):
            acc = 0
            for c, which in terms:
                for tb in which:
                    c = c * host[tb][i] % p
                acc += c
            want.append(acc % p)
        assert poly.to_evaluations() == want
        assert poly.sum() == sum(want) % p
    with pytest.raises(ValueError):
        ProductPolynomial(polys, [(1, (0, 1, 2, 3))], p)
    with pytest.raises(ValueError):
        ProductPolynomial(polys, [(1, (4,))], p)
    with pytest.raises(ValueError):
        ProductPolynomial(polys + [MLE_OBJECT[p].from_evaluations([1, 2], p)], [(1, (0,))], p)


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_verify_rejects(gpu, name, p):
    from zksnake_amd.polynomial import Polynomial
    n = 4
    host = tables(p, n)
    polys = [MLE_OBJECT[p].from_evaluations(t, p) for t in host]
    terms = shapes(p)["gkr"]
    poly = ProductPolynomial(polys, terms, p)
    sc = Sumcheck(n, p)
    claim, proof, rs = sc.prove_arbitrary(poly)
    assert sc.verify(claim, proof, 3, mlpoly=poly) == rs
    assert sc.verify(claim, proof, 2, mlpoly=poly) is False                      # below the true degree
    assert sc.verify((claim + 1) % p, proof, 3, mlpoly=poly) is False
    for rnd in (0, 2, n - 1):
        bad = list(proof)
        c = proof[rnd].coeffs()
        bad[rnd] = Polynomial([(c[0] + 1) % p] + c[1:], p)
        assert sc.verify(claim, bad, 3, mlpoly=poly) is False
    wrong = ProductPolynomial(polys[::-1], terms, p)
    assert sc.verify(claim, proof, 3, mlpoly=wrong) is False


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_round_function_restarts_when_the_prefix_differs(gpu, name, p):
    n = T + 2
    host = tables(p, n)
    polys = [MLE_OBJECT[p].from_evaluations(t, p) for t in host]
    terms = shapes(p)["gkr"]
    poly = ProductPolynomial(polys, terms, p)
    rnd = random.Random(8)
    rs = [rnd.randrange(p) for _ in range(n)]

    def want(prefix):
        return M.interpolate(M.round_sums([M.fix(t, prefix, p) for t in host], terms, p), p)

    assert poly.first_round().coeffs() == want([])
    assert poly.round_function(rs[:1]).coeffs() == want(rs[:1])
    assert poly.round_function(rs[:2]).coeffs() == want(rs[:2])                  # the cached prefix: one fused fold
    other = [rs[0] + 1, rs[5], rs[6]]
    assert poly.round_function(other).coeffs() == want([x % p for x in other])    # a different prefix, and a longer list
    assert poly.round_function(rs[:2]).coeffs() == want(rs[:2])                  # back, shorter than what is cached
    assert poly.round_function(rs[:2]).coeffs() == want(rs[:2])                  # the same list again
    assert poly.round_function(rs).coeffs() == want(rs)                          # every variable fixed: the constant f(rs)
    assert poly.round_function([]).coeffs() == want([])
    for t, m in zip(host, polys):
        assert m.to_evaluations() == t


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_a_callers_transcript_with_earlier_content(gpu, name, p):
    n = 3
    host = tables(p, n)
    polys = [MLE_OBJECT[p].from_evaluations(t, p) for t in host]
    terms = shapes(p)["two terms share a table"]
    ours, model = FiatShamirTranscript(b"outer", field=p), M.Transcript(b"outer", p)
    for tr in (ours, model):
        tr.append(12345)
        tr.append([7, p - 1])
    assert ours.get_challenge_scalar() == model.challenge()
    sc = Sumcheck(n, p)
    claim, proof, rs = sc.prove_arbitrary(ProductPolynomial(polys, terms, p), ours)
    assert (claim, _coeffs(proof), rs) == M.prove(host, terms, p, model)
    assert (claim, _coeffs(proof), rs) != M.prove(host, terms, p)
    check = FiatShamirTranscript(b"outer", field=p)
    check.append(12345)
    check.append([7, p - 1])
    check.get_challenge_scalar()
    assert sc.verify(claim, proof, 2, transcript=check) == rs
