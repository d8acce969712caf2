"""GPU: KZG (zksnake_amd/commitment/polynomial/kzg.py) against integers.  With tau known every commitment is p(tau) G1, so the
model is integer evaluation (tests/pcs_model.py KzgModel): commit = G1 * p(tau), the opening proof = G1 * ((p(tau) - p(z)) / (tau - z))
and the evaluation = p(z); every element of a multi-opening proof is checked the same way.  All comparisons are == on integers
and affine coordinates."""

import random

import numpy as np
import pytest

import pcs_model as M
from oracle import pyref
from test_pcs_model import MULTI_SETS
from zksnake_amd import _native as N
from zksnake_amd.commitment.polynomial import KZG, MultiOpeningQuery
from zksnake_amd.ecc import EllipticCurve
from zksnake_amd.frvec import DevVec, FrOps
from zksnake_amd.polynomial import Polynomial

pytestmark = pytest.mark.gpu

CURVES = ("BN254", "BLS12_381")
TAU = 0x1F2E3D4C5B6A79880102030405060708090A0B0C0D0E0F
_CACHE = {}


def tup(pt):
    return None if pt.is_zero() else (pt.x, pt.y)


def point(E, t):
    return E.curve.PointG1.identity() if t is None else E.curve.PointG1(*t)


def scheme(name, degree):
    """one scheme object and model per curve and size (shared; the test that assigns the SRS makes its own)"""
    if (name, degree) not in _CACHE:
        kzg = KZG(degree, name)
        kzg.setup(tau=TAU)
        _CACHE[(name, degree)] = (kzg, M.KzgModel(pyref.curve_by_name(name), degree, TAU))
    return _CACHE[(name, degree)]


def coefficients(r, count, seed):
    """0 and r-1 scattered through random values; the leading coefficient is not zero"""
    rnd = random.Random(seed)
    out = [rnd.randrange(r) for _ in range(count)]
    for i in range(1, count - 1, 7):
        out[i] = 0 if i % 2 else r - 1
    return out


def check_commit_and_open(kzg, K, poly, z):
    r, g1 = K.cv.r, K.g1
    at_tau, at_z = M.poly_eval(poly, K.tau, r), M.poly_eval(poly, z, r)
    assert tup(kzg.commit(poly)) == g1.mul(g1.gen, at_tau)
    proof, value = kzg.open(poly, z)
    assert value == at_z
    assert tup(proof) == g1.mul(g1.gen, (at_tau - at_z) * pow(K.tau - z, -1, r))
    return proof, value


@pytest.mark.parametrize("degree", [1, 4, 1000, 1 << 16])
@pytest.mark.parametrize("name", CURVES)
def test_commit_and_open_are_integer_evaluation(gpu, name, degree):
    kzg, K = scheme(name, degree)
    r = K.cv.r
    assert len(kzg.G1_tau) == degree + 1 and tup(kzg.G1_tau[degree]) == K.g1.mul(K.g1.gen, pow(TAU, degree, r))
    assert kzg.G2_tau == EllipticCurve(name).G2() * TAU
    rnd = random.Random(degree)
    full = coefficients(r, degree + 1, seed=degree)
    check_commit_and_open(kzg, K, full, rnd.randrange(r))
    check_commit_and_open(kzg, K, full, 0)                               # division by X: the shift branch
    short = coefficients(r, max(degree // 2, 1), seed=degree + 1)        # shorter than the SRS
    check_commit_and_open(kzg, K, short, rnd.randrange(r))
    root = rnd.randrange(1, r)                                           # z a root of p: the evaluation is 0
    rooted = list(full)
    rooted[0] = (rooted[0] - M.poly_eval(full, root, r)) % r
    _, value = check_commit_and_open(kzg, K, rooted, root)
    assert value == 0
    for zero in ([0] * min(degree + 1, 3), []):                          # the zero polynomial
        assert kzg.commit(zero).is_zero()
        proof, value = kzg.open(zero, 5)
        assert proof.is_zero() and value == 0
    with pytest.raises(ValueError):
        kzg.commit([1] * (degree + 2))


@pytest.mark.parametrize("name", CURVES)
def test_the_four_input_kinds_give_equal_results(gpu, name):
    kzg, K = scheme(name, 1000)
    r, ops = K.cv.r, FrOps(K.cv.r)
    poly = coefficients(r, 700, seed=3)
    z = 0xABCDEF
    want = kzg.commit(poly), kzg.open(poly, z)
    limbs = N.ints_to_limbs([x + r if i % 3 == 0 and x + r < 1 << 256 else x for i, x in enumerate(poly)], 4)   # canonicalised on upload
    assert int.from_bytes(limbs[0].tobytes(), "little") >= r
    vec = ops.d_from(ops.limbs(poly))
    assert isinstance(vec, DevVec)
    before, limbs_before = vec.download(), limbs.copy()
    for kind in (Polynomial(poly, r), limbs, vec, tuple(poly)):
        assert kzg.commit(kind) == want[0] and kzg.open(kind, z) == want[1]
    assert (vec.download() == before).all() and (limbs == limbs_before).all()      # the caller's data is never modified


@pytest.mark.parametrize("name", CURVES)
def test_verify_accepts_the_model_and_rejects_tampering(gpu, name):
    kzg, K = scheme(name, 4)
    E, r = EllipticCurve(name), K.cv.r
    poly, z = [1, 3, 3, 7, r - 1], 0x123456789
    commitment, (proof, value) = point(E, K.commit(poly)), K.open(poly, z)
    proof = point(E, proof)
    assert kzg.verify(commitment, proof, z, value)
    assert kzg.verify(commitment, proof, z + r, value + r)
    assert not kzg.verify(commitment + E.G1(), proof, z, value)
    assert not kzg.verify(commitment, proof + E.G1(), z, value)
    assert not kzg.verify(commitment, proof, z + 1, value)
    assert not kzg.verify(commitment, proof, z, (value + 1) % r)
    # the model's pairing check accepts the GPU's proof
    got_proof, got_value = kzg.open(poly, z)
    assert K.verify(tup(kzg.commit(poly)), tup(got_proof), z, got_value)


def build_query(kzg, polys, asks, kinds=None):
    query = MultiOpeningQuery()
    objs = []
    for i, p in enumerate(polys):
        obj = p if kinds is None else kinds[i % len(kinds)](p)
        query.add_polynomial(obj, kzg.commit(p))
        objs.append(obj)
    for i, z in asks:
        query.prover_query(objs[i], z)
    return query


def model_multi(K, polys, asks):
    commitments = [K.commit(p) for p in polys]
    return commitments, M.multi_open(K, polys, commitments, [1] * len(polys), asks)


def check_multi(name, degree, polys, asks, kinds=None):
    kzg, K = scheme(name, degree)
    E, r = EllipticCurve(name), K.cv.r
    commitments, (want, evaluations) = model_multi(K, polys, asks)
    query = build_query(kzg, polys, asks, kinds)
    proof, verifier_query = kzg.multi_open(query)
    assert [tup(x) if not isinstance(x, int) else x for x in proof] == want
    assert [tup(c) for c in verifier_query.commitments] == commitments
    for (z, i), value in evaluations.items():
        assert verifier_query.evaluations[z][i] == value and query.evaluations[z][i] == value
    assert kzg.multi_verify(verifier_query, list(proof))
    from_model = [x if isinstance(x, int) else point(E, x) for x in want]
    assert kzg.multi_verify(verifier_query, from_model), "the GPU verifier rejects the model's proof"
    assert M.multi_verify(K, commitments, asks, evaluations, [tup(x) if not isinstance(x, int) else x for x in proof])
    for k in range(len(proof)):
        bad = list(proof)
        bad[k] = (bad[k] + 1) % r if isinstance(bad[k], int) else bad[k] + E.G1()
        assert not kzg.multi_verify(verifier_query, bad), f"component {k}"
    assert not kzg.multi_verify(verifier_query, proof[:1] + proof[2:])       # one value short
    z0, i0 = next(iter(evaluations))
    verifier_query.evaluations[z0][i0] = (verifier_query.evaluations[z0][i0] + 1) % r
    assert not kzg.multi_verify(verifier_query, list(proof))


@pytest.mark.parametrize("which", sorted(MULTI_SETS))
@pytest.mark.parametrize("name", CURVES)
def test_multi_opening_against_the_model(gpu, name, which):
    polys, asks = MULTI_SETS[which]
    check_multi(name, 4, polys, asks)


@pytest.mark.parametrize("name", CURVES)
def test_multi_opening_of_longer_polynomials_of_every_input_kind(gpu, name):
    r = pyref.curve_by_name(name).r
    ops = FrOps(r)
    polys = [coefficients(r, count, seed=count) for count in (1001, 300, 1, 640)]
    asks = [(0, 11), (0, 0), (0, r - 1), (1, 0), (2, 0), (2, 44), (3, 44), (3, 0)]
    kinds = (lambda p: Polynomial(p, r), lambda p: ops.limbs(p), lambda p: ops.d_from(ops.limbs(p)), list)
    check_multi(name, 1000, polys, asks, kinds)


@pytest.mark.parametrize("name", CURVES)
def test_assigning_the_srs_rebuilds_the_plan(gpu, name):
    E = EllipticCurve(name)
    cv = pyref.curve_by_name(name)
    kzg = KZG(4, name)
    assert not kzg.is_setup
    kzg.setup(tau=99)
    poly = [5, 4, 3, 2, 1]
    first = kzg.commit(poly)
    assert tup(first) == M.KzgModel(cv, 4, 99).commit(poly)
    other, K = scheme(name, 4)
    kzg.G1_tau = other.G1_tau.to_list()              # an existing SRS, as a list of points
    kzg.G2_tau = other.G2_tau
    assert kzg.is_setup and tup(kzg.commit(poly)) == K.commit(poly) != tup(first)
    proof, value = kzg.open(poly, 7)
    assert kzg.verify(kzg.commit(poly), proof, 7, value)
    with pytest.raises(ValueError):
        kzg.G1_tau = other.G1_tau[:3]
    with pytest.raises(TypeError):
        kzg.G2_tau = E.G1()
    drawn = KZG(2, name)
    drawn.setup()                                    # a drawn tau: the scheme agrees with itself
    proof, value = drawn.open([1, 2, 3], 5)
    assert value == 1 + 2 * 5 + 3 * 25 and drawn.verify(drawn.commit([1, 2, 3]), proof, 5, value)
    assert np.any(drawn.G1_tau.limbs[1] != kzg.G1_tau.limbs[1])
