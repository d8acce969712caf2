"""GPU: IPA (zksnake_amd/commitment/polynomial/ipa.py) against the integer model of tests/pcs_model.py, which folds its
generators every round, keeps b as a vector and builds the verifier's g by polynomial products, as the reference does: proof,
commitment and evaluation by == for given randomness.

Hashed generators up to n = 16 (the folded model in Python integers takes about a second there on BLS12-381); structured
generators G_i = g_i B, H = h B at n = 64 and 1024, where the model needs one scalar multiplication per MSM."""

import random

import pytest

import pcs_model as M
from oracle import pyref
from test_pcs_model import MULTI_SETS
from zksnake_amd.commitment.polynomial import IPA, MultiOpeningQuery
from zksnake_amd.ecc import EllipticCurve
from zksnake_amd.frvec import FrOps
from zksnake_amd.polynomial import Polynomial
from zksnake_amd.transcript import FiatShamirTranscript

pytestmark = pytest.mark.gpu

CURVES = ("BN254", "BLS12_381")
_CACHE = {}


def tup(pt):
    return None if pt.is_zero() else (pt.x, pt.y)


def point(E, t):
    return E.curve.PointG1.identity() if t is None else E.curve.PointG1(*t)


def model_proof(proof):
    return [[tup(p) for p in proof[0]], [tup(p) for p in proof[1]], tup(proof[2]), proof[3], proof[4]]


def package_proof(E, proof):
    return [[point(E, p) for p in proof[0]], [point(E, p) for p in proof[1]], point(E, proof[2]), proof[3], proof[4]]


def hashed(name, degree):
    """one scheme object per curve and size with its model (shared; tests that assign G or H make their own)"""
    if (name, degree) not in _CACHE:
        ipa = IPA(degree, name)
        ipa.setup()
        _CACHE[(name, degree)] = (ipa, M.IpaModel(pyref.curve_by_name(name), [tup(p) for p in ipa.G], tup(ipa.H)))
    return _CACHE[(name, degree)]


def inputs(r, n, length, seed, multi=False):
    """(poly, blinding, point, randomness): 0 and r-1 scattered through the coefficients"""
    rnd = random.Random(seed)
    poly = [rnd.randrange(r) for _ in range(length)]
    poly[0] = r - 1
    for i in range(2, length, 5):
        poly[i] = 0
    randomness = {"poly_r": [rnd.randrange(r) for _ in range(n)], "t_bar": rnd.randrange(1, r)}
    if multi:
        randomness["f_blind"] = rnd.randrange(1, r)
    return poly, rnd.randrange(1, r), rnd.randrange(r), randomness


@pytest.mark.parametrize("degree", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("name", CURVES)
def test_hashed_generators_against_the_folded_model(gpu, name, degree):
    cv, E = pyref.curve_by_name(name), EllipticCurve(name)
    ipa, S = hashed(name, degree)
    n = 1 << (degree - 1).bit_length()
    assert ipa.n == n == len(ipa.G) and ipa.is_setup
    assert S.gens == [M.h2c(b"IPA-PCS", b"G", cv, i) for i in range(n)] and S.H == M.h2c(b"IPA-PCS", b"H", cv, 0)
    poly, blinding, z, randomness = inputs(cv.r, n, min(degree, n), seed=degree)
    commitment = ipa.commit(poly, blinding)
    assert tup(commitment) == S.commit(poly, blinding)
    proof, value = ipa.open(poly, z, commitment, blinding, randomness=randomness)
    want, want_value = S.open(poly, z, tup(commitment), blinding, randomness=randomness)
    assert value == want_value and model_proof(proof) == want
    assert len(proof[0]) == len(proof[1]) == n.bit_length() - 1
    assert ipa.verify(commitment, proof, z, value)
    assert S.verify(tup(commitment), model_proof(proof), z, value), "the model rejects the GPU proof"
    assert ipa.verify(point(E, S.commit(poly, blinding)), package_proof(E, want), z, want_value), "the GPU rejects the model's proof"
    # the randomness as a limb array, the polynomial as a Polynomial: the same proof
    again = dict(randomness, poly_r=FrOps(cv.r).limbs(randomness["poly_r"]))
    assert ipa.open(Polynomial(poly, cv.r), z, commitment, blinding, randomness=again) == (proof, value)


@pytest.mark.parametrize("n,length", [(64, 64), (1024, 1000)])
@pytest.mark.parametrize("name", CURVES)
def test_structured_generators_against_the_closed_form(gpu, name, n, length):
    cv, E = pyref.curve_by_name(name), EllipticCurve(name)
    rnd = random.Random(n)
    g, h = [rnd.randrange(1, cv.r) for _ in range(n)], rnd.randrange(1, cv.r)
    ipa = IPA(n, name)
    assert not ipa.is_setup
    ipa.G, ipa.H = E.batch_mul(E.G1(), g, as_array=True), E.G1() * h      # assigned, not hashed
    assert ipa.is_setup
    S = M.IpaModel(cv, structured=(g, h), gen_bytes=ipa.G.to_bytes() + bytes(ipa.H.to_bytes()))
    poly, blinding, z, randomness = inputs(cv.r, n, length, seed=n + length)
    commitment = ipa.commit(poly, blinding)
    assert tup(commitment) == S.commit(poly, blinding)
    proof, value = ipa.open(poly, z, commitment, blinding, randomness=randomness)
    want, want_value = S.open(poly, z, tup(commitment), blinding, randomness=randomness)
    assert value == want_value and model_proof(proof) == want
    assert ipa.verify(commitment, proof, z, value)
    # z = 0 and z = 1: b = (1, 0, 0, ..) and (1, 1, 1, ..)
    for z in (0, 1):
        proof, value = ipa.open(poly, z, commitment, blinding, randomness=randomness)
        assert (model_proof(proof), value) == S.open(poly, z, tup(commitment), blinding, randomness=randomness)
        assert ipa.verify(commitment, proof, z, value)


@pytest.mark.parametrize("name", CURVES)
def test_verify_rejects_every_tamper(gpu, name):
    cv, E = pyref.curve_by_name(name), EllipticCurve(name)
    r = cv.r
    ipa, _ = hashed(name, 5)
    poly, blinding, z, randomness = inputs(r, 8, 8, seed=77)
    commitment = ipa.commit(poly, blinding)
    proof, value = ipa.open(poly, z, commitment, blinding, randomness=randomness)
    zero, G1 = E.curve.PointG1.identity(), E.G1()
    assert ipa.verify(commitment, proof, z, value)
    assert not ipa.verify(commitment, proof, (z + 1) % r, value)
    assert not ipa.verify(commitment, proof, z, (value + 1) % r)
    assert not ipa.verify(commitment + G1, proof, z, value)
    assert not ipa.verify(zero, proof, z, value)                              # the early False returns
    for k, values in ((2, (zero, proof[2] + G1)), (3, (0, r, (proof[3] + 1) % r)), (4, (0, r, (proof[4] + 1) % r))):
        for new in values:
            bad = list(proof)
            bad[k] = new
            assert not ipa.verify(commitment, bad, z, value), (k, new)
    for side in (0, 1):
        for k in range(3):
            for new in (zero, proof[side][k] + G1):
                bad = [list(proof[0]), list(proof[1])] + proof[2:]
                bad[side][k] = new
                assert not ipa.verify(commitment, bad, z, value), (side, k)
    assert not ipa.verify(commitment, proof[:4], z, value)                    # wrong proof length
    assert not ipa.verify(commitment, proof + [1], z, value)
    assert not ipa.verify(commitment, [proof[0][:2], proof[1][:2]] + proof[2:], z, value)
    assert not ipa.verify(commitment, [proof[0] + [G1], proof[1] + [G1]] + proof[2:], z, value)


@pytest.mark.parametrize("name", CURVES)
def test_a_callers_transcript_and_drawn_randomness(gpu, name):
    cv = pyref.curve_by_name(name)
    r = cv.r
    ipa, S = hashed(name, 5)
    poly, blinding, z, randomness = inputs(r, 8, 6, seed=5)
    commitment = ipa.commit(poly, blinding)
    mine = lambda: FiatShamirTranscript(b"a caller's transcript", field=r)  # noqa: E731
    proof, value = ipa.open(poly, z, commitment, blinding, mine(), randomness=randomness)
    assert (model_proof(proof), value) == S.open(poly, z, tup(commitment), blinding, mine(), randomness=randomness)
    assert ipa.verify(commitment, proof, z, value, mine())
    assert not ipa.verify(commitment, proof, z, value)
    # no randomness given: two openings differ, both verify
    first, _ = ipa.open(poly, z, commitment, blinding)
    second, _ = ipa.open(poly, z, commitment, blinding)
    assert first[2] != second[2] and first[3] != second[3]
    assert ipa.verify(commitment, first, z, value) and ipa.verify(commitment, second, z, value)
    drawn = ipa.random()
    assert set(drawn) == {"poly_r", "t_bar"} and drawn["poly_r"].shape == (8, 4)
    with pytest.raises(ValueError):
        ipa.commit([1] * 9, 1)


@pytest.mark.parametrize("which", sorted(MULTI_SETS))
@pytest.mark.parametrize("name", CURVES)
def test_multi_opening_against_the_model(gpu, name, which):
    cv, E = pyref.curve_by_name(name), EllipticCurve(name)
    r = cv.r
    polys, asks = MULTI_SETS[which]
    ipa, S = hashed(name, 4)
    rnd = random.Random(len(asks))
    blindings = [rnd.randrange(1, r) for _ in polys]
    _, _, _, randomness = inputs(r, 4, 4, seed=9, multi=True)
    query = MultiOpeningQuery()
    objs = [Polynomial(p, r) if i % 2 else list(p) for i, p in enumerate(polys)]
    for obj, p, t in zip(objs, polys, blindings):
        query.add_polynomial(obj, ipa.commit(p, t), t)
    for i, z in asks:
        query.prover_query(objs[i], z)
    proof, verifier_query = ipa.multi_open(query, randomness=randomness)
    commitments = [S.commit(p, t) for p, t in zip(polys, blindings)]
    want, evaluations = M.multi_open(S, polys, commitments, blindings, asks, randomness=randomness)
    flat = proof[:-1] + [model_proof(proof[-1])]
    assert [x if isinstance(x, (int, list)) else tup(x) for x in flat] == want
    for (z, i), value in evaluations.items():
        assert verifier_query.evaluations[z][i] == value
    assert ipa.multi_verify(verifier_query, list(proof))
    assert M.multi_verify(S, commitments, asks, evaluations, want)
    from_model = [point(E, want[0])] + want[1:-1] + [package_proof(E, want[-1])]
    assert ipa.multi_verify(verifier_query, from_model), "the GPU verifier rejects the model's proof"
    for k in range(len(proof) - 1):
        bad = list(proof)
        bad[k] = (bad[k] + 1) % r if isinstance(bad[k], int) else bad[k] + E.G1()
        assert not ipa.multi_verify(verifier_query, bad), f"component {k}"
    bad = list(proof)
    bad[-1] = proof[-1][:3] + [(proof[-1][3] + 1) % r] + proof[-1][4:]
    assert not ipa.multi_verify(verifier_query, bad)
    # drawn randomness: the scheme agrees with itself
    proof, verifier_query = ipa.multi_open(query)
    assert ipa.multi_verify(verifier_query, proof)


def test_sizes_above_the_limit_are_refused(gpu):
    with pytest.raises(ValueError):
        IPA((1 << 21) + 1, "BN254")
