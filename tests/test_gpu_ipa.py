"""GPU: InnerProductArgument / InnerProductProof (zksnake_amd/subprotocol/ipa.py) against the integer model of
tests/ipa_model.py, which folds its generators every round as the reference does: proof bytes, commitment and <a, b> by ==.

Hashed generators up to n = 16 (the folded model in Python integers takes about a second there on BLS12-381); structured
generators G_i = g_i B at n = 64 and 1024, where the model's closed form needs one scalar multiplication per MSM."""

import random

import pytest

import ipa_model as M
from oracle import pyref
from zksnake_amd.ecc import CurvePointSize, EllipticCurve
from zksnake_amd.frvec import FrOps
from zksnake_amd.subprotocol import InnerProductArgument, InnerProductProof
from zksnake_amd.transcript import FiatShamirTranscript

pytestmark = pytest.mark.gpu

CURVES = ("BN254", "BLS12_381")
_CACHE = {}


def tup(pt):
    return None if pt.is_zero() else (pt.x, pt.y)


def tups(points):
    return [tup(p) for p in points]


def model_proof(proof):
    return M.Proof(proof.a, proof.b, tups(proof.L), tups(proof.R))


def point_bytes(cv, pt):
    return pyref.compress(cv, 1, pt)


def vectors(r, n, seed, zero_a=False):
    """scattered zeros and r-1 among random values; or a all zero"""
    rnd = random.Random(seed)
    a = [0] * n if zero_a else [rnd.randrange(r) for _ in range(n)]
    b = [rnd.randrange(r) for _ in range(n)]
    if not zero_a:
        a[0] = r - 1
        for i in range(2, n, 5):
            a[i] = 0
    for i in range(1, n, 7):
        b[i] = r - 1 if i % 2 else 0
    return a, b


def hashed(name, n):
    """one argument object per curve and size with its model generators (shared; tests that assign G or H make their own)"""
    if (name, n) not in _CACHE:
        ipa = InnerProductArgument(n, name)
        _CACHE[(name, n)] = (ipa, tups(ipa.G), tups(ipa.H))
    return _CACHE[(name, n)]


def assert_same(cv, got, want):
    proof, com, ab = got
    assert proof.to_bytes() == M.proof_bytes(cv, want[0])
    assert bytes(com.to_bytes()) == point_bytes(cv, want[1])
    assert ab == want[2]


@pytest.mark.parametrize("length", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("name", CURVES)
def test_hashed_generators_against_the_folded_model(gpu, name, length):
    cv = pyref.curve_by_name(name)
    n = 1 << (length - 1).bit_length()
    ipa, G, H = hashed(name, n)
    assert ipa.n == n and len(ipa.G) == len(ipa.H) == n
    assert G == [M.h2c(b"InnerProductProof", b"G", cv, i) for i in range(n)]
    a, b = vectors(cv.r, length, seed=length)
    got = ipa.prove(a, b)
    want = M.prove(cv, G, H, a, b)
    assert_same(cv, got, want)
    assert len(got[0].L) == len(got[0].R) == n.bit_length() - 1
    assert M.verify(cv, G, H, model_proof(got[0]), tup(got[1]), got[2]), "the model rejects the GPU proof"
    from_model = InnerProductProof.from_bytes(M.proof_bytes(cv, want[0]), name)
    assert ipa.verify(from_model, EllipticCurve(name).from_hex(point_bytes(cv, want[1]).hex()), want[2]), "the GPU rejects the model's proof"


@pytest.mark.parametrize("n,length,zero_a,with_q", [(64, 64, False, True), (64, 64, True, False), (1024, 1000, False, False),
                                                   (1024, 1000, True, True)])
@pytest.mark.parametrize("name", CURVES)
def test_structured_generators_against_the_closed_form(gpu, name, n, length, zero_a, with_q):
    cv = pyref.curve_by_name(name)
    E = EllipticCurve(name)
    rnd = random.Random(n)
    g = [rnd.randrange(1, cv.r) for _ in range(n)]
    h = [rnd.randrange(1, cv.r) for _ in range(n)]
    Q = E.G1() * 424242 if with_q else None
    G, H = E.batch_mul(E.G1(), g, as_array=True), E.batch_mul(E.G1(), h, as_array=True)
    if n == 64:
        ipa = InnerProductArgument(n, name, Q=Q)     # hashed generators first, then assigned as a range proof does
        ipa.G, ipa.H = G, H
    else:
        ipa = InnerProductArgument(n, name, Q=Q, generators=(G, H))
    a, b = vectors(cv.r, length, seed=n + length, zero_a=zero_a)
    got = ipa.prove(a, b)
    # at 64 the closed form makes the generators' bytes itself; at 1024 that would be 2048 scalar multiplications in Python
    gen_bytes = None if n == 64 else ipa.G.to_bytes() + ipa.H.to_bytes()
    want = M.closed_form(cv, g, h, a, b, q=424242 if with_q else None, gen_bytes=gen_bytes)
    assert_same(cv, got, want)
    assert ipa.verify(*got)
    limbs = FrOps(cv.r).limbs(a)
    again = ipa.prove(limbs, b)      # a limb array in place of a list: the same proof
    assert again[0].to_bytes() == got[0].to_bytes()


@pytest.mark.parametrize("name", CURVES)
def test_verify_rejects_every_tamper(gpu, name):
    cv = pyref.curve_by_name(name)
    E = EllipticCurve(name)
    ipa, _, _ = hashed(name, 8)
    a, b = vectors(cv.r, 8, seed=77)
    proof, com, ab = ipa.prove(a, b)
    assert ipa.verify(proof, com, ab)
    data = proof.to_bytes()
    assert len(data) == 2 * 3 * CurvePointSize[name].value + 64
    back = InnerProductProof.from_bytes(data, name)
    assert (back.a, back.b, back.L, back.R) == (proof.a, proof.b, proof.L, proof.R) and back.to_bytes() == data
    with pytest.raises(AssertionError):
        InnerProductProof.from_bytes(data + b"\0", name)
    other = E.G1() * 5
    P = InnerProductProof
    assert not ipa.verify(P((proof.a + 1) % cv.r, proof.b, proof.L, proof.R), com, ab)
    assert not ipa.verify(P(proof.a, (proof.b + 1) % cv.r, proof.L, proof.R), com, ab)
    assert not ipa.verify(proof, com, (ab + 1) % cv.r)
    assert not ipa.verify(proof, com + other, ab)
    for j in (0, 2):
        L, R = list(proof.L), list(proof.R)
        L[j] = L[j] + other
        R[j] = R[j] + other
        assert not ipa.verify(P(proof.a, proof.b, L, proof.R), com, ab)
        assert not ipa.verify(P(proof.a, proof.b, proof.L, R), com, ab)
    assert ipa.verify(P(proof.a, proof.b, proof.L[:-1], proof.R[:-1]), com, ab) is False, "one round too few"
    with pytest.raises(AssertionError):
        ipa.verify(P(proof.a, proof.b, proof.L * 11, proof.R * 11), com, ab)
    # a proof made with a given Q passes with that Q only (the reference's verifier cannot check these at all)
    given = InnerProductArgument(8, name, Q=other)
    proof_q, com_q, ab_q = given.prove(a, b)
    assert given.verify(proof_q, com_q, ab_q)
    assert not ipa.verify(proof_q, com_q, ab_q)


@pytest.mark.parametrize("name", CURVES)
def test_state_is_not_carried_between_calls(gpu, name):
    cv = pyref.curve_by_name(name)
    E = EllipticCurve(name)
    ipa = InnerProductArgument(8, name)
    G, H = tups(ipa.G), tups(ipa.H)
    a1, b1 = vectors(cv.r, 8, seed=1)
    a2, b2 = vectors(cv.r, 6, seed=2)
    first = ipa.prove(a1, b1)
    second = ipa.prove(a2, b2)
    assert_same(cv, first, M.prove(cv, G, H, a1, b1))
    assert_same(cv, second, M.prove(cv, G, H, a2, b2))
    fresh = InnerProductArgument(8, name).prove(a2, b2)
    assert fresh[0].to_bytes() == second[0].to_bytes() and fresh[1] == second[1]
    # the profiled form runs the two MSMs of a round one after the other: the same proof, and a record per round
    timed = ipa.prove(a2, b2, profile=True)
    assert timed[0].to_bytes() == second[0].to_bytes() and [r["round"] for r in ipa.last_profile] == [0, 1, 2]

    # new generators: a list of points for G, a PointArray for H; the plan and the cached bytes follow
    g = [3 + 2 * i for i in range(8)]
    new_g = E.batch_mul(E.G1(), g)
    new_h = hashed(name, 8)[0].G        # H := the hashed G
    ipa.G = new_g
    ipa.H = new_h
    moved = ipa.prove(a2, b2)
    assert_same(cv, moved, M.prove(cv, tups(new_g), G, a2, b2))
    assert moved[0].to_bytes() != second[0].to_bytes()
    assert ipa.verify(*moved)
    with pytest.raises(ValueError):
        ipa.G = new_g[:4]

    # a transcript that is already in use: the model's challenges
    def seeded():
        t = FiatShamirTranscript(b"outer protocol", field=cv.r)
        t.append(12345)
        return t
    inside = ipa.prove(a1, b1, transcript=seeded())
    assert_same(cv, inside, M.prove(cv, tups(new_g), G, a1, b1, transcript=seeded()))
    assert ipa.verify(*inside, transcript=seeded())
    assert not ipa.verify(*inside)

    # device-resident inputs: the same proof, and the caller's vectors as they were
    ops = FrOps(cv.r)
    la, lb = ops.limbs(a1), ops.limbs(b1)
    da, db = ops.d_from(la), ops.d_from(lb)
    on_device = ipa.prove(da, db, transcript=seeded())
    assert on_device[0].to_bytes() == inside[0].to_bytes() and on_device[2] == inside[2]
    assert (da.download() == la).all() and (db.download() == lb).all()


def test_one_element_has_no_rounds(gpu):
    ipa, G, H = hashed("BN254", 1)
    proof, com, ab = ipa.prove([5], [7])
    assert (proof.a, proof.b, proof.L, proof.R, ab) == (5, 7, [], [], 35)
    assert len(proof.to_bytes()) == 64
    assert ipa.verify(proof, com, ab) and not ipa.verify(proof, com, 36)
