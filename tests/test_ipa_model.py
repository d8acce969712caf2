"""CPU: the integer model of the inner-product argument (tests/ipa_model.py) is consistent with itself -- the folded
prover against the verifier, the closed form for structured generators, and the unfolded scalars of the two kernels'
contracts against the folded generators -- and the package's hash_to_curve / hash_to_scalar do what transcript.py says."""

import random

import pytest

import ipa_model as M
from oracle import pyref
from zksnake_amd.ecc import EllipticCurve
from zksnake_amd.transcript import FiatShamirTranscript, hash_to_curve, hash_to_scalar

CURVES = ("BN254", "BLS12_381")
_GENS = {}


def gens(name, n):
    """hashed generators G, H of the model (shared, never modified)"""
    if (name, n) not in _GENS:
        cv = pyref.curve_by_name(name)
        _GENS[(name, n)] = ([M.h2c(b"model", b"G", cv, i) for i in range(n)], [M.h2c(b"model", b"H", cv, i) for i in range(n)])
    return _GENS[(name, n)]


def vectors(cv, n, seed):
    rnd = random.Random(seed)
    a = [rnd.randrange(cv.r) for _ in range(n)]
    b = [rnd.randrange(cv.r) for _ in range(n)]
    a[0] = cv.r - 1
    if n > 2:
        b[1], a[n - 1] = 0, 0
    return a, b


@pytest.mark.parametrize("n", [1, 2, 4, 8])
@pytest.mark.parametrize("name", CURVES)
def test_model_verifier_accepts_and_rejects_every_tamper(name, n):
    cv = pyref.curve_by_name(name)
    grp = pyref.G1(cv)
    G, H = gens(name, n)
    a, b = vectors(cv, n, 5 + n)
    proof, com, ab = M.prove(cv, G, H, a, b)
    assert ab == sum(x * y for x, y in zip(a, b)) % cv.r
    assert M.verify(cv, G, H, proof, com, ab)
    other = grp.mul(grp.gen, 7)
    assert not M.verify(cv, G, H, M.Proof((proof.a + 1) % cv.r, proof.b, proof.L, proof.R), com, ab)
    assert not M.verify(cv, G, H, M.Proof(proof.a, (proof.b + 1) % cv.r, proof.L, proof.R), com, ab)
    assert not M.verify(cv, G, H, proof, com, (ab + 1) % cv.r)
    assert not M.verify(cv, G, H, proof, grp.add(com, other), ab)
    for j in range(len(proof.L)):
        L = list(proof.L)
        L[j] = grp.add(L[j], other)
        assert not M.verify(cv, G, H, M.Proof(proof.a, proof.b, L, proof.R), com, ab)
        R = list(proof.R)
        R[j] = grp.add(R[j], other)
        assert not M.verify(cv, G, H, M.Proof(proof.a, proof.b, proof.L, R), com, ab)
    if n > 1:
        assert not M.verify(cv, G, H, M.Proof(proof.a, proof.b, proof.L[:-1], proof.R[:-1]), com, ab)
    # a given Q is used by both sides, and a proof made with it does not pass as one made without
    Q = grp.mul(grp.gen, 99)
    proof_q, com_q, ab_q = M.prove(cv, G, H, a, b, Q=Q)
    assert M.verify(cv, G, H, proof_q, com_q, ab_q, Q=Q)
    if n > 1:
        assert not M.verify(cv, G, H, proof_q, com_q, ab_q)


@pytest.mark.parametrize("q", [None, 12345])
@pytest.mark.parametrize("name", CURVES)
def test_closed_form_equals_the_folded_model(name, q):
    cv = pyref.curve_by_name(name)
    grp, n = pyref.G1(cv), 8
    rnd = random.Random(3)
    g = [rnd.randrange(1, cv.r) for _ in range(n)]
    h = [rnd.randrange(1, cv.r) for _ in range(n)]
    G, H = [grp.mul(grp.gen, x) for x in g], [grp.mul(grp.gen, x) for x in h]
    a, b = vectors(cv, 5, 8)     # shorter than n: zero padded by both
    Q = None if q is None else grp.mul(grp.gen, q)
    want = M.prove(cv, G, H, a, b, Q=Q)
    got = M.closed_form(cv, g, h, a, b, q=q)
    assert M.proof_bytes(cv, got[0]) == M.proof_bytes(cv, want[0])
    assert got[1:] == want[1:]
    assert M.verify(cv, G, H, got[0], got[1], got[2], Q=Q)


@pytest.mark.parametrize("log_n", [0, 1, 2, 3])
@pytest.mark.parametrize("name", CURVES)
def test_unfolded_scalars_give_the_folded_points(name, log_n):
    """the kernels' contract: L_k = <scal_L, G || H> + cross_L Q over the ORIGINAL generators equals the folded prover's L_k, the
    last a[0], b[0] are the proof's, and the verifier's scalars are a s_i, b / s_i"""
    cv = pyref.curve_by_name(name)
    grp, r, n = pyref.G1(cv), cv.r, 1 << log_n
    G, H = gens(name, n)
    a, b = vectors(cv, n, 40 + log_n)
    Q = grp.mul(grp.gen, 31337)
    transcript = FiatShamirTranscript(b"seeded", field=r)
    transcript.append(b"something before")
    proof, _, _ = M.prove(cv, G, H, a, b, Q=Q, transcript=transcript)
    # the same challenges again
    transcript = FiatShamirTranscript(b"seeded", field=r)
    transcript.append(b"something before")
    M._start(cv, G, H, transcript)
    a, b, s, s_inv = list(a), list(b), [None] * n, [None] * n
    u = u_inv = None
    us = []
    for k in range(log_n + 1):
        res = M.round_step(log_n, k, a, b, s, s_inv, u, u_inv, r)
        if res is None:
            break
        scal_l, scal_r, cross = res
        L = grp.add(grp.msm(list(G) + list(H), scal_l), grp.mul(Q, cross[0]))
        R = grp.add(grp.msm(list(G) + list(H), scal_r), grp.mul(Q, cross[1]))
        assert (L, R) == (proof.L[k], proof.R[k]), f"round {k}"
        transcript.append(pyref.compress(cv, 1, L))
        transcript.append(pyref.compress(cv, 1, R))
        u = transcript.get_challenge_scalar()
        u_inv = pow(u, -1, r)
        us.append(u)
    assert (a[0], b[0]) == (proof.a, proof.b)
    sv = M.s_vector(us, log_n, r)
    assert s == sv and s_inv == [pow(x, -1, r) for x in sv]
    assert M.verify_scalars(log_n, us, proof.a, proof.b, r) == [proof.a * x % r for x in sv] + [proof.b * pow(x, -1, r) % r for x in sv]


@pytest.mark.parametrize("name", CURVES)
def test_hash_to_curve(name):
    cv = pyref.curve_by_name(name)
    grp = pyref.G1(cv)
    E = EllipticCurve(name)
    pts = hash_to_curve(b"seed", b"G", name, 4)
    assert isinstance(pts, list) and len(pts) == 4
    one = hash_to_curve(b"seed", b"G", name)
    assert isinstance(one, E.curve.PointG1) and one == pts[0], "size = 1 is a point, and point i does not depend on size"
    assert hash_to_curve(b"seed", b"G", name, 4) == pts
    as_ints = [(p.x, p.y) for p in pts]
    assert as_ints == [M.h2c(b"seed", b"G", cv, i) for i in range(4)]
    for p in as_ints:
        assert grp.is_on_curve(p)
        assert pyref.ec_mul(grp.F, p, cv.r) is None, "not in the subgroup of order r"
    seen = set(as_ints)
    seen.add(tuple([hash_to_curve(b"seed", b"H", name).x, hash_to_curve(b"seed", b"H", name).y]))
    seen.add(tuple([hash_to_curve(b"seee", b"G", name).x, hash_to_curve(b"seee", b"G", name).y]))
    # the framing keeps (dst, data) pairs apart that concatenate to the same bytes
    seen.add(tuple([hash_to_curve(b"eed", b"Gs", name).x, hash_to_curve(b"eed", b"Gs", name).y]))
    assert len(seen) == 7
    assert hash_to_scalar(b"seed", b"G", name) == M.h2s(b"seed", b"G", cv) < cv.r
    assert hash_to_scalar(b"seed", b"G", name) != hash_to_scalar(b"seed", b"H", name)


def test_sizes_beyond_the_largest_plan_are_refused():
    """2n bases must fit the largest split-scalar MSM plan (2^22 points): refused before a single generator is hashed"""
    from zksnake_amd.subprotocol import InnerProductArgument
    with pytest.raises(ValueError):
        InnerProductArgument((1 << 21) + 1, "BN254")
