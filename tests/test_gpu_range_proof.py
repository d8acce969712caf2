"""GPU: RangeProof / RangeProofObject (zksnake_amd/subprotocol/range_proof.py) against the integer model of
tests/range_proof_model.py, which rescales H into H' and folds G, H' every round as the reference does: proof bytes by ==, and
each side's verifier on the other's proofs.

Hashed generators up to N = 16 positions (the folded model in Python integers takes about a second there on BLS12-381);
structured generators G_k = g_k P at N = 64 and 1024, where the model works on exponents and every proof point costs it one
scalar multiplication."""

import hashlib
import random

import pytest

import range_proof_model as M
from oracle import pyref
from zksnake_amd.ecc import CurvePointSize, EllipticCurve
from zksnake_amd.frvec import FrOps
from zksnake_amd.subprotocol import InnerProductProof, RangeProof, RangeProofObject
from zksnake_amd.transcript import FiatShamirTranscript

pytestmark = pytest.mark.gpu

CURVES = ("BN254", "BLS12_381")
C = 0x1234567890ABCDEF1234567890ABCDEF      # the verifier's random c, pinned
_CACHE = {}


def tup(pt):
    return None if pt.is_zero() else (pt.x, pt.y)


def tups(points):
    return [tup(p) for p in points]


def hashed(name, n, m):
    """one object per curve and shape with its model generators (shared; tests that assign generators make their own)"""
    if (name, n, m) not in _CACHE:
        rp = RangeProof(n, name, values=m)
        _CACHE[(name, n, m)] = (rp, (tups(rp.G), tups(rp.H), tup(rp.B), tup(rp.B_blinding)))
    return _CACHE[(name, n, m)]


def randomness(r, n, m, seed):
    rnd = random.Random(seed)
    size = n * m
    s_l, s_r = [rnd.randrange(r) for _ in range(size)], [rnd.randrange(r) for _ in range(size)]
    s_l[0], s_r[-1] = r - 1, 0
    out = {k: rnd.randrange(r) for k in ("a_blinding", "s_blinding", "t1_blinding", "t2_blinding")}
    out.update(s_L=s_l, s_R=s_r, v_blinding=[rnd.randrange(r) for _ in range(m)])
    return out


def in_range_values(n, m, seed):
    rnd = random.Random(seed)
    vals = [rnd.randrange(1 << n) for _ in range(m)]
    vals[0] = (1 << n) - 1
    return vals


def arg(values):
    """what prove takes: an int for one value"""
    return values[0] if len(values) == 1 else values


def to_model(proof):
    ip = proof.ipa_proof
    V = proof.V if isinstance(proof.V, list) else [proof.V]
    return M.Proof(tups(V), tup(proof.A), tup(proof.S), tup(proof.T1), tup(proof.T2), proof.t, proof.t_blinding, proof.e_blinding,
                   ip.a, ip.b, tups(ip.L), tups(ip.R))


def replaced(proof, **kw):
    fields = dict(proof.__dict__)
    fields.update(kw)
    return RangeProofObject(**fields)


def replaced_ipa(proof, **kw):
    ip = proof.ipa_proof
    fields = dict(a=ip.a, b=ip.b, L=ip.L, R=ip.R)
    fields.update(kw)
    return replaced(proof, ipa_proof=InnerProductProof(**fields))


@pytest.mark.parametrize("n,m", [(1, 1), (2, 1), (8, 1), (16, 1), (4, 4), (1, 2)])
@pytest.mark.parametrize("name", CURVES)
def test_hashed_generators_against_the_folded_model(gpu, name, n, m):
    cv = pyref.curve_by_name(name)
    grp = M.PointGroup(cv)
    rp, (G, H, B, Bb) = hashed(name, n, m)
    assert (rp.n, rp.m, len(rp.G), len(rp.H)) == (n, m, n * m, n * m)
    assert (rp.E.name, rp.E.order) == (name, cv.r)
    values = in_range_values(n, m, seed=n + m)
    rnd = randomness(cv.r, n, m, seed=10 * n + m)
    got = rp.prove(arg(values), randomness=rnd if m > 1 else dict(rnd, v_blinding=rnd["v_blinding"][0]))
    want = M.prove(grp, n, m, G, H, B, Bb, values, rnd)
    assert got.to_bytes() == M.proof_bytes(grp, want)
    assert isinstance(got.V, list) == (m > 1)
    assert len(got.ipa_proof.L) == len(got.ipa_proof.R) == (n * m).bit_length() - 1
    assert M.verify(grp, n, m, G, H, B, Bb, to_model(got), C), "the model rejects the GPU proof"
    from_model = RangeProofObject.from_bytes(M.proof_bytes(grp, want), name, values=m)
    assert rp.verify(from_model, c=C) is True, "the GPU rejects the model's proof"
    assert rp.verify(got) is True, "a c of its own"


@pytest.mark.parametrize("n,m", [(64, 1), (32, 32), (8, 128)])
@pytest.mark.parametrize("name", CURVES)
def test_structured_generators_against_the_closed_form(gpu, name, n, m):
    cv = pyref.curve_by_name(name)
    E = EllipticCurve(name)
    r, size = cv.r, n * m
    rnd = random.Random(size + n)
    g = [rnd.randrange(1, r) for _ in range(size)]
    h = [rnd.randrange(1, r) for _ in range(size)]
    beta, beta_b = rnd.randrange(1, r), rnd.randrange(1, r)
    rp = RangeProof(n, name, values=m, generators=(E.batch_mul(E.G1(), g, as_array=True), E.batch_mul(E.G1(), h, as_array=True)))
    rp.B, rp.B_blinding = E.G1() * beta, E.G1() * beta_b
    values = in_range_values(n, m, seed=size)
    randoms = randomness(r, n, m, seed=size + 1)
    got = rp.prove(arg(values), randomness=randoms)
    # the model works on exponents; the generators' bytes come from the device codec (2048 scalar multiplications otherwise)
    digest = hashlib.blake2b(rp.G.to_bytes() + rp.H.to_bytes()).digest()
    grp = M.ExponentGroup(r, cv)
    want = M.prove(grp, n, m, g, h, beta, beta_b, values, randoms, gen_digest=digest)
    assert got.to_bytes() == M.proof_bytes(grp, want)
    assert rp.verify(got, c=C) and rp.verify(got)
    assert M.verify(grp, n, m, g, h, beta, beta_b, want, C, gen_digest=digest)
    # one value past its range, the last bit of the last value's neighbour untouched
    bad = list(values)
    bad[m // 2] += 1 << n
    assert rp.verify(rp.prove(arg(bad), randomness=randoms), c=C) is False
    moved = replaced(got, t=(got.t + 1) % r)
    assert rp.verify(moved, c=C) is False


@pytest.mark.parametrize("name", CURVES)
def test_a_value_out_of_range_gives_a_proof_that_is_rejected(gpu, name):
    cv = pyref.curve_by_name(name)
    grp = M.PointGroup(cv)
    rp, (G, H, B, Bb) = hashed(name, 8, 1)
    rnd = randomness(cv.r, 8, 1, seed=500)
    proof = rp.prove(500, randomness=rnd)
    assert proof.to_bytes() == M.proof_bytes(grp, M.prove(grp, 8, 1, G, H, B, Bb, [500], rnd))
    assert rp.verify(proof, c=C) is False and rp.verify(proof) is False
    assert M.verify(grp, 8, 1, G, H, B, Bb, to_model(proof), C) is False
    assert rp.verify(rp.prove(255, randomness=rnd), c=C) and rp.verify(rp.prove(0, randomness=rnd), c=C)
    # V commits to v mod r, and only the bits below 8 are read
    big = rp.prove(cv.r + 7, randomness=rnd)
    assert big.V == rp.B * 7 + rp.B_blinding * rnd["v_blinding"][0]


@pytest.mark.parametrize("name", CURVES)
def test_verify_rejects_every_tamper(gpu, name):
    cv = pyref.curve_by_name(name)
    E, r = EllipticCurve(name), cv.r
    n, m = 4, 4
    rp, _ = hashed(name, n, m)
    proof = rp.prove(in_range_values(n, m, 1), randomness=randomness(r, n, m, 2))
    assert rp.verify(proof, c=C)
    other = E.G1() * 5
    for field in ("A", "S", "T1", "T2"):
        assert rp.verify(replaced(proof, **{field: getattr(proof, field) + other}), c=C) is False, field
    for j in range(m):
        V = list(proof.V)
        V[j] = V[j] + other
        assert rp.verify(replaced(proof, V=V), c=C) is False, f"V[{j}]"
    for field in ("t", "t_blinding", "e_blinding"):
        assert rp.verify(replaced(proof, **{field: (getattr(proof, field) + 1) % r}), c=C) is False, field
    ip = proof.ipa_proof
    assert rp.verify(replaced_ipa(proof, a=(ip.a + 1) % r), c=C) is False
    assert rp.verify(replaced_ipa(proof, b=(ip.b + 1) % r), c=C) is False
    for j in (0, 3):
        L, R = list(ip.L), list(ip.R)
        L[j], R[j] = L[j] + other, R[j] + other
        assert rp.verify(replaced_ipa(proof, L=L), c=C) is False and rp.verify(replaced_ipa(proof, R=R), c=C) is False, f"round {j}"
    assert rp.verify(replaced(proof, V=[proof.V[1], proof.V[0]] + proof.V[2:]), c=C) is False, "two V swapped"
    assert rp.verify(replaced_ipa(proof, L=ip.L[:-1], R=ip.R[:-1]), c=C) is False, "one round too few"
    # the wrong `values`: the same 16 positions cut into 2 values of 8 bits, and 4 values where 2 are expected
    two, _ = hashed(name, 8, 2)
    assert two.verify(proof, c=C) is False and two.verify(replaced(proof, V=proof.V[:2]), c=C) is False
    assert rp.verify(replaced(proof, V=proof.V[:2]), c=C) is False and rp.verify(replaced(proof, V=proof.V[0]), c=C) is False


@pytest.mark.parametrize("n,m", [(8, 1), (4, 4)])
@pytest.mark.parametrize("name", CURVES)
def test_bytes_round_trip(gpu, name, n, m):
    r = pyref.curve_by_name(name).r
    rp, _ = hashed(name, n, m)
    proof = rp.prove(arg(in_range_values(n, m, 3)), randomness=randomness(r, n, m, 4))
    data = proof.to_bytes()
    rounds = (n * m).bit_length() - 1
    assert len(data) == (m + 4 + 2 * rounds) * CurvePointSize[name].value + 5 * 32
    back = RangeProofObject.from_bytes(data, name, values=m)
    assert back.to_bytes() == data and rp.verify(back, c=C)
    assert (back.V, back.A, back.S, back.T1, back.T2) == (proof.V, proof.A, proof.S, proof.T1, proof.T2)
    assert (back.t, back.t_blinding, back.e_blinding) == (proof.t, proof.t_blinding, proof.e_blinding)
    assert (back.ipa_proof.a, back.ipa_proof.b, back.ipa_proof.L, back.ipa_proof.R) == (proof.ipa_proof.a, proof.ipa_proof.b, proof.ipa_proof.L,
                                                                                        proof.ipa_proof.R)
    with pytest.raises(AssertionError):
        RangeProofObject.from_bytes(data + b"\0", name, values=m)
    if name == "BN254" and m == 1:
        assert RangeProofObject.from_bytes(data).to_bytes() == data, "the reference's defaults"


@pytest.mark.parametrize("name", CURVES)
def test_state_is_not_carried_between_calls(gpu, name):
    cv = pyref.curve_by_name(name)
    E, r = EllipticCurve(name), cv.r
    grp = M.PointGroup(cv)
    n, m = 2, 4
    rp = RangeProof(n, name, values=m)
    G, H, B, Bb = tups(rp.G), tups(rp.H), tup(rp.B), tup(rp.B_blinding)
    v1, v2 = in_range_values(n, m, 1), in_range_values(n, m, 2)
    r1, r2 = randomness(r, n, m, 3), randomness(r, n, m, 4)
    first, second = rp.prove(v1, randomness=r1), rp.prove(v2, randomness=r2)
    assert first.to_bytes() == M.proof_bytes(grp, M.prove(grp, n, m, G, H, B, Bb, v1, r1))
    assert second.to_bytes() == M.proof_bytes(grp, M.prove(grp, n, m, G, H, B, Bb, v2, r2))
    assert RangeProof(n, name, values=m).prove(v2, randomness=r2).to_bytes() == second.to_bytes()
    assert rp.verify(first, c=C) and rp.verify(second, c=C)
    timed = rp.prove(v2, randomness=r2, profile=True)
    assert timed.to_bytes() == second.to_bytes() and len(rp.last_profile["rounds"]) == 3

    # randomness as limb arrays and as device vectors: the same bytes, and the caller's vectors as they were
    ops = FrOps(r)
    ll, lr = ops.limbs(r2["s_L"]), ops.limbs(r2["s_R"])
    keep_l, keep_r = ll.copy(), lr.copy()
    assert rp.prove(v2, randomness=dict(r2, s_L=ll, s_R=lr)).to_bytes() == second.to_bytes()
    assert (ll == keep_l).all() and (lr == keep_r).all()
    dl, dr = ops.d_from(ll), ops.d_from(lr)
    assert rp.prove(v2, randomness=dict(r2, s_L=dl, s_R=dr)).to_bytes() == second.to_bytes()
    assert (dl.download() == keep_l).all() and (dr.download() == keep_r).all()
    with pytest.raises(ValueError):
        rp.prove(v2, randomness=dict(r2, s_L=r2["s_L"][:-1]))
    with pytest.raises(ValueError):
        rp.prove(v2[:-1], randomness=r2)
    with pytest.raises(ValueError):
        rp.prove(v2, randomness={k: v for k, v in r2.items() if k != "t2_blinding"})

    # a transcript that is already in use
    def seeded():
        t = FiatShamirTranscript(b"outer protocol", field=r)
        t.append(12345)
        return t
    inside = rp.prove(v1, transcript=seeded(), randomness=r1)
    assert inside.to_bytes() == M.proof_bytes(grp, M.prove(grp, n, m, G, H, B, Bb, v1, r1, transcript=seeded()))
    assert rp.verify(inside, transcript=seeded(), c=C) and rp.verify(inside, c=C) is False

    # new generators: a list of points for G, a PointArray for H, new B and B_blinding; plan and digest follow
    before = rp._generator_digest()
    new_g = E.batch_mul(E.G1(), [3 + 2 * i for i in range(n * m)])
    new_h = hashed(name, 8, 1)[0].G        # H := the hashed G of another object
    rp.G = new_g
    rp.H = new_h
    rp.B, rp.B_blinding = E.G1() * 11, E.G1() * 13
    assert rp._generator_digest() != before
    moved = rp.prove(v2, randomness=r2)
    want = M.prove(grp, n, m, tups(new_g), tups(new_h), tup(rp.B), tup(rp.B_blinding), v2, r2)
    assert moved.to_bytes() == M.proof_bytes(grp, want) != second.to_bytes()
    assert rp.verify(moved, c=C) and rp.verify(second, c=C) is False
    with pytest.raises(ValueError):
        rp.G = new_g[:4]
    rp.release()
    assert rp.verify(moved, c=C), "the plan is rebuilt on the next use"


@pytest.mark.parametrize("name", CURVES)
def test_default_randomness(gpu, name):
    rp, _ = hashed(name, 4, 4)
    values = in_range_values(4, 4, 9)
    one, two = rp.prove(values), rp.prove(values)
    assert one.to_bytes() != two.to_bytes() and one.V != two.V and one.S != two.S
    assert rp.verify(one) and rp.verify(two)


class FixedTranscript(FiatShamirTranscript):
    """hands out the scalars it was given, then falls back to the hash"""

    def __init__(self, scalars, field):
        super().__init__(b"fixed", field=field)
        self.scalars = list(scalars)

    def get_challenge_scalar(self):
        value = super().get_challenge_scalar()
        return self.scalars.pop(0) if self.scalars else value


@pytest.mark.parametrize("scalars", [[0], [5, 0], [5, 1], [5, 7, 9, 11, 0]], ids=["y=0", "z=0", "z=1", "u=0"])
def test_degenerate_challenges(gpu, scalars):
    r = pyref.BN254.r
    rp, _ = hashed("BN254", 8, 1)
    rnd = randomness(r, 8, 1, 6)
    with pytest.raises(ValueError):
        rp.prove(9, transcript=FixedTranscript(scalars, r), randomness=rnd)
    proof = rp.prove(9, randomness=rnd)
    assert rp.verify(proof, c=C)
    assert rp.verify(proof, transcript=FixedTranscript(scalars, r), c=C) is False
    # y = 1 is an ordinary challenge: the sum of its powers is N, not a quotient by zero
    t = lambda: FixedTranscript([1], r)  # noqa: E731
    assert rp.verify(rp.prove(9, transcript=t(), randomness=rnd), transcript=t(), c=C)


def test_the_reference_test_cases(gpu):
    """the range-proof cases of the reference's tests/test_bulletproofs.py through its import path"""
    from zksnake_amd.subprotocol.bulletproofs import RangeProof as RP
    from zksnake_amd.subprotocol.bulletproofs.range_proof import RangeProofObject as RPO
    for name in CURVES:
        rp = RP(32, name)
        proof = rp.prove(1337)
        assert rp.verify(proof)
        assert rp.verify(RPO.from_bytes(proof.to_bytes(), name))
        rp = RP(8, name)
        assert not rp.verify(rp.prove(500))
