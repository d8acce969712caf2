"""CPU: the integer model of the range proof (tests/range_proof_model.py) is consistent with itself -- prover against verifier
over integers and over curve points, every tamper rejected, the closed form for structured generators against the folded
points byte for byte, the m = 1 check as the reference writes it against the general one, and the five kernel contracts
(unfolded generators, seeded s_inv) against the folded prover -- and the package's RangeProof refuses sizes outside its limits
and draws its randomness below r."""

import random

import numpy as np
import pytest

import ipa_model
import range_proof_model as M
from oracle import pyref
from zksnake_amd.transcript import FiatShamirTranscript

CURVES = ("BN254", "BLS12_381")
SHAPES = [(1, 1), (8, 1), (4, 4), (1, 2)]


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


def integer_setup(r, n, m, seed=1):
    rnd = random.Random(seed)
    size = n * m
    return ([rnd.randrange(1, r) for _ in range(size)], [rnd.randrange(1, r) for _ in range(size)], rnd.randrange(1, r), rnd.randrange(1, r))


@pytest.mark.parametrize("n,m", SHAPES + [(64, 1), (16, 8), (128, 2)])
@pytest.mark.parametrize("name", CURVES)
def test_integers_accept_and_reject_every_tamper(name, n, m):
    r = pyref.curve_by_name(name).r
    grp = M.ExponentGroup(r)
    G, H, B, Bb = integer_setup(r, n, m)
    values = in_range_values(n, m, 3)
    rnd = randomness(r, n, m, 4)
    proof = M.prove(grp, n, m, G, H, B, Bb, values, rnd)
    c = 0x1234567890ABCDEF
    ok = lambda p, mm=m: M.verify(grp, n, mm, G, H, B, Bb, p, c)  # noqa: E731
    assert ok(proof)
    assert len(proof.L) == len(proof.R) == (n * m).bit_length() - 1
    for field in ("A", "S", "T1", "T2", "t", "t_blinding", "e_blinding", "a", "b"):
        assert not ok(proof.replace(**{field: (getattr(proof, field) + 1) % r})), field
    for j in range(m):
        V = list(proof.V)
        V[j] = (V[j] + 1) % r
        assert not ok(proof.replace(V=V)), f"V[{j}]"
    for j in range(len(proof.L)):
        L, R = list(proof.L), list(proof.R)
        L[j], R[j] = (L[j] + 1) % r, (R[j] + 1) % r
        assert not ok(proof.replace(L=L)) and not ok(proof.replace(R=R)), f"round {j}"
    if m > 1:
        assert not ok(proof.replace(V=[proof.V[1], proof.V[0]] + proof.V[2:])), "two V swapped"
        assert not ok(proof, m // 2) and not ok(proof.replace(V=proof.V[:m // 2]), m // 2), "the wrong number of values"
    if proof.L:
        assert not ok(proof.replace(L=proof.L[:-1], R=proof.R[:-1])), "one round too few"
    # out of range: bit n set in one value.  Only bits below n are read and V commits to the whole value: a proof, rejected
    for j in {0, m - 1}:
        bad = list(values)
        bad[j] += 1 << n
        assert not ok(M.prove(grp, n, m, G, H, B, Bb, bad, rnd)), f"value {j} out of range"
    # a transcript already in use, on both sides
    def seeded():
        t = FiatShamirTranscript(b"outer", field=r)
        t.append(77)
        return t
    inside = M.prove(grp, n, m, G, H, B, Bb, values, rnd, transcript=seeded())
    assert M.verify(grp, n, m, G, H, B, Bb, inside, c, transcript=seeded()) and not ok(inside)
    assert M.proof_bytes(grp, inside) != M.proof_bytes(grp, proof)


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("name", CURVES)
def test_closed_form_equals_the_folded_points(name, n, m):
    """(a) over curve points with G_k = g_k P against (b) over the exponents: the same bytes, and each verifier accepts"""
    cv = pyref.curve_by_name(name)
    r = cv.r
    pts, exps = M.PointGroup(cv), M.ExponentGroup(r, cv)
    g, h, beta, beta_b = integer_setup(r, n, m, seed=9)
    P = pts.g.gen
    G, H, B, Bb = [pts.mul(P, x) for x in g], [pts.mul(P, x) for x in h], pts.mul(P, beta), pts.mul(P, beta_b)
    values = in_range_values(n, m, 5)
    rnd = randomness(r, n, m, 6)
    want = M.prove(pts, n, m, G, H, B, Bb, values, rnd)
    got = M.prove(exps, n, m, g, h, beta, beta_b, values, rnd)
    assert M.proof_bytes(exps, got) == M.proof_bytes(pts, want)
    assert M.generator_digest(exps, g, h) == M.generator_digest(pts, G, H)
    c = 987654321
    assert M.verify(pts, n, m, G, H, B, Bb, want, c)
    assert M.verify(exps, n, m, g, h, beta, beta_b, got, c)
    assert not M.verify(pts, n, m, G, H, B, Bb, want.replace(t=(want.t + 1) % r), c)
    bad = list(values)
    bad[-1] += 1 << n
    assert not M.verify(pts, n, m, G, H, B, Bb, M.prove(pts, n, m, G, H, B, Bb, bad, rnd), c)


@pytest.mark.parametrize("n", [1, 8, 32])
@pytest.mark.parametrize("name", CURVES)
def test_single_value_check_as_the_reference_writes_it(name, n):
    r = pyref.curve_by_name(name).r
    grp = M.ExponentGroup(r)
    G, H, B, Bb = integer_setup(r, n, 1, seed=n)
    rnd = randomness(r, n, 1, 12)
    c = 55555
    for value, expect in (((1 << n) - 1, True), (1 << n, False), (0, True)):
        proof = M.prove(grp, n, 1, G, H, B, Bb, [value], rnd)
        assert M.verify(grp, n, 1, G, H, B, Bb, proof, c) is expect
        assert M.verify_single_as_the_reference_writes_it(grp, n, G, H, B, Bb, proof, c) is expect
        moved = proof.replace(e_blinding=(proof.e_blinding + 1) % r)
        assert not M.verify(grp, n, 1, G, H, B, Bb, moved, c)
        assert not M.verify_single_as_the_reference_writes_it(grp, n, G, H, B, Bb, moved, c)


@pytest.mark.parametrize("log_bits,log_N", [(0, 0), (0, 1), (1, 1), (3, 3), (2, 4), (6, 7), (7, 8)])
@pytest.mark.parametrize("name", CURVES)
def test_kernel_contracts_give_the_folded_proof(name, log_bits, log_N):
    """The device path on lists of ints: bits, t(X), l || r with the weights y^-k, the seeded rounds over the ORIGINAL G || H
    and the verifier's scalars reproduce the proof of the prover that rescales H and folds, and its verifier's check."""
    r = pyref.curve_by_name(name).r
    grp = M.ExponentGroup(r)
    n, size = 1 << log_bits, 1 << log_N
    m = size // n
    G, H, B, Bb = integer_setup(r, n, m, seed=log_N)
    values = in_range_values(n, m, 21)
    rnd = randomness(r, n, m, 22)
    proof = M.prove(grp, n, m, G, H, B, Bb, values, rnd)
    bases = G + H
    # bits above n do not matter to any contract
    noisy = [v | (5 << n) for v in values]

    bits = M.bits_contract(log_bits, log_N, noisy, r)
    assert bits == M.bits_contract(log_bits, log_N, values, r)
    assert grp.add(grp.msm(bases, bits), grp.mul(Bb, rnd["a_blinding"])) == proof.A
    transcript = FiatShamirTranscript(M.label(n, m), field=r)
    y, z, x, w, us = M._replay(grp, n, m, G, H, proof, transcript, None)
    y_inv = pow(y, -1, r)
    s = rnd["s_L"] + rnd["s_R"]
    t0, t1, t2 = M.poly_contract(log_bits, log_N, noisy, s, y, z, r)
    assert grp.add(grp.mul(B, t1), grp.mul(Bb, rnd["t1_blinding"])) == proof.T1
    assert grp.add(grp.mul(B, t2), grp.mul(Bb, rnd["t2_blinding"])) == proof.T2
    assert (t0 + t1 * x + t2 * x * x) % r == proof.t
    ab, h_weight = M.eval_contract(log_bits, log_N, noisy, s, y, y_inv, z, x, r)
    assert sum(p * q for p, q in zip(ab[:size], ab[size:])) % r == proof.t
    assert h_weight == [pow(y_inv, k, r) for k in range(size)]

    Q = grp.mul(B, w)
    a, b, sv, s_inv = ab[:size], ab[size:], [None] * size, [None] * size
    u = u_inv = None
    for k in range(log_N + 1):
        res = M.seeded_round_contract(log_N, k, a, b, sv, s_inv, h_weight if k == 0 else None, u, u_inv, r)
        if res is None:
            break
        scal_l, scal_r, cross = res
        assert grp.add(grp.msm(bases, scal_l), grp.mul(Q, cross[0])) == proof.L[k], f"L, round {k}"
        assert grp.add(grp.msm(bases, scal_r), grp.mul(Q, cross[1])) == proof.R[k], f"R, round {k}"
        u, u_inv = us[k], pow(us[k], -1, r)
    assert (a[0], b[0]) == (proof.a, proof.b)
    assert sv == ipa_model.s_vector(us, log_N, r)
    assert s_inv == [pow(p, -1, r) * q % r for p, q in zip(sv, h_weight)]

    scal = M.verify_scalars_contract(log_bits, log_N, us, proof.a, proof.b, y_inv, z, r)
    zj = M.powers(z, m, r, first=z * z)
    assert scal[:size] == [(-z - proof.a * p) % r for p in sv]
    assert scal[size:] == [(z + h_weight[k] * (zj[k // n] * (1 << (k % n)) - proof.b * pow(sv[k], -1, r))) % r for k in range(size)]
    # without weights the seeded round is the plain one
    a1, b1, a2, b2 = list(ab[:size]), list(ab[size:]), list(ab[:size]), list(ab[size:])
    s1, si1, s2, si2 = ([None] * size for _ in range(4))
    assert M.seeded_round_contract(log_N, 0, a1, b1, s1, si1, None, None, None, r) == ipa_model.round_step(log_N, 0, a2, b2, s2, si2, None, None, r)


def test_delta_closed_forms_against_the_sums():
    r = pyref.BN254.r
    for n, m, y, z in ((8, 1, 5, 7), (4, 4, 1, 9), (1, 2, r - 1, r - 2), (16, 8, 12345, 1), (2, 1, r + 1, 3)):
        want = ((z - z * z) * sum(pow(y, k, r) for k in range(n * m)) - sum(pow(z, 3 + j, r) for j in range(m)) * ((1 << n) - 1)) % r
        assert M.delta(n, m, y, z, r) == want


class FixedTranscript(FiatShamirTranscript):
    """hands out the scalars it was given, then falls back to the hash"""

    def __init__(self, scalars, field):
        super().__init__(b"fixed", field=field)
        self.scalars = list(scalars)

    def get_challenge_scalar(self):
        value = super().get_challenge_scalar()
        return self.scalars.pop(0) if self.scalars else value


@pytest.mark.parametrize("scalars", [[0], [5, 0], [5, 1], [5, 7, 9, 11, 0]], ids=["y=0", "z=0", "z=1", "u=0"])
def test_degenerate_challenges(scalars):
    r = pyref.BN254.r
    grp = M.ExponentGroup(r)
    G, H, B, Bb = integer_setup(r, 4, 1)
    rnd = randomness(r, 4, 1, 2)
    with pytest.raises(ValueError):
        M.prove(grp, 4, 1, G, H, B, Bb, [9], rnd, transcript=FixedTranscript(scalars, r))
    proof = M.prove(grp, 4, 1, G, H, B, Bb, [9], rnd)
    assert M.verify(grp, 4, 1, G, H, B, Bb, proof, 3)
    assert M.verify(grp, 4, 1, G, H, B, Bb, proof, 3, transcript=FixedTranscript(scalars, r)) is False


# ---- the package, as far as it goes without a GPU ------------------------------------------------------------------------------
def test_import_paths_and_size_limits():
    from zksnake_amd.subprotocol import RangeProof as A, RangeProofObject as AO
    from zksnake_amd.subprotocol.bulletproofs import InnerProductArgument, InnerProductProof, RangeProof
    from zksnake_amd.subprotocol.bulletproofs.range_proof import RangeProofObject
    from zksnake_amd.subprotocol import ipa
    assert RangeProof is A and RangeProofObject is AO
    assert InnerProductArgument is ipa.InnerProductArgument and InnerProductProof is ipa.InnerProductProof
    for bitsize, values in ((0, 1), (3, 1), (256, 1), (-8, 1), (8, 0), (8, 3), (8, 1 << 19), (128, 1 << 15), (8.0, 1), (True, 1)):
        with pytest.raises(ValueError):
            RangeProof(bitsize, "BN254", values=values)
    rp = RangeProof(2, "BN254", values=2)
    assert (rp.n, rp.m, len(rp.G), len(rp.H)) == (2, 2, 4, 4)
    cv = pyref.BN254
    assert [(p.x, p.y) for p in rp.G] == [ipa_model.h2c(b"RangeProof", b"G", cv, i) for i in range(4)]
    assert [(p.x, p.y) for p in rp.H] == [ipa_model.h2c(b"RangeProof", b"H", cv, i) for i in range(4)]
    assert (rp.B.x, rp.B.y) == ipa_model.h2c(b"RangeProof", b"B", cv)
    assert (rp.B_blinding.x, rp.B_blinding.y) == ipa_model.h2c(b"RangeProof", b"Blinding", cv)
    pts = M.PointGroup(cv)
    assert rp._generator_digest() == M.generator_digest(pts, [(p.x, p.y) for p in rp.G], [(p.x, p.y) for p in rp.H])
    with pytest.raises(ValueError):
        rp.G = rp.G[:2]


@pytest.mark.parametrize("name", CURVES)
def test_default_random_vectors_are_below_the_order(name):
    from zksnake_amd import _native as N
    from zksnake_amd.subprotocol import RangeProof
    r = pyref.curve_by_name(name).r
    rp = RangeProof(1, name)
    limbs = rp.random_vector(4096)
    assert limbs.shape == (4096, 4) and limbs.dtype == np.uint64
    ints = N.limbs_to_ints(limbs)
    assert max(ints) < r
    assert len(set(ints)) == 4096
    # exactly uniform below r means the top bit of the order's length is used: about r's share of 2^bits lies above half
    assert sum(1 for x in ints if x >> (r.bit_length() - 1)) > 512
    again = rp.random()
    assert set(again) == set(M.RANDOMNESS_KEYS) and again["s_L"].shape == (1, 4) and len(again["v_blinding"]) == 1
