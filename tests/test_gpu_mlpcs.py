"""GPU: MultilinearKZG (commitment/polynomial/mkzg.py) against the integer model (tests/mlpcs_model.py).  With a known trapdoor
a commitment is f(tau) G and a proof element q_k(tau_(k+1) ..) G: the expected scalar comes from the model and the expected point
from ONE host scalar multiplication; comparisons are ==.  The scheme has 10 variables (setup is instant), which leaves room for
m = T + 1 = 9 < n, the first size at which an opening runs two kernel passes, and for every m < n through the higher levels."""

import random

import pytest

import mlpcs_model as M
from helpers import CURVES
from zksnake_amd import _native as N
from zksnake_amd.commitment.polynomial import MultilinearKZG
from zksnake_amd.frvec import FrOps
from zksnake_amd.mle import MLE_OBJECT
from zksnake_amd.transcript import FiatShamirTranscript

pytestmark = pytest.mark.gpu

T = N.MLE_TILE_LOG
NV = 10
per_curve = pytest.mark.parametrize("name,cid", CURVES, ids=[c[0] for c in CURVES])
_SCHEMES = {}


def trapdoor(p):
    rnd = random.Random(2024)
    return [rnd.randrange(p) for _ in range(NV - 3)] + [0, 1, p - 1]    # the ends of the range among the last variables


def scheme(gpu, name):
    """one scheme per curve, set up once and shared; the tests do not change it"""
    if name not in _SCHEMES:
        s = MultilinearKZG(NV, name)
        s.setup(tau=trapdoor(s.order))
        _SCHEMES[name] = s
    return _SCHEMES[name]


def table(p, m, seed=0):
    rnd = random.Random(100 * m + seed)
    t = [rnd.randrange(p) for _ in range(1 << m)]
    t[-1] = p - 1
    if m:
        t[0] = 0
    return t


def point(p, m, seed=0):
    rnd = random.Random(7 * m + seed)
    z = [rnd.randrange(p) for _ in range(m)]
    for i, v in enumerate([1, 0, p - 1][:m]):      # the ends of the range last, none equal to the trapdoor's coordinate there
        z[m - 1 - i] = v
    return z


@per_curve
@pytest.mark.parametrize("m", [0, 1, 2, T + 1, NV])
def test_commitment_and_proof_are_the_models_points(gpu, name, cid, m):
    s = scheme(gpu, name)
    p, G, tau = s.order, s.E.G1(), trapdoor(s.order)
    t, z = table(p, m), point(p, m)
    assert s.commit(t) == G * M.commit(t, tau, p)
    proof, v = s.open(t, z)
    want_q, want_v = M.open_(t, z, tau, p)
    assert v == want_v == M.evaluate(t, z, p)
    assert len(proof) == m and proof == [G * q for q in want_q]
    assert s.verify(s.commit(t), proof, z, v)


@per_curve
def test_every_input_form_gives_the_same_commitment_and_proof(gpu, name, cid):
    s = scheme(gpu, name)
    p, ops = s.order, FrOps(s.order)
    m = 5
    t, z = table(p, m), point(p, m)
    big = N.ints_to_limbs([v + p if v < p // 4 else v for v in t], 4)    # a limb table with entries >= r is reduced on the device
    forms = [t, tuple(t), N.ints_to_limbs(t, 4), big, ops.d_from(N.ints_to_limbs(t, 4)), MLE_OBJECT[p].from_evaluations(t, p)]
    want_c, (want_proof, want_v) = s.commit(t), s.open(t, z)
    for form in forms:
        assert s.commit(form) == want_c
        assert s.open(form, z) == (want_proof, want_v)
    assert forms[-1].to_evaluations() == t and N.limbs_to_ints(forms[-2].download()) == t, "an input was modified"
    other = MLE_OBJECT[next(k for k in MLE_OBJECT if k != p)]
    with pytest.raises(TypeError):
        s.commit(other.from_evaluations([1, 2], other.p))                # a polynomial over the other curve's field
    with pytest.raises(ValueError):
        s.open(t, z[:-1])
    with pytest.raises(ValueError):
        s.commit([1] * (2 << NV))


@per_curve
def test_zero_and_constant_polynomials(gpu, name, cid):
    s = scheme(gpu, name)
    p, G = s.order, s.E.G1()
    for m in (0, 3, T + 1):
        z = point(p, m)
        for value in (0, 5, p - 1):
            t = [value] * (1 << m)
            c = s.commit(t)
            proof, v = s.open(t, z)
            assert c == G * value and v == value and (value != 0 or c.is_zero())
            assert len(proof) == m and all(q.is_zero() for q in proof)
            assert s.verify(c, proof, z, v) and not s.verify(c, proof, z, (v + 1) % p)


@per_curve
def test_the_four_rejections(gpu, name, cid):
    s = scheme(gpu, name)
    p, G = s.order, s.E.G1()
    for m in (1, T + 1):
        t, z = table(p, m, seed=1), point(p, m, seed=1)
        c = s.commit(t)
        proof, v = s.open(t, z)
        assert s.verify(c, proof, z, v)
        assert not s.verify(c, proof[:-1], z, v) and not s.verify(c, proof + [G], z, v)      # a proof of the wrong length
        assert not s.verify(c, proof, z, (v + 1) % p)                                          # a wrong evaluation
        for k in {0, m - 1}:                                                                   # a tampered Q_k
            bad = list(proof)
            bad[k] = bad[k] + G
            assert not s.verify(c, bad, z, v)
        assert not s.verify(c, proof, [(z[0] + 1) % p] + z[1:], v)                             # a different point
        assert not s.verify(c, proof, z[::-1], v) or z == z[::-1]
        assert not s.verify(c + G, proof, z, v)


@per_curve
def test_batch_open_and_verify(gpu, name, cid):
    s = scheme(gpu, name)
    p = s.order
    m = T + 1
    z = point(p, m, seed=2)
    tables = [table(p, m, seed=10 + i) for i in range(5)]
    for count in (1, 5):
        polys = tables[:count]
        cs = [s.commit(t) for t in polys]
        proof, vs = s.batch_open(polys, z)
        assert vs == [M.evaluate(t, z, p) for t in polys] and len(proof) == m
        rho = s._challenge(None, cs, z, vs)
        want_q, _ = M.open_(M.combine(polys, rho, p), z, trapdoor(p), p)
        assert proof == [s.E.G1() * q for q in want_q]
        assert s.batch_open(polys, z, commitments=cs) == (proof, vs)
        assert s.batch_verify(cs, proof, z, vs)
        assert not s.batch_verify(cs, proof, z, [(vs[0] + 1) % p] + vs[1:])
        if count > 1:
            assert not s.batch_verify(cs[1:] + cs[:1], proof, z, vs)
            assert not s.batch_verify(cs[:-1], proof, z, vs[:-1])
    # a caller's transcript: prover and verifier stay in step, and the label separates it from the default one
    ta, tb = FiatShamirTranscript(b"outer protocol", p), FiatShamirTranscript(b"outer protocol", p)
    ta.append(7)
    tb.append(7)
    proof2, vs2 = s.batch_open(tables, z, transcript=ta)
    assert vs2 == vs and proof2 != proof
    assert s.batch_verify(cs, proof2, z, vs2, transcript=tb)
    assert ta.get_challenge_scalar() == tb.get_challenge_scalar()
    assert not s.batch_verify(cs, proof2, z, vs2)
    # no variable at all: the transcript takes no point
    proof0, vs0 = s.batch_open([[3], [p - 1]], [])
    assert proof0 == [] and vs0 == [3, p - 1] and s.batch_verify([s.commit([3]), s.commit([p - 1])], proof0, [], vs0)


@per_curve
def test_nothing_is_carried_between_runs(gpu, name, cid):
    """an opening after commits and openings of other sizes on the same scheme gives the bytes of a fresh scheme's"""
    s = scheme(gpu, name)
    p = s.order
    m = T + 1
    t, z = table(p, m, seed=3), point(p, m, seed=3)
    s.commit(table(p, NV, seed=4))
    s.open(table(p, 4, seed=4), point(p, 4))
    s.commit([p - 1] * (1 << m))
    proof, v = s.open(t, z)
    fresh = MultilinearKZG(NV, name)
    fresh.setup(tau=trapdoor(p))
    want_proof, want_v = fresh.open(t, z)
    assert v == want_v and b"".join(bytes(q.to_bytes()) for q in proof) == b"".join(bytes(q.to_bytes()) for q in want_proof)
    assert fresh.G2_tau == s.G2_tau and len(s.G2_tau) == NV
    # release() frees every level; the scheme is unusable until the next setup
    fresh.release()
    assert not fresh.is_setup and fresh.G2_tau is None
    with pytest.raises(RuntimeError):
        fresh.commit(t)
    with pytest.raises(RuntimeError):
        fresh.open(t, z)
    fresh.setup(tau=trapdoor(p))
    assert fresh.open(t, z) == (want_proof, want_v)
    fresh.release()


@per_curve
def test_setup_with_a_drawn_trapdoor_and_a_smaller_scheme(gpu, name, cid):
    s = MultilinearKZG(3, name)
    with pytest.raises(ValueError):
        s.setup(tau=[1, 2])
    s.setup()
    p = s.order
    t, z = table(p, 3, seed=6), point(p, 3, seed=6)
    proof, v = s.open(t, z)
    assert v == M.evaluate(t, z, p) and s.verify(s.commit(t), proof, z, v) and not s.verify(s.commit(t), proof, z, v + 1)
    other = MultilinearKZG(3, name)
    other.setup()
    assert not other.verify(s.commit(t), proof, z, v)       # another trapdoor
    zero = MultilinearKZG(0, name)
    zero.setup()
    assert zero.G2_tau == [] and zero.commit([9]) == zero.E.G1() * 9 and zero.open([9], []) == ([], 9)
    assert zero.verify(zero.commit([9]), [], [], 9)
    for x in (s, other, zero):
        x.release()
