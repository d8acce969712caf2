"""CPU: the checked PointArray constructor, the owner of a generator set and the canonicalising upload, as far as they need no
GPU: every point array stays below PointArray.BATCH_CODEC_MIN (host codec) and no MSM plan is created."""

import types

import numpy as np
import pytest

from zksnake_amd._algebra import PointArray
from zksnake_amd.ecc import EllipticCurve
from zksnake_amd.frvec import DevVec, FrOps
from zksnake_amd.subprotocol._generators import GeneratorSet
from zksnake_amd.transcript import FiatShamirTranscript

BN, BLS = EllipticCurve("BN254"), EllipticCurve("BLS12_381")
POINTS = [BN.G1() * k for k in (3, 5, 7, 11)]


# ---- PointArray.from_points -------------------------------------------------------------------------------------------------------
def test_a_list_and_an_array_of_the_same_points_give_equal_limbs():
    from_list = PointArray.from_points(0, 1, POINTS, count=4)
    from_iter = PointArray.from_points(0, 1, iter(POINTS))
    assert (from_list.limbs == np.stack([p._limbs for p in POINTS])).all() and (from_iter.limbs == from_list.limbs).all()
    assert PointArray.from_points(0, 1, from_list, count=4) is from_list
    assert list(from_list) == POINTS
    g2 = PointArray.from_points(0, 2, [BN.G2() * 2, BN.G2()])
    assert g2.group == 2 and g2[0] == BN.G2() * 2 and len(PointArray.from_points(0, 1, [])) == 0


def test_foreign_points_are_a_type_error_and_a_wrong_length_a_value_error():
    arr = PointArray.from_points(0, 1, POINTS)
    foreign = [[BN.G2()], [BLS.G1()], POINTS[:1] + [BLS.G1()], [3], PointArray.from_points(0, 2, [BN.G2()]),
               PointArray.from_points(1, 1, [BLS.G1()])]
    for points in foreign:
        with pytest.raises(TypeError, match="powers of tau"):
            PointArray.from_points(0, 1, points, what="powers of tau")
    with pytest.raises(TypeError):
        PointArray.from_points(1, 1, arr)
    with pytest.raises(TypeError):
        PointArray.from_points(0, 2, arr)
    for points in (POINTS, arr):
        for count in (3, 5):
            with pytest.raises(ValueError, match=f"{count} generators expected, got 4"):
                PointArray.from_points(0, 1, points, count=count, what="generators")
    with pytest.raises(TypeError):      # the type is looked at before the length
        PointArray.from_points(0, 1, [BN.G2()], count=2)


# ---- GeneratorSet -----------------------------------------------------------------------------------------------------------------
def _fresh_challenge(label, field, points):
    transcript = FiatShamirTranscript(label, field)
    for p in points:
        transcript.append(p)
    return transcript.get_challenge()


@pytest.mark.parametrize("sizes", [(4, 4), (4, None)], ids=["G-H", "G-h"])
def test_owner_of_four_generators(sizes):
    other = [BN.G1() * k for k in (13, 17, 19, 23)]
    second = other if sizes[1] else other[0]
    flat = POINTS + (other if sizes[1] else other[:1])
    gens = GeneratorSet(BN, sizes)
    gens.set(0, POINTS)
    gens.set(1, second)
    assert isinstance(gens.parts[0], PointArray) and list(gens.parts[0]) == POINTS
    assert gens.parts[1] is second if sizes[1] is None else list(gens.parts[1]) == other

    assert b"".join(gens.bytes()) == b"".join(bytes(p.to_bytes()) for p in flat)
    assert gens.bytes() is gens.bytes()
    assert list(gens.bases()) == flat and gens.bases() is gens.bases()

    label, field = b"label", BN.order
    want = _fresh_challenge(label, field, flat)
    assert gens._hasher is None
    assert gens.transcript(None, label, field).get_challenge() == want
    assert gens._hasher is not None
    assert gens.transcript(None, label, field).get_challenge() == want        # from the kept hasher
    given = FiatShamirTranscript(b"another", field)
    given.append(5)
    assert gens.transcript(given, label, field) is given
    assert given.get_challenge() == _fresh_challenge(b"another", field, [5] + flat)

    for i, value in ((0, list(reversed(POINTS))), (1, second)):
        gens.bytes(), gens.bases(), gens.transcript(None, label, field)
        gens.set(i, value)
        assert gens._bytes is None and gens._hasher is None and gens._bases is None
    flat = list(reversed(POINTS)) + flat[4:]
    assert gens.transcript(None, label, field).get_challenge() == _fresh_challenge(label, field, flat) != want

    gens.bases()
    gens.release()
    gens.release()
    assert gens._bases is None and gens._bytes is not None and gens._hasher is not None      # only the plans go
    assert list(gens.bases()) == flat


def test_owner_validates_what_it_is_given():
    gens = GeneratorSet(BN, (4, None))
    with pytest.raises(ValueError, match="4 generators expected, got 3"):
        gens.set(0, POINTS[:3])
    for bad in ([BLS.G1()] * 4, [BN.G2()] * 4):
        with pytest.raises(TypeError):
            gens.set(0, bad)
    for bad in (BLS.G1(), BN.G2(), POINTS, None):
        with pytest.raises(TypeError):
            gens.set(1, bad)
    assert gens.parts == [None, None]


def test_the_protocols_hold_one_owner_each():
    from zksnake_amd.commitment.polynomial import IPA
    from zksnake_amd.subprotocol import InnerProductArgument, RangeProof
    arg = InnerProductArgument(4, "BN254")
    assert arg.G is arg._gens.parts[0] and arg.H is arg._gens.parts[1] and len(arg.G) == len(arg.H) == 4
    before = arg._transcript(None).get_challenge()
    assert arg._transcript(None).get_challenge() == before == _fresh_challenge((4).to_bytes(32, "big"), BN.order, list(arg.G) + list(arg.H))
    arg.H = POINTS
    assert arg._gens._hasher is None and list(arg.H) == POINTS and arg._transcript(None).get_challenge() != before
    with pytest.raises(ValueError):
        arg.G = POINTS[:2]
    rp = RangeProof(4, "BN254")
    assert rp.G is rp._ipa._gens.parts[0]

    pcs = IPA(4, "BN254")
    assert not pcs.is_setup and pcs.G is None and pcs.H is None
    pcs.G = POINTS
    assert not pcs.is_setup
    pcs.H = BN.G1()
    assert pcs.is_setup and pcs.H == BN.G1()
    assert pcs._transcript(None).get_challenge() == _fresh_challenge(b"IPA-PCS", BN.order, POINTS + [BN.G1()])
    with pytest.raises(TypeError):
        pcs.H = BN.G2()
    with pytest.raises(TypeError):
        pcs.G = [BLS.G1()] * 4
    pcs.release()
    pcs.release()


# ---- FrOps.d_load -----------------------------------------------------------------------------------------------------------------
def _empty_devvec():
    vec = DevVec.__new__(DevVec)      # no allocation: nothing may read it
    vec.n, vec.buf = 0, None
    return vec


def test_upload_refuses_more_than_the_limit_and_skips_the_device_for_nothing():
    ops = FrOps(BN.order)
    untouchable = types.SimpleNamespace(n=8)      # no ptr(), no upload(): any use is an AttributeError
    long_vec = _empty_devvec()
    long_vec.n = 5
    for values in ([1, 2, 3, 4, 5], np.ones((5, 4), dtype=np.uint64), long_vec):
        with pytest.raises(ValueError, match="at most 4 elements"):
            ops.d_load(untouchable, 0, values, 4)
    for values in ([], np.zeros((0, 4), dtype=np.uint64), _empty_devvec()):
        assert ops.d_load(untouchable, 8, values, 4) == 0
        assert ops.d_load(untouchable, 0, values, 0) == 0
