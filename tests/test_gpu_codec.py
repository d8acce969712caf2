"""GPU parity: batched point (de)compression (zk_points_compress / zk_points_decompress) against the CPU oracle's
per-point encodings (oracle/pyref.py compress / decompress, pinned by the reference's golden points), all four groups,
with the error behaviour of the reference's from_hex (ark deserialize_compressed) on damaged input."""

import functools
import random

import numpy as np
import pytest

import codec_model as M
from helpers import CURVES, oracle_bases
from oracle import corc, pyref
from zksnake_amd import _native as N
from zksnake_amd._algebra import PointArray

pytestmark = pytest.mark.gpu

# the tests against the integer model (tests/codec_model.py), below the oracle ones
SIZES = (1, 127, 128, 129, 300)     # one lane; one below, exactly and one above a 128-lane workgroup; three workgroups
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
GROUPS = [(name, cid, grp) for name, cid in CURVES for grp in (1, 2)]
group_id = lambda v: v if isinstance(v, str) else None  # noqa: E731


def _compress(lib, cid, grp, limbs):
    nb = lib.zk_point_bytes(cid, grp)
    out = np.zeros(limbs.shape[0] * nb, dtype=np.uint8)
    bad = N._u64(0)
    N.check(lib.zk_points_compress(cid, grp, limbs.shape[0], N.u64p(limbs), N.u8p(out), bad))
    return out


def _decompress(lib, cid, grp, raw, n):
    out = np.zeros((n, N.point_limbs(cid, grp)), dtype=np.uint64)
    bad = N._u64(0)
    rc = lib.zk_points_decompress(cid, grp, n, N.u8p(raw), N.u64p(out), bad)
    return rc, bad.value, out


@pytest.mark.parametrize("name,cid", CURVES)
@pytest.mark.parametrize("grp", [1, 2])
def test_batch_codec_matches_oracle(gpu, name, cid, grp):
    cv = pyref.curve_by_name(name)
    n = 300
    _, bases = oracle_bases(cid, grp, n, 7 + grp)
    bases[5] = 0      # the point at infinity
    bases[n - 1] = 0
    pts = corc.limbs_to_points(bases, cid, grp)
    want = b"".join(pyref.compress(cv, grp, p) for p in pts)
    got = _compress(gpu, cid, grp, bases)
    assert got.tobytes() == want
    rc, _, back = _decompress(gpu, cid, grp, got, n)
    assert rc == 0 and (back == bases).all()
    # the per-point host codec agrees
    nb = gpu.zk_point_bytes(cid, grp)
    one = np.zeros(N.point_limbs(cid, grp), dtype=np.uint64)
    for i in (0, 5, 17):
        N.check(gpu.zk_point_decompress(cid, grp, N.u8p(got[i * nb:(i + 1) * nb].copy()), N.u64p(one)))
        assert (one == bases[i]).all()


@pytest.mark.parametrize("name,cid", CURVES)
@pytest.mark.parametrize("grp", [1, 2])
def test_batch_decompress_rejects_like_from_hex(gpu, name, cid, grp):
    """first offending point decides; same messages as the per-point path"""
    n = 200
    _, bases = oracle_bases(cid, grp, n, 11)
    good = _compress(gpu, cid, grp, bases)
    nb = gpu.zk_point_bytes(cid, grp)
    one = np.zeros(N.point_limbs(cid, grp), dtype=np.uint64)

    def damaged(index, mutate):
        raw = good.copy()
        mutate(raw[index * nb:(index + 1) * nb])
        return raw

    def all_ones(p):
        p[:] = 0xFF if cid == N.CURVE_BN254 else p
        if cid != N.CURVE_BN254:
            p[0] &= 0x7F  # BLS: clear the "compressed" bit

    def x_out_of_range(p):
        if cid == N.CURVE_BN254:
            p[:] = 0xFF
            p[nb - 1] = 0x3F
            if grp == 2:
                p[nb // 2 - 1] = 0x3F
        else:
            p[:] = 0xFF
            p[0] = 0x9F

    def infinity_with_x(p):
        if cid == N.CURVE_BN254:
            p[nb - 1] |= 0x40
            p[nb - 1] &= 0x7F
        else:
            p[0] = (p[0] | 0x40) & 0xDF

    for index, mutate in ((3, all_ones), (150, x_out_of_range), (199, infinity_with_x)):
        raw = damaged(index, mutate)
        rc, bad, _ = _decompress(gpu, cid, grp, raw, n)
        assert rc == N.ZK_ERR_POINT and bad == index
        msg = gpu.zk_last_error()
        assert gpu.zk_point_decompress(cid, grp, N.u8p(raw[index * nb:(index + 1) * nb].copy()), N.u64p(one)) == N.ZK_ERR_POINT
        assert gpu.zk_last_error() == msg
    # two damaged points: the lower index is reported
    raw = damaged(150, x_out_of_range)
    all_ones(raw[20 * nb:21 * nb])
    rc, bad, _ = _decompress(gpu, cid, grp, raw, n)
    assert rc == N.ZK_ERR_POINT and bad == 20


@pytest.mark.parametrize("name,cid", CURVES)
@pytest.mark.parametrize("grp", [1, 2])
def test_batch_decompress_checks_curve_and_subgroup(gpu, name, cid, grp):
    """an x with no y on the curve, and (where the cofactor is not 1) a curve point outside the r-torsion"""
    n = 100
    _, bases = oracle_bases(cid, grp, n, 13)
    good = _compress(gpu, cid, grp, bases)
    nb = gpu.zk_point_bytes(cid, grp)
    one = np.zeros(N.point_limbs(cid, grp), dtype=np.uint64)
    # walk x = 1, 2, ... (c1 = 0 in G2): collect one x off the curve and one on the curve but outside the subgroup,
    # as classified by the per-point host codec
    off_curve = not_subgroup = None
    fb = nb // grp
    x = 1
    while off_curve is None or (not_subgroup is None and not (cid == N.CURVE_BN254 and grp == 1)):
        if cid == N.CURVE_BN254:
            enc = x.to_bytes(fb, "little") + bytes(nb - fb)
        else:
            enc = bytearray(bytes(nb - fb) + x.to_bytes(fb, "big"))
            enc[0] |= 0x80
        enc = np.frombuffer(bytes(enc), dtype=np.uint8).copy()
        rc = gpu.zk_point_decompress(cid, grp, N.u8p(enc), N.u64p(one))
        msg = gpu.zk_last_error().decode()
        if rc and "not on the curve" in msg and off_curve is None:
            off_curve = (enc, msg)
        if rc and "subgroup" in msg and not_subgroup is None:
            not_subgroup = (enc, msg)
        x += 1
        assert x < 200
    for case in (off_curve, not_subgroup):
        if case is None:
            continue
        raw = good.copy()
        raw[42 * nb:43 * nb] = case[0]
        rc, bad, _ = _decompress(gpu, cid, grp, raw, n)
        assert rc == N.ZK_ERR_POINT and bad == 42 and gpu.zk_last_error().decode() == case[1]


def test_batch_compress_rejects_off_curve_point(gpu):
    _, bases = oracle_bases(N.CURVE_BN254, 1, 100, 17)
    bases[31, 0] ^= 1
    out = np.zeros(100 * 32, dtype=np.uint8)
    bad = N._u64(0)
    assert gpu.zk_points_compress(N.CURVE_BN254, 1, 100, N.u64p(bases), N.u8p(out), bad) == N.ZK_ERR_POINT
    assert bad.value == 31 and b"not on the curve" in gpu.zk_last_error()


@pytest.mark.parametrize("name,cid", CURVES)
def test_key_sized_round_trip(gpu, name, cid):
    """2^16 distinct points (k * G for random k through the fixed-base batch multiplication) through PointArray"""
    cv = pyref.curve_by_name(name)
    n = 1 << 16
    rng = np.random.default_rng(5)
    sc = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= (1 << 60) - 1
    for grp in (1, 2):
        gen = np.zeros(N.point_limbs(cid, grp), dtype=np.uint64)
        N.check(gpu.zk_point_generator(cid, grp, N.u64p(gen)))
        pts = np.zeros((n, N.point_limbs(cid, grp)), dtype=np.uint64)
        N.check(gpu.zk_batch_mul(cid, grp, n, N.u64p(sc), N.u64p(gen), 1, N.u64p(pts)))
        arr = PointArray(cid, grp, pts)
        raw = arr.to_bytes()
        assert len(raw) == n * gpu.zk_point_bytes(cid, grp)
        back = PointArray.from_compressed(cid, grp, raw, n)
        assert (back.limbs == pts).all()
        # spot-check against the oracle's encoding
        for i in (0, 1, n - 1):
            p = corc.limbs_to_points(pts[i:i + 1], cid, grp)[0]
            nb = gpu.zk_point_bytes(cid, grp)
            assert raw[i * nb:(i + 1) * nb] == pyref.compress(cv, grp, p)


# ---- every decode branch, validation edge and batch position against the integer model (tests/codec_model.py) ---------------
def _positions(n, rnd):
    """first and last lane of the first workgroup, first lane of the second, the last point, a seeded interior point"""
    return sorted({at for at in (0, 127, 128, n - 1, rnd.randrange(n)) if at < n})


@functools.lru_cache(maxsize=None)
def _fillers(cid, grp):
    """300 valid points k G from the C++ oracle and their encodings by oracle/pyref.py; shared, so callers copy"""
    cv = pyref.curve_by_name(CURVES[cid][0])
    _, bases = oracle_bases(cid, grp, max(SIZES), 23 + grp)
    enc = b"".join(pyref.compress(cv, grp, p) for p in corc.limbs_to_points(bases, cid, grp))
    return bases, np.frombuffer(enc, dtype=np.uint8)


def _decode_into_sentinel(lib, cid, grp, raw, n):
    out = np.full((n, N.point_limbs(cid, grp)), SENTINEL, dtype=np.uint64)
    bad = N._u64(0)
    rc = lib.zk_points_decompress(cid, grp, n, N.u8p(raw), N.u64p(out), bad)
    return rc, bad.value, out


def _encode_into_sentinel(lib, cid, grp, rows):
    out = np.full(rows.shape[0] * lib.zk_point_bytes(cid, grp), 0xA5, dtype=np.uint8)
    bad = N._u64(0)
    rc = lib.zk_points_compress(cid, grp, rows.shape[0], N.u64p(rows), N.u8p(out), bad)
    return rc, bad.value, out


def _put(raw, nb, at, data):
    raw[at * nb:(at + 1) * nb] = np.frombuffer(data, dtype=np.uint8)


@pytest.mark.parametrize("name,cid,grp", GROUPS, ids=group_id)
def test_batch_decode_accepts_every_valid_model_case(gpu, name, cid, grp):
    """each valid case of codec_model.cases at each position of each batch size among valid points (a batch carries one case per
    position, the cases rotating through the positions from batch to batch): the model's point limb for limb, every other row
    the point it encodes"""
    cv = pyref.curve_by_name(name)
    nb = gpu.zk_point_bytes(cid, grp)
    bases, enc = _fillers(cid, grp)
    valid = [c for c in M.cases(cv, grp, 1) if c[2] == "CODEC_OK"]
    rows = corc.points_to_limbs([c[3] for c in valid], cid, grp)
    rnd = random.Random(31)
    for n in SIZES:
        pos = _positions(n, rnd)
        for b in range(len(valid)):
            raw, want = enc[:n * nb].copy(), bases[:n].copy()
            for j, at in enumerate(pos):
                k = (b + j) % len(valid)
                _put(raw, nb, at, valid[k][1])
                want[at] = rows[k]
            rc, _, out = _decode_into_sentinel(gpu, cid, grp, raw, n)
            assert rc == 0, (n, b, gpu.zk_last_error())
            assert (out == want).all(), (n, b, np.flatnonzero((out != want).any(axis=1)))


@pytest.mark.parametrize("name,cid,grp", GROUPS, ids=group_id)
def test_batch_decode_refuses_every_invalid_model_case(gpu, name, cid, grp):
    """each refused case at each position of each batch size: its index, the message of the model's status (the strings of
    codec.hip.h as codec_model restates them) and an untouched output buffer"""
    cv = pyref.curve_by_name(name)
    nb = gpu.zk_point_bytes(cid, grp)
    _, enc = _fillers(cid, grp)
    rnd = random.Random(32)
    invalid = [c for c in M.cases(cv, grp, 1) if c[2] != "CODEC_OK"]
    assert invalid
    for n in SIZES:
        for at in _positions(n, rnd):
            for label, data, status, _ in invalid:
                raw = enc[:n * nb].copy()
                _put(raw, nb, at, data)
                rc, bad, out = _decode_into_sentinel(gpu, cid, grp, raw, n)
                assert rc == N.ZK_ERR_POINT and bad == at and gpu.zk_last_error() == M.MESSAGE[status], \
                    (label, data.hex(), n, at, rc, bad, gpu.zk_last_error())
                assert (out == SENTINEL).all(), (label, n, at)


@pytest.mark.parametrize("name,cid,grp", GROUPS, ids=group_id)
def test_batch_decode_reports_the_lowest_index_not_the_lowest_code(gpu, name, cid, grp):
    """two and three refused points with different statuses, the lower index carrying the numerically larger status code:
    across workgroups, on either side of a workgroup boundary and inside one workgroup"""
    cv = pyref.curve_by_name(name)
    nb = gpu.zk_point_bytes(cid, grp)
    _, enc = _fillers(cid, grp)
    by_status = {}
    for c in M.cases(cv, grp, 1):
        if c[2] != "CODEC_OK":
            by_status.setdefault(c[2], c)
    picks = sorted(by_status.values(), key=lambda c: -M.CODE[c[2]])[:3]
    assert len(picks) == 3 and M.CODE[picks[0][2]] > M.CODE[picks[1][2]] > M.CODE[picks[2][2]]
    n = 300
    for spots in ((10, 140, 270), (127, 128), (200, 299), (3, 100), (0, 127), (128, 129, 130)):
        raw = enc[:n * nb].copy()
        for at, c in zip(spots, picks):
            _put(raw, nb, at, c[1])
        rc, bad, out = _decode_into_sentinel(gpu, cid, grp, raw, n)
        assert rc == N.ZK_ERR_POINT and bad == spots[0] and gpu.zk_last_error() == M.MESSAGE[picks[0][2]], (spots, bad, gpu.zk_last_error())
        assert (out == SENTINEL).all()


@pytest.mark.parametrize("name,cid,grp", GROUPS, ids=group_id)
def test_batch_encode_matches_the_model(gpu, name, cid, grp):
    """the model's valid points and infinity at each position of each batch size give the model's bytes; -P differs from P in
    the sign bit alone"""
    cv = pyref.curve_by_name(name)
    g = pyref.Group(cv, grp)
    nb = gpu.zk_point_bytes(cid, grp)
    bases, enc = _fillers(cid, grp)
    pts = [c[3] for c in M.cases(cv, grp, 1) if c[2] == "CODEC_OK"]
    assert None in pts
    rows = corc.points_to_limbs(pts, cid, grp)
    rnd = random.Random(33)
    for n in SIZES:
        pos = _positions(n, rnd)
        for b in range(len(pts)):
            batch, want = bases[:n].copy(), enc[:n * nb].copy()
            for j, at in enumerate(pos):
                k = (b + j) % len(pts)
                batch[at] = rows[k]
                _put(want, nb, at, M.encode_point(cv, grp, pts[k]))
            rc, _, out = _encode_into_sentinel(gpu, cid, grp, batch)
            assert rc == 0 and (out == want).all(), (n, b, gpu.zk_last_error())
    finite = [p for p in pts if p is not None]
    rc, _, pos_bytes = _encode_into_sentinel(gpu, cid, grp, corc.points_to_limbs(finite, cid, grp))
    rc2, _, neg_bytes = _encode_into_sentinel(gpu, cid, grp, corc.points_to_limbs([g.neg(p) for p in finite], cid, grp))
    assert rc == 0 and rc2 == 0
    diff = (pos_bytes ^ neg_bytes).reshape(len(finite), nb)
    want = np.zeros_like(diff)
    if cid == N.CURVE_BN254:
        want[:, nb - 1] = 0x80
    else:
        want[:, 0] = 0x20
    assert (diff == want).all()


@pytest.mark.parametrize("name,cid,grp", GROUPS, ids=group_id)
def test_batch_encode_refuses_off_curve_and_unreduced_rows(gpu, name, cid, grp):
    """an off-curve row, and a row with one coordinate raised by p (x + p or y + p, each component alone; 2 p fits the limbs),
    at the first and last lane of a workgroup and at the last point: the index, the message, an untouched output buffer.  The
    x bytes are the caller's words, so x + p accepted would be written with its top bits on the flag bits; the lowest index wins
    here too, against the status order"""
    cv = pyref.curve_by_name(name)
    bases, _ = _fillers(cid, grp)
    fw = N.point_limbs(cid, grp) // (2 * grp)     # 64-bit limbs per base-field element
    rnd = random.Random(34)

    def refused(batch, at, status):
        rc, bad, out = _encode_into_sentinel(gpu, cid, grp, batch)
        assert rc == N.ZK_ERR_POINT and bad == at and gpu.zk_last_error() == M.MESSAGE[status], (batch.shape[0], at, rc, bad, gpu.zk_last_error())
        assert (out == 0xA5).all()

    def raised(row, k):
        row = row.copy()
        v = N.limbs_to_ints(row[k * fw:(k + 1) * fw].reshape(1, fw))[0] + cv.p
        row[k * fw:(k + 1) * fw] = N.ints_to_limbs([v], fw)[0]
        return row

    for n in SIZES:
        for at in _positions(n, rnd):
            batch = bases[:n].copy()
            batch[at, 0] ^= 1
            refused(batch, at, "CODEC_NOT_ON_CURVE")
            for k in range(2 * grp):
                batch = bases[:n].copy()
                batch[at] = raised(batch[at], k)
                refused(batch, at, "CODEC_COORD_RANGE")
    batch = bases.copy()
    batch[5] = raised(batch[5], 0)      # status 8 at the lower index, status 1 in another workgroup
    batch[200, 0] ^= 1
    refused(batch, 5, "CODEC_COORD_RANGE")
