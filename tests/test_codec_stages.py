"""The pieces of the point codec called directly: tests/native/codec_stages.hip runs fp_pow, fp_sqrt, fp2_sqrt, coord_is_larger,
canonical_lt_mod, point_decode and point_encode (csrc/codec.hip.h, csrc/field.hip.h) on records built here.  The host build (g++)
runs in the CPU suite; the device build (the library's own hipcc pipeline, gfx950; ZKMI_CODEC_STAGE_LIB names an already built one)
must give the host's output word for word (`-m gpu`).  Every record is checked against plain integers:

  fp_pow            pow(a, e, p): bases 0, 1, 2, p - 1 and seeded ones against the exponents 0, 1, 2, p - 1, (p + 1) / 4, all-ones
                    words, a single top bit, and one- and two-word exponents with set words above them that must not be read
  fp_sqrt           0, 1, 4, seeded s^2: found, and the root squares to the input; p - 1 and p - s^2 (p = 3 mod 4): not found
  fp2_sqrt          zero; real arguments, whose root is (s, 0) for a square of Fp and (0, s) with s^2 = -a otherwise; (0, b); squares
                    of seeded elements, at least 8 for each outcome of the first candidate; non-square norms: not found
  coord_is_larger   1, (p - 1) / 2, (p + 1) / 2, p - 1 give false, false, true, true; in Fp2 c1 decides unless it is zero
  canonical_lt_mod  0, p - 1, p, p + 1, all-ones
  point_decode      every case of codec_model.cases: status and, when accepted, the model's point; a refusal writes nothing
  point_encode      the model's points give the model's bytes, -P differs in the sign bit alone, an off-curve row and a coordinate
                    of p or above are refused and write nothing (point_encode is handed the record's own fill to write over)
"""

import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import codec_model as M
from helpers import build_device_harness
from oracle import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "codec_stages.hip")
POW, SQRT, FP2_SQRT, LARGER, LARGER_FP2, LT_MOD, DECODE, ENCODE = range(8)
IN_WORDS = OUT_WORDS = 128
SENTINEL = 0xA5A5A5A5
CURVES = [pyref.BN254, pyref.BLS12_381]            # the field selector of cs_run is the curve's index here
GROUPS = [(cv, grp) for cv in CURVES for grp in (1, 2)]   # and the group selector the index here
cid = lambda cv: cv.name  # noqa: E731
gid = lambda cg: f"{cg[0].name}-G{cg[1]}"  # noqa: E731


def words(v, nwords):
    assert 0 <= v < 1 << (32 * nwords)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(nwords)]


def value(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def W(cv):
    return cv.fp_bytes // 4


class Harness:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.cs_run.restype = ctypes.c_int
        self.lib.cs_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]

    def run(self, op, sel, recs):
        """recs: one list of words per record -> (count, OUT_WORDS) uint32, each record prefilled with SENTINEL"""
        arr = np.zeros((len(recs), IN_WORDS), dtype=np.uint32)
        for i, r in enumerate(recs):
            arr[i, :len(r)] = r
        out = np.full((len(recs), OUT_WORDS), SENTINEL, dtype=np.uint32)
        rc = self.lib.cs_run(op, sel, len(recs), arr.ctypes.data, out.ctypes.data)
        assert rc == 0, f"cs_run(op {op}, sel {sel}) returned {rc}"
        return out


# ---- the checks: each runs its records through a harness, compares with integers and returns the raw output -----------------
def check_pow(h, cv):
    p, w = cv.p, W(cv)
    rnd = random.Random(41)
    top = (1 << (32 * w)) - 1
    bases = [0, 1, p - 1, 2] + [rnd.randrange(p) for _ in range(4)]
    exps = [(e, w) for e in (0, 1, 2, p - 1, (p + 1) // 4, top, 1 << (32 * w - 1), rnd.randrange(top))]
    exps += [(top, 1), (top, 2), ((1 << 32) | 5, 1), (rnd.randrange(top), 2), (top, 0)]
    recs = [(a, e, nw) for a in bases for e, nw in exps]
    out = h.run(POW, CURVES.index(cv), [words(a, w) + words(e, w) + [nw] for a, e, nw in recs])
    for (a, e, nw), o in zip(recs, out):
        assert value(o[:w]) == pow(a, e & ((1 << (32 * nw)) - 1), p), (hex(a), hex(e), nw)
    return out


def check_sqrt(h, cv):
    p, w = cv.p, W(cv)
    rnd = random.Random(42)
    ss = [rnd.randrange(1, p) for _ in range(12)]
    recs = [0, 1, 4, p - 1] + [s * s % p for s in ss] + [p - s * s % p for s in ss]
    out = h.run(SQRT, CURVES.index(cv), [words(a, w) for a in recs])
    for a, o in zip(recs, out):
        root = value(o[1:1 + w])
        assert int(o[0]) == int(M.fp_is_square(a, p)), hex(a)
        assert root < p and (root * root % p == a if o[0] else root == 0), hex(a)
    assert [int(o[0]) for o in out[:4]] == [1, 1, 1, 0]
    return out


def fp2_sqrt_inputs(cv):
    p = cv.p
    rnd = random.Random(43)
    res = [rnd.randrange(1, p) ** 2 % p for _ in range(4)]
    recs = [(0, 0)] + [(a, 0) for a in res] + [(p - a, 0) for a in res] + [(0, a) for a in res] + [(0, p - a) for a in res]
    recs += [(1, 0), (p - 1, 0), (0, 1), (0, p - 1)]
    squares = [pyref.f2_mul(e, e, p) for e in ((rnd.randrange(p), rnd.randrange(1, p)) for _ in range(40))]
    squares = [a for a in squares if a[1]]
    first = [M.first_attempt_is_square(a, p) for a in squares]
    assert first.count(True) >= M.SQRT_MIN and first.count(False) >= M.SQRT_MIN
    non = []
    while len(non) < 12:
        a = (rnd.randrange(p), rnd.randrange(1, p))
        if not M.is_square(a, p):
            non.append(a)
    return recs + squares + non, len(res)


def check_fp2_sqrt(h, cv):
    p, w = cv.p, W(cv)
    recs, k = fp2_sqrt_inputs(cv)
    out = h.run(FP2_SQRT, CURVES.index(cv), [words(a[0], w) + words(a[1], w) for a in recs])
    for a, o in zip(recs, out):
        root = (value(o[1:1 + w]), value(o[1 + w:1 + 2 * w]))
        assert int(o[0]) == int(M.is_square(a, p)), a
        assert root[0] < p and root[1] < p and (pyref.f2_mul(root, root, p) == a if o[0] else root == (0, 0)), (a, root)
    roots = [(value(o[1:1 + w]), value(o[1 + w:1 + 2 * w])) for o in out]
    assert all(o[0] == 1 for o in out[:1 + 4 * k + 4]), "every element of Fp is a square in Fp2"
    assert all(r[1] == 0 and r[0] for r in roots[1:1 + k]), "a square of Fp has a real root"
    assert all(r[0] == 0 and r[1] for r in roots[1 + k:1 + 2 * k]), "a non-square of Fp has a purely imaginary root"
    return out


def larger_inputs(cv):
    p = cv.p
    rnd = random.Random(44)
    edge = [(1, False), ((p - 1) // 2, False), ((p + 1) // 2, True), (p - 1, True)]
    fp2 = [((v, 0), e) for v, e in edge]
    fp2 += [((c0, v), e) for v, e in edge for c0 in (0, 1, (p - 1) // 2, (p + 1) // 2, p - 1, rnd.randrange(p))]
    fp2 += [((p - 1, 1), False), ((1, p - 1), True), ((0, 0), False)]
    return edge + [(0, False)], fp2


def check_larger(h, cv):
    w = W(cv)
    fp, fp2 = larger_inputs(cv)
    out1 = h.run(LARGER, CURVES.index(cv), [words(v, w) for v, _ in fp])
    assert [int(o[0]) for o in out1] == [int(e) for _, e in fp]
    out2 = h.run(LARGER_FP2, CURVES.index(cv), [words(v[0], w) + words(v[1], w) for v, _ in fp2])
    assert [int(o[0]) for o in out2] == [int(e) for _, e in fp2]
    assert all(M.is_larger(v, cv.p) == e for v, e in fp + fp2)
    return np.concatenate([out1, out2])


def check_lt_mod(h, cv):
    p, w = cv.p, W(cv)
    vals = [0, 1, p - 1, p, p + 1, 2 * p, (1 << M.flag_bits(cv)) - 1, (1 << (32 * w)) - 1, p ^ (1 << 32), p - (1 << (32 * (w - 1)))]
    out = h.run(LT_MOD, CURVES.index(cv), [words(v, w) for v in vals])
    assert [int(o[0]) for o in out] == [int(v < p) for v in vals]
    return out


def point_words(cv, grp, P):
    flat = [0] * (2 * grp) if P is None else ([P[0], P[1]] if grp == 1 else [*P[0], *P[1]])
    return [x for c in flat for x in words(c, W(cv))]


def check_decode(h, cv, grp):
    cs = M.cases(cv, grp, 1)
    row = 2 * grp * W(cv)
    out = h.run(DECODE, GROUPS.index((cv, grp)), [list(c[1]) for c in cs])
    for (label, data, status, pt), o in zip(cs, out):
        assert M.STATUS[int(o[0])] == status, (label, data.hex(), M.STATUS[int(o[0])], status)
        want = point_words(cv, grp, pt) if status == "CODEC_OK" else [SENTINEL] * row
        assert [int(x) for x in o[1:1 + row]] == want, (label, data.hex())
    return out


def encode_inputs(cv, grp):
    """(row words, expected status, expected bytes or None)"""
    p, w = cv.p, W(cv)
    g = pyref.Group(cv, grp)
    pts = [c[3] for c in M.cases(cv, grp, 1) if c[2] == "CODEC_OK"]
    recs = [(point_words(cv, grp, P), "CODEC_OK", M.encode_point(cv, grp, P)) for P in pts]
    P = next(P for P in pts if P is not None)
    rowP = point_words(cv, grp, P)
    for k in range(2 * grp):          # one coordinate at a time raised by p (2 p fits the words), then set to p
        v = value(rowP[k * w:(k + 1) * w])
        for nc in (v + p, p):
            recs.append((rowP[:k * w] + words(nc, w) + rowP[(k + 1) * w:], "CODEC_COORD_RANGE", None))
    recs.append((words(p, w) * (2 * grp), "CODEC_COORD_RANGE", None))
    off = list(rowP)
    off[0] ^= 1
    recs.append((off, "CODEC_NOT_ON_CURVE", None))
    recs.append((point_words(cv, grp, (P[0], g.F.zero)), "CODEC_NOT_ON_CURVE", None))
    return recs, pts


def check_encode(h, cv, grp):
    recs, pts = encode_inputs(cv, grp)
    nb = grp * cv.fp_bytes
    out = h.run(ENCODE, GROUPS.index((cv, grp)), [r[0] for r in recs])
    enc = {}
    for (row, status, data), o in zip(recs, out):
        assert M.STATUS[int(o[0])] == status, (row, M.STATUS[int(o[0])], status)
        want = [SENTINEL & ~0xFF | b for b in data] if status == "CODEC_OK" else [SENTINEL] * nb   # only the low byte is the codec's
        assert [int(x) for x in o[1:1 + nb]] == want, row
        enc[tuple(row)] = [int(x) for x in o[1:1 + nb]]
    g = pyref.Group(cv, grp)
    sign_byte, sign_bit = (nb - 1, 0x80) if M.is_bn(cv) else (0, 0x20)
    flipped = 0
    for P in pts:
        if P is None or g.neg(P) not in pts or P[1] == g.F.zero:
            continue
        a, b = ([x & 0xFF for x in enc[tuple(point_words(cv, grp, Q))]] for Q in (P, g.neg(P)))
        assert [x ^ y for x, y in zip(a, b)] == [sign_bit if i == sign_byte else 0 for i in range(nb)]
        flipped += 1
    assert flipped >= 8
    return out


FIELD_CHECKS = [check_pow, check_sqrt, check_fp2_sqrt, check_larger, check_lt_mod]
POINT_CHECKS = [check_decode, check_encode]


# ---- builds ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    dst = str(tmp_path_factory.mktemp("cs_host") / "codec_stages_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-x", "c++", "-o", dst, SRC], check=True, timeout=600)
    return Harness(dst)


@pytest.fixture(scope="module")
def device(tmp_path_factory, gpu):
    return Harness(build_device_harness(SRC, tmp_path_factory.mktemp("cs_dev"), "ZKMI_CODEC_STAGE_LIB"))


# ---- tests ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check", FIELD_CHECKS, ids=lambda c: c.__name__[6:])
@pytest.mark.parametrize("cv", CURVES, ids=cid)
def test_host_field_pieces(host, cv, check):
    check(host, cv)


@pytest.mark.parametrize("check", POINT_CHECKS, ids=lambda c: c.__name__[6:])
@pytest.mark.parametrize("cg", GROUPS, ids=gid)
def test_host_point_codec(host, cg, check):
    check(host, *cg)


@pytest.mark.gpu
@pytest.mark.parametrize("cv", CURVES, ids=cid)
def test_device_field_pieces(host, device, cv):
    for check in FIELD_CHECKS:
        assert (check(device, cv) == check(host, cv)).all(), check.__name__


@pytest.mark.gpu
@pytest.mark.parametrize("cg", GROUPS, ids=gid)
def test_device_point_codec(host, device, cg):
    for check in POINT_CHECKS:
        assert (check(device, *cg) == check(host, *cg)).all(), check.__name__
