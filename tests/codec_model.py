"""Integer model of the compressed point codec (csrc/codec.hip.h), written from the definitions and not from the kernel's method.

classify(cv, group, data) reads one encoding and returns (status, point): status is a CodecStatus name, point is the affine point in
oracle.pyref form ((x, y) ints for G1, ((x0, x1), (y0, y1)) for G2, None for infinity and for every refused input).  The checks run
in the order the kernel documents: flags, infinity rules, x < p per component, x on the curve, prime-order subgroup.
  on the curve   Euler's criterion on x^3 + b in Fp; in Fp2 "a is a square iff norm(a) is a square in Fp" (zero apart)
  subgroup       r P = O with pyref.ec_mul
  y              the root of y^2 = x^3 + b whose sign under ark's ordering (c1 first, then c0; "larger" = above (p - 1) / 2) is the
                 one the flag asks for.  Fp2 roots come from one exponentiation chain (Adj, Rodriguez-Henriquez, "Square root
                 computation over even extension fields", algorithm 9), not from the complex method the kernel and pyref.f2_sqrt
                 share, and y^2 = x^3 + b is verified before the point is returned.  That root is unique, so a decoder must equal
                 it limb for limb.

cases(cv, group, seed) is the deterministic list of (label, bytes, status, point) the codec tests run: every decode branch and
validation edge, each label asserted non-empty and every expectation the construction implies asserted against classify."""

import functools
import random

from oracle import pyref

STATUS = ["CODEC_OK", "CODEC_NOT_ON_CURVE", "CODEC_UNCOMPRESSED", "CODEC_BAD_FLAGS", "CODEC_INF_NONZERO_X", "CODEC_X_RANGE",
          "CODEC_X_NOT_ON_CURVE", "CODEC_NOT_IN_SUBGROUP", "CODEC_COORD_RANGE"]
CODE = {name: i for i, name in enumerate(STATUS)}
# codec_message() of csrc/codec.hip.h, restated
MESSAGE = {
    "CODEC_NOT_ON_CURVE": b"point is not on the curve",
    "CODEC_UNCOMPRESSED": b"Cannot deserialize point: uncompressed encoding",
    "CODEC_BAD_FLAGS": b"Cannot deserialize point: invalid flags",
    "CODEC_INF_NONZERO_X": b"Cannot deserialize point: non-zero x with the infinity flag",
    "CODEC_X_RANGE": b"Cannot deserialize point: x is not a field element",
    "CODEC_X_NOT_ON_CURVE": b"Cannot deserialize point: x is not on the curve",
    "CODEC_NOT_IN_SUBGROUP": b"Cannot deserialize point: not in the prime-order subgroup",
    "CODEC_COORD_RANGE": b"point coordinates are not reduced field elements",
}
SQRT_MIN = 8   # cases() holds at least this many G2 points (distinct x) for each outcome of the complex method's first attempt


def is_bn(cv):
    return cv.name == "BN254"


def has_cofactor(cv, group):
    return not (is_bn(cv) and group == 1)


def flag_bits(cv):
    """bits of a base-field element's encoding that the flags leave to x"""
    return 254 if is_bn(cv) else 381


# ---- field pieces -----------------------------------------------------------------------------------------------------------
def fp_is_square(a, p):
    a %= p
    return a == 0 or pow(a, (p - 1) // 2, p) == 1


def is_square(a, p):
    """a in Fp (int) or Fp2 (pair); p = 3 mod 4, so the norm of a non-zero element of Fp2 is non-zero"""
    if isinstance(a, int):
        return fp_is_square(a, p)
    return a == (0, 0) or fp_is_square(a[0] * a[0] + a[1] * a[1], p)


def sqrt(a, p):
    """one root of a square a (checked by the caller)"""
    if isinstance(a, int):
        return pow(a, (p + 1) // 4, p)
    if a == (0, 0):
        return a
    mul = lambda u, v: pyref.f2_mul(u, v, p)  # noqa: E731
    a1 = pyref.f2_pow(a, (p - 3) // 4, p)
    x0 = mul(a1, a)
    alpha = mul(a1, x0)                       # a^((p - 1) / 2)
    if alpha == (p - 1, 0):
        return mul((0, 1), x0)
    return mul(pyref.f2_pow(((1 + alpha[0]) % p, alpha[1]), (p - 1) // 2, p), x0)


def is_larger(y, p):
    """ark's y > -y"""
    if isinstance(y, int):
        return y > (p - 1) // 2
    return (y[1] if y[1] else y[0]) > (p - 1) // 2


def first_attempt_is_square(rhs, p):
    """for rhs in Fp2 with c1 != 0: whether (c0 + alpha) / 2 with alpha = norm^((p + 1) / 4), the candidate the complex method
    tries first, is a square (exactly one of (c0 +- alpha) / 2 is: their product is -c1^2 / 4)"""
    alpha = pow((rhs[0] * rhs[0] + rhs[1] * rhs[1]) % p, (p + 1) // 4, p)
    return fp_is_square((rhs[0] + alpha) * pow(2, -1, p), p)


def curve_rhs(cv, group, x):
    g = pyref.Group(cv, group)
    return g.F.add(g.F.mul(g.F.mul(x, x), x), g.b if group == 2 else g.b % cv.p)


# ---- encodings ----------------------------------------------------------------------------------------------------------------
def encode_x(cv, group, comps, sign=False, inf=False, compressed=True):
    """comps: the x components c0 (, c1) as integers of any size the bytes hold; the flags are OR-ed onto them"""
    fb = cv.fp_bytes
    assert len(comps) == group
    if is_bn(cv):
        out = bytearray(b"".join(c.to_bytes(fb, "little") for c in comps))
        out[-1] |= (0x80 if sign else 0) | (0x40 if inf else 0)
    else:
        out = bytearray(b"".join(c.to_bytes(fb, "big") for c in reversed(comps)))
        out[0] |= (0x80 if compressed else 0) | (0x40 if inf else 0) | (0x20 if sign else 0)
    return bytes(out)


def encode_point(cv, group, P):
    """the one valid encoding of a point"""
    if P is None:
        return encode_x(cv, group, [0] * group, inf=True)
    return encode_x(cv, group, [P[0]] if group == 1 else list(P[0]), sign=is_larger(P[1], cv.p))


def classify(cv, group, data):
    data, fb, p = bytes(data), cv.fp_bytes, cv.p
    assert len(data) == fb * group
    if is_bn(cv):
        flags = data[-1] & 0xC0
        body = data[:-1] + bytes([data[-1] & 0x3F])
        if flags == 0xC0:
            return "CODEC_BAD_FLAGS", None
        inf, sign = bool(flags & 0x40), bool(flags & 0x80)
        comps = [int.from_bytes(body[k * fb:(k + 1) * fb], "little") for k in range(group)]
    else:
        flags = data[0] & 0xE0
        body = bytes([data[0] & 0x1F]) + data[1:]
        if not flags & 0x80:
            return "CODEC_UNCOMPRESSED", None
        inf, sign = bool(flags & 0x40), bool(flags & 0x20)
        comps = [int.from_bytes(body[k * fb:(k + 1) * fb], "big") for k in range(group)][::-1]
    if inf:
        if any(comps):
            return "CODEC_INF_NONZERO_X", None
        return ("CODEC_BAD_FLAGS", None) if sign else ("CODEC_OK", None)
    if any(c >= p for c in comps):
        return "CODEC_X_RANGE", None
    x = comps[0] if group == 1 else tuple(comps)
    rhs = curve_rhs(cv, group, x)
    if not is_square(rhs, p):
        return "CODEC_X_NOT_ON_CURVE", None
    g = pyref.Group(cv, group)
    y = sqrt(rhs, p)
    if is_larger(y, p) != sign:
        y = g.F.neg(y)
    assert g.F.mul(y, y) == rhs and (is_larger(y, p) == sign or y == g.F.zero), "the model's own root"
    if has_cofactor(cv, group) and pyref.ec_mul(g.F, (x, y), cv.r) is not None:
        return "CODEC_NOT_IN_SUBGROUP", None
    return "CODEC_OK", (x, y)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def curve_point(cv, group, rnd):
    """a seeded point of the curve (of the whole curve, not of the subgroup)"""
    p = cv.p
    while True:
        x = rnd.randrange(p) if group == 1 else (rnd.randrange(p), rnd.randrange(p))
        rhs = curve_rhs(cv, group, x)
        if is_square(rhs, p) and rhs not in (0, (0, 0)):
            return (x, sqrt(rhs, p))


def real_rhs_points(cv):
    """x = (a, c) in Fp2 with x^3 + b real, i.e. 3 a^2 c - c^3 = -b.c1: the first c = 1, 2, ... with a root a for which the real
    x^3 + b is a square of Fp, and the first for which it is not (its root is then purely imaginary); both a and -a are tried"""
    p, (b0, b1) = cv.p, cv.b2
    found = {}
    c = 0
    while len(found) < 2:
        c += 1
        assert c < 200
        a2 = (c ** 3 - b1) * pow(3 * c, -1, p) % p
        if a2 == 0 or not fp_is_square(a2, p):
            continue
        for a in (pow(a2, (p + 1) // 4, p), p - pow(a2, (p + 1) // 4, p)):
            rhs = curve_rhs(cv, 2, (a, c))
            assert rhs[1] == 0 and rhs[0] != 0
            found.setdefault(fp_is_square(rhs[0], p), (a, c))
    return [found[True], found[False]]


@functools.lru_cache(maxsize=None)
def cases(cv, group, seed):
    p, r, bn = cv.p, cv.r, is_bn(cv)
    g = pyref.Group(cv, group)
    rnd = random.Random(1000 * seed + 10 * group + (0 if bn else 1))
    out = []
    comps = lambda x: [x] if isinstance(x, int) else list(x)  # noqa: E731

    def add(label, data, expect=None):
        status, pt = classify(cv, group, data)
        assert expect is None or status == expect, (label, data.hex(), status, expect)
        out.append((label, data, status, pt))
        return status, pt

    def both_signs(label, x, expect=None):
        return [add(label, encode_x(cv, group, comps(x), sign=s), expect) for s in (False, True)]

    # valid: k G with both sign flags (the other flag reads as -k G), infinity
    def multiple(label_of, k):
        P = g.mul(g.gen, k)
        label = label_of(curve_rhs(cv, group, P[0]))
        for (status, pt), s in zip(both_signs(label, P[0], "CODEC_OK"), (False, True)):
            assert pt == (P if is_larger(P[1], p) == s else g.neg(P)), "sqrt and scalar multiplication disagree"
        return label, P[0]
    for k in [1, 2, r - 1, r - 2] + [rnd.randrange(1, r) for _ in range(3)]:
        multiple(lambda rhs: "valid", k)
    add("valid", encode_point(cv, group, None), "CODEC_OK")
    # both outcomes of the complex method's first candidate: seeded multiples until each outcome has SQRT_MIN of them.  The two
    # sign flags of one x give the square root the same argument, so the count is of distinct x, not of cases.
    sqrt_xs = {"sqrt_first": set(), "sqrt_second": set()}
    while group == 2 and min(len(xs) for xs in sqrt_xs.values()) < SQRT_MIN:
        assert sum(len(xs) for xs in sqrt_xs.values()) < 8 * SQRT_MIN, "about half of all points fall on each side"
        label, x = multiple(lambda rhs: "sqrt_first" if first_attempt_is_square(rhs, p) else "sqrt_second", rnd.randrange(1, r))
        sqrt_xs[label].add(x)

    # x range: p - 1, p, p + 1 and the largest value the unflagged bits hold, in each component; the others keep the generator's x
    gx = comps(g.gen[0])
    for k in range(group):
        widths = [flag_bits(cv)] + ([8 * cv.fp_bytes] if group == 2 and k == 0 else [])   # c0 of G2 shares no byte with the flags
        for v in [p - 1, p, p + 1] + [(1 << w) - 1 for w in widths]:
            x = gx[:k] + [v] + gx[k + 1:]
            below = ("CODEC_OK" if bn else "CODEC_X_NOT_ON_CURVE") if group == 1 else None   # x = p - 1 goes on to the curve check
            if v >= p:
                add("x_range", encode_x(cv, group, x, sign=len(out) % 2 == 1), "CODEC_X_RANGE")
            else:
                both_signs("x_range", x, below)

    # small x
    if group == 1:
        both_signs("small_x", 0, "CODEC_X_NOT_ON_CURVE" if bn else "CODEC_NOT_IN_SUBGROUP")   # BLS12-381: (0, +-2)
    for v in (1, 2, 3):
        for x in ([v], [v, 0], [0, v])[group - 1:2 * group - 1]:
            both_signs("small_x", x)

    # G2: x^3 + b real, so that the root is (s, 0) or (0, s); these points are on the twist and outside the subgroup
    if group == 2:
        for x in real_rhs_points(cv):
            both_signs("real_rhs", x, "CODEC_NOT_IN_SUBGROUP")

    # subgroup: a point of cofactor torsion T = r Q, and P + T for a subgroup point P.  BN254 G1 is the whole curve.
    while not any(c[0] == "subgroup" for c in out):
        Q = curve_point(cv, group, rnd)
        if not has_cofactor(cv, group):
            add("subgroup", encode_point(cv, group, Q), "CODEC_OK")
            continue
        T = pyref.ec_mul(g.F, Q, r)
        if T is None:
            continue
        for pt in (T, g.add(g.mul(g.gen, rnd.randrange(1, r)), T)):
            assert g.is_on_curve(pt)
            add("subgroup", encode_point(cv, group, pt), "CODEC_NOT_IN_SUBGROUP")

    # flags
    valid = encode_point(cv, group, g.mul(g.gen, rnd.randrange(1, r)))
    assert classify(cv, group, valid)[0] == "CODEC_OK"
    add("flags", encode_x(cv, group, [0] * group, sign=True, inf=True), "CODEC_BAD_FLAGS")
    add("flags", encode_x(cv, group, [1] + [0] * (group - 1), inf=True), "CODEC_INF_NONZERO_X")
    add("flags", encode_x(cv, group, gx, inf=True), "CODEC_INF_NONZERO_X")
    if bn:
        add("flags", valid[:-1] + bytes([valid[-1] | 0xC0]), "CODEC_BAD_FLAGS")
    else:
        add("flags", bytes([valid[0] & 0x7F]) + valid[1:], "CODEC_UNCOMPRESSED")

    labels = ["valid", "x_range", "small_x", "subgroup", "flags"] + (["real_rhs", "sqrt_first", "sqrt_second"] if group == 2 else [])
    count = {lb: sum(1 for c in out if c[0] == lb) for lb in labels}
    assert all(count[lb] > 0 for lb in labels) and set(c[0] for c in out) == set(labels), count
    if group == 2:
        assert all(len(xs) >= SQRT_MIN and count[lb] == 2 * len(xs) for lb, xs in sqrt_xs.items()), (count, sqrt_xs)
    return tuple(out)
