"""Integer model of multilinear polynomials and the sumcheck protocol, written from the definitions with Python integers
only.  A polynomial in n variables is the list of its 2^n values over {0,1}^n; variable 0 is the least significant bit of
the list index.  The GPU kernels (csrc/mle.hip) and the Python front end (mle.py, subprotocol/sumcheck.py) are compared
with it by ==.  The last two sections give exact expectations for tables too large for lists: closed forms on geometric
tables, and one table whose coefficients are known outright."""

import hashlib


# ---- dense tables ----
def fix(table, rs, p):
    """fix variables 0 .. len(rs)-1 to rs"""
    for r in rs:
        table = [(table[2 * j] + r * (table[2 * j + 1] - table[2 * j])) % p for j in range(len(table) // 2)]
    return [v % p for v in table]


def evaluate(table, point, p):
    assert len(table) == 1 << len(point)
    return fix(table, point, p)[0]


def total(table, p):
    return sum(table) % p


def coefficients(table, p):
    """c[S] with f = sum_S c[S] prod_{i in S} x_i, S read as a bit mask (Moebius inversion over subsets)"""
    c = list(table)
    bit = 1
    while bit < len(c):
        for i in range(len(c)):
            if i & bit:
                c[i] = (c[i] - c[i ^ bit]) % p
        bit <<= 1
    return c


def expand(coeffs, point, p):
    """sum_S c[S] prod_{i in S} point[i]"""
    acc = 0
    for mask, c in enumerate(coeffs):
        for i, x in enumerate(point):
            if (mask >> i) & 1:
                c = c * x % p
        acc += c
    return acc % p


def permute(table, perm):
    """out[j] = table[i] where bit t of j is bit perm[t] of i"""
    out = [None] * len(table)
    for i, v in enumerate(table):
        j = 0
        for t, src in enumerate(perm):
            j |= ((i >> src) & 1) << t
        out[j] = v
    return out


def swap_perm(n, a, b, k):
    perm = list(range(n))
    for i in range(k):
        perm[a + i], perm[b + i] = b + i, a + i
    return perm


# ---- the round of a sum of products ----
def line_values(table):
    """per pair (lo, hi) = (table[2j], table[2j+1]) the values of lo + X (hi - lo) at X = 0 .. 3 (not reduced); a table of one
    element is the constant"""
    if len(table) == 1:
        return [list(table)] * 4
    lo, hi = table[0::2], table[1::2]
    return [lo, hi, [2 * h - l for l, h in zip(lo, hi)], [3 * h - 2 * l for l, h in zip(lo, hi)]]


def product_sums(lines, which, p):
    """sum over pairs of prod_{i in which} M_i(X), X = 0 .. 3"""
    out = []
    for x in range(4):
        cols = [lines[i][x] for i in which]
        if len(cols) == 1:
            out.append(sum(cols[0]) % p)
        elif len(cols) == 2:
            out.append(sum(a * b for a, b in zip(*cols)) % p)
        else:
            out.append(sum(a * b * c for a, b, c in zip(*cols)) % p)
    return out


def round_sums(tables, terms, p, cache=None):
    """[s(0), s(1), s(2), s(3)], s(X) = sum_{x'} sum_t c_t prod_j M_tj(X, x'); `cache` (a dict) keeps the per-product sums"""
    lines = {}
    s = [0, 0, 0, 0]
    for c, which in terms:
        key = tuple(sorted(which))
        if cache is None or key not in cache:
            for i in which:
                if i not in lines:
                    lines[i] = line_values(tables[i])
            val = product_sums(lines, which, p)
            if cache is not None:
                cache[key] = val
        else:
            val = cache[key]
        s = [(a + c * b) % p for a, b in zip(s, val)]
    return s


def interpolate(s, p):
    """coefficients (lowest first, trailing zeros dropped) of the polynomial of degree <= 3 through (X, s[X]), by Lagrange"""
    out = [0, 0, 0, 0]
    for j in range(4):
        num, den = [1], 1
        for m in range(4):
            if m != j:
                num = [(a - m * b) % p for a, b in zip([0] + num, num + [0])]   # times (X - m)
                den = den * (j - m) % p
        scale = s[j] * pow(den, -1, p) % p
        out = [(o + scale * c) % p for o, c in zip(out, num)]
    while out and out[-1] == 0:
        out.pop()
    return out


def poly_at(coeffs, x, p):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


# ---- Fiat-Shamir transcript (the byte encoding documented in zksnake_amd/transcript.py) ----
class Transcript:
    def __init__(self, label, p):
        self.p = p
        self.h = hashlib.blake2b(label)

    @staticmethod
    def _int(v):
        return v.to_bytes(v.bit_length(), "big")   # bit_length() BYTES: leading zeros included, 0 is empty

    def append(self, item):
        if isinstance(item, int):
            self.h.update(self._int(item))
        elif isinstance(item, bytes):
            self.h.update(item)
        elif isinstance(item, list) and item:
            self.h.update(b"".join(self._int(v) for v in item))
        else:
            raise TypeError("not a transcript item")

    def challenge(self):
        digest = self.h.digest()
        self.h = hashlib.blake2b(digest)
        return int.from_bytes(digest, "big") % self.p


def f_value(tables, terms, point, p):
    vals = [evaluate(t, point, p) for t in tables]
    acc = 0
    for c, which in terms:
        for i in which:
            c = c * vals[i] % p
        acc += c
    return acc % p


def prove(tables, terms, p, transcript=None):
    """(sum_claim, [coefficient list per round], challenges) of the sumcheck prover for f = sum_t c_t prod_j tables[t_j]"""
    n = len(tables[0]).bit_length() - 1
    s = round_sums(tables, terms, p)
    claim = (s[0] + s[1]) % p if n else s[0]
    tr = transcript or Transcript(b"sumcheck", p)
    tr.append(claim)
    rounds, rs = [], []
    for rnd in range(n):
        if rnd:
            r = tr.challenge()
            rs.append(r)
            tables = [fix(t, [r], p) for t in tables]
            s = round_sums(tables, terms, p)
        coeffs = interpolate(s, p)
        tr.append(coeffs)
        rounds.append(coeffs)
    rs.append(tr.challenge())
    return claim, rounds, rs


def verify(n, claim, rounds, degree_bound, p, transcript=None, final=None):
    """the challenges, or False; `final(point)` gives the polynomial's value for the last check"""
    assert len(rounds) == n
    tr = transcript or Transcript(b"sumcheck", p)
    tr.append(claim)
    rs, expected = [], claim
    for rnd, coeffs in enumerate(rounds):
        if len(coeffs) - 1 > degree_bound:
            return False
        if rnd:
            r = tr.challenge()
            rs.append(r)
            expected = poly_at(rounds[rnd - 1], r, p)
        if expected != (poly_at(coeffs, 0, p) + poly_at(coeffs, 1, p)) % p:
            return False
        tr.append(coeffs)
    r = tr.challenge()
    rs.append(r)
    if final is not None and final(rs) != poly_at(rounds[-1], r, p):
        return False
    return rs


# ---- geometric tables: closed forms where the lists above cannot follow ----
# A table T[i] = c g^i is the triple (c, g, log_n).  Every operation above maps a geometric table to a geometric table or to a
# geometric series, so the expectations below cost O(log n) integer operations at any size.  tests/test_mle_model.py holds
# each of them to the definitions above at small sizes, including the ratios at which a series degenerates.
def geo_table(tab, p):
    c, g, log_n = tab
    return [c * pow(g, i, p) % p for i in range(1 << log_n)]


def geo_sum(first, ratio, count, p):
    """first (1 + ratio + .. + ratio^(count-1))"""
    ratio %= p
    if ratio == 1:
        return first * count % p
    return first * (pow(ratio, count, p) - 1) * pow(ratio - 1, -1, p) % p


def geo_fix(tab, rs, p):
    """T[2j] + r (T[2j+1] - T[2j]) = c (1 + r (g - 1)) (g^2)^j"""
    c, g, log_n = tab
    assert len(rs) <= log_n
    for r in rs:
        c, g, log_n = c * (1 + r * (g - 1)) % p, g * g % p, log_n - 1
    return c, g, log_n


def geo_evaluate(tab, point, p):
    assert len(point) == tab[2]
    return geo_fix(tab, point, p)[0]


def geo_total(tab, p):
    c, g, log_n = tab
    return geo_sum(c, g, 1 << log_n, p)


def geo_round_sums(tabs, terms, p):
    """round_sums: pair j of a table is c g^(2j) (1, g), so its line at X is c (1 + X (g - 1)) (g^2)^j and a term is one series"""
    log_n = tabs[0][2]
    s = [0, 0, 0, 0]
    for coef, which in terms:
        for x in range(4):
            first, ratio = coef, 1
            for i in which:
                c, g, _ = tabs[i]
                first = first * c % p
                if log_n:
                    first = first * (1 + x * (g - 1)) % p
                    ratio = ratio * g * g % p
            s[x] = (s[x] + (geo_sum(first, ratio, 1 << (log_n - 1), p) if log_n else first)) % p
    return s


def geo_coefficient(tab, i, p):
    """f = c prod_b (1 + x_b (g^(2^b) - 1))"""
    c, g, log_n = tab
    assert 0 <= i < 1 << log_n
    b = 0
    while i >> b:
        if (i >> b) & 1:
            c = c * (pow(g, 1 << b, p) - 1) % p
        b += 1
    return c % p


def geo_permuted_at(tab, perm, j, p):
    """element j of permute(table, perm): bit t of j is bit perm[t] of the source index"""
    c, g, _ = tab
    return c * pow(g, sum(((j >> t) & 1) << src for t, src in enumerate(perm)), p) % p


def geo_f_value(tabs, terms, point, p):
    vals = [geo_evaluate(t, point, p) for t in tabs]
    acc = 0
    for c, which in terms:
        for i in which:
            c = c * vals[i] % p
        acc += c
    return acc % p


def geo_prove(tabs, terms, p, transcript=None):
    """prove(), line for line, on triples"""
    n = tabs[0][2]
    s = geo_round_sums(tabs, terms, p)
    claim = (s[0] + s[1]) % p if n else s[0]
    tr = transcript or Transcript(b"sumcheck", p)
    tr.append(claim)
    rounds, rs = [], []
    for rnd in range(n):
        if rnd:
            r = tr.challenge()
            rs.append(r)
            tabs = [geo_fix(t, [r], p) for t in tabs]
            s = geo_round_sums(tabs, terms, p)
        coeffs = interpolate(s, p)
        tr.append(coeffs)
        rounds.append(coeffs)
    rs.append(tr.challenge())
    return claim, rounds, rs


# ---- the table T[i] = p - 1 - i, which needs no model ----
def descending_limbs(p, log_n):
    """T[i] = p - 1 - i as a (2^log_n, 4) uint64 limb array: only the low limb changes while 2^log_n stays below it"""
    import numpy as np
    low = (p - 1) & ((1 << 64) - 1)
    assert (1 << log_n) <= low
    out = np.empty((1 << log_n, 4), dtype=np.uint64)
    out[:, 0] = np.uint64(low) - np.arange(1 << log_n, dtype=np.uint64)
    for k in (1, 2, 3):
        out[:, k] = np.uint64(((p - 1) >> (64 * k)) & ((1 << 64) - 1))
    return out


def descending_coefficient_limbs(p, log_n):
    """its coefficients: f = (p - 1) - sum_b 2^b x_b, so p - 1 at index 0, p - 2^b at index 2^b and zero elsewhere"""
    import numpy as np
    out = np.zeros((1 << log_n, 4), dtype=np.uint64)
    for i, v in [(0, p - 1)] + [(1 << b, p - (1 << b)) for b in range(log_n)]:
        out[i] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint64)
    return out
