"""Inputs for the fused QAP chain (zk_qap_h_dev, include/zkmi.h) whose u, v and h are known in closed form, so that a dense,
nonzero quotient can be checked element by element at sizes where the CPU oracle's whole chain takes many seconds.  Integers,
numpy and oracle.corc only; nothing of the package's device path.

Notation: n = 2^log_n, w the n-th root of unity of oracle.pyref, forward transform a[k] = sum_e u_e w^(ek) (corc.ntt).  The chain
takes evaluation vectors a, b, c = a o b and gives the coefficient vectors u, v and h with u v = P_lo + X^n P_hi, h = P_hi.

  mixed       random canonical elements, every second one from {0, 1, r-1, r-2} (family A: the expectation is corc.qap_h)
  monomial    family B: u dense, v = beta X^f.  b[k] = beta w^(fk) has period n / gcd(n, f) (2, 4 or 8 for f = n/2, 3n/4, 7n/8), and
              u v = beta X^f u, so h[t] = beta u[t + n - f] for t < f and 0 above: dense over up to 7/8 of the vector, and where it
              is zero P_lo is not, so the chain forms w/2 + (-d/2) from two nonzero halves that must cancel to four zero limbs.
  reflection  family C: u = sum alpha_e X^e over a dozen exponents and b[k] = a[(s - k) mod n], so v has alpha_e w^(se) at
              (n - e) mod n and h[e - e'] collects alpha_e alpha_e' w^(se') over the pairs e >= e' > 0.  The exponents put nonzero
              values at chosen output indices (both ends, and either side of the last pass's run length, of 2048 and of n/2), and
              one coefficient is solved for so that two products meet at one index and cancel exactly.
"""

import random

import numpy as np

from helpers import rand_limbs
from oracle import corc, pyref

CURVES = (("BN254", 0), ("BLS12_381", 1))
TILE_LOG, MAX_DIGIT = 11, 8      # NTT_TILE_LOG, NTT_MAX_DIGIT of csrc/ntt_plan.h


def plan(log_n):
    """[(stages m, run length exponent q)] of the passes ntt_dev_impl launches for a 2^log_n transform: ntt_plan of csrc/ntt_plan.h, restated
    (tests/test_host_lib.py compares the two on the CPU)"""
    if log_n == 0:
        return []
    passes = 1 if log_n <= TILE_LOG else -(-log_n // MAX_DIGIT)
    digits, rest = [], log_n
    for i in range(passes):
        digits.append(rest // (passes - i))
        rest -= digits[-1]
    while True:      # odd stage counts are paired up into even ones
        odd = [i for i, d in enumerate(digits) if d & 1]
        if len(odd) < 2:
            break
        a, b = odd[0], odd[1]
        if digits[a] < MAX_DIGIT:
            digits[a] += 1
            digits[b] -= 1
        elif digits[b] < MAX_DIGIT:
            digits[b] += 1
            digits[a] -= 1
        else:
            break
    digits.sort(reverse=True)
    if passes >= 3:  # the smallest digit goes to the middle
        digits.insert(passes // 2, digits.pop())
    return [(m, 0 if passes == 1 else min(TILE_LOG - m, log_n - m)) for m in digits]


def limbs(vals):
    return corc.ints_to_limbs(vals, 4)


def mul(cid, a, b, threads=8):
    """a o b by corc.vec_op, which is one thread's work: long vectors are cut into row blocks (ctypes drops the GIL)"""
    n = a.shape[0]
    if n < 1 << 16:
        return corc.vec_op(cid, "mul", a, b)
    from concurrent.futures import ThreadPoolExecutor
    cuts = [n * i // threads for i in range(threads + 1)]
    with ThreadPoolExecutor(threads) as pool:
        parts = pool.map(lambda lo_hi: corc.vec_op(cid, "mul", a[lo_hi[0]:lo_hi[1]], b[lo_hi[0]:lo_hi[1]]), zip(cuts, cuts[1:]))
        return np.concatenate(list(parts))


def sparse_limbs(n, entries):
    """(n, 4) limbs, zero but for {index: value}"""
    out = np.zeros((n, 4), dtype=np.uint64)
    if entries:
        idx = sorted(entries)
        out[idx] = limbs([entries[i] for i in idx])
    return out


def mixed(cv, n, seed):
    """n canonical elements: random below 2^252, every second one from {0, 1, r-1, r-2}"""
    rng = np.random.default_rng(seed)
    out = rand_limbs(n, seed)
    edge = limbs([0, 1, cv.r - 1, cv.r - 2])
    out[0::2] = edge[rng.integers(0, 4, size=(n + 1) // 2)]
    return out


# ---- family B: dense times a monomial ---------------------------------------------------------------------------------------
def monomial_shifts(n):
    """the f of family B: n/2, 3n/4, 7n/8 where they are integers with 0 < f < n"""
    return [num * n // den for num, den in ((1, 2), (3, 4), (7, 8)) if n % den == 0]


def monomial_beta(cv, n, f):
    """r - 1 for the largest f of a size, a fixed 128-bit value for the others"""
    return cv.r - 1 if f == monomial_shifts(n)[-1] else 0xC2B2AE3D27D4EB4F165667B19E3779F9 ^ f


def monomial_evals(cv, n, f, beta):
    """b[k] = beta w^(fk): one period in Python integers, tiled"""
    wf = pow(cv.root_of_unity(n), f, cv.r)
    period = next(p for p in (1, 2, 4, 8) if pow(wf, p, cv.r) == 1)
    assert n % period == 0
    return np.tile(limbs([beta * pow(wf, k, cv.r) % cv.r for k in range(period)]), (n // period, 1))


def monomial_case(cid, cv, u, a, f, beta):
    """u: dense coefficients, a = corc.ntt(u).  Returns (b, c, v, h) for v = beta X^f; u itself is the expected u."""
    n = u.shape[0]
    assert 0 < f < n and 0 < beta < cv.r
    b = monomial_evals(cv, n, f, beta)
    c = mul(cid, a, b)
    v = sparse_limbs(n, {f: beta})
    h = np.zeros((n, 4), dtype=np.uint64)
    h[:f] = mul(cid, u[n - f:], np.tile(limbs([beta]), (f, 1)))
    assert not h[n - 1].any()
    return b, c, v, h


# ---- family C: sparse times its reflection -----------------------------------------------------------------------------------
def reflection_targets(log_n):
    """output indices at which h must be nonzero: both ends, and B - 1 and B for B = the last pass's run length, 2048 and n/2"""
    n = 1 << log_n
    marks = {1 << plan(log_n)[-1][1], 2048, n // 2}
    return sorted({0, 1, n - 2} | {t for B in marks if B < n for t in (B - 1, B)})


def _products(alpha, s, w, r):
    """{index t of h: [alpha_e alpha_e' w^(s e') for the pairs e - e' = t, e >= e' > 0]} (Python integers)"""
    out = {}
    for e, x in alpha.items():
        for e2, y in alpha.items():
            if e >= e2 > 0:
                out.setdefault(e - e2, []).append(x * y * pow(w, s * e2, r) % r)
    return out


class Reflection:
    """u = sum alpha[e] X^e, the shift s, the expected v and h as {index: value}, and `cancel`: the index at which two products
    sum to zero.  Everything here is integer work on a dozen terms; `case` takes the one oracle transform."""

    def __init__(self, cv, log_n, seed=0):
        assert log_n >= 3
        r, n = cv.r, 1 << log_n
        w = cv.root_of_unity(n)
        rnd = random.Random(1000 * log_n + seed + (r & 0xFF))
        self.n, self.targets = n, reflection_targets(log_n)
        self.s = s = (rnd.randrange(n) | 1) % n
        # t + 1 for every target t: with exponent 1 below it that is the difference t (and 2 gives t - 1 once more); exponent 0
        # reaches v[0] and no h at all
        expo = {0, 1, 2, n - 1} | {t + 1 for t in self.targets if 0 < t + 1 < n}
        while log_n >= 6 and len(expo) < 9:
            expo.add(rnd.randrange(3, n - 1))
        special = [1, r - 1, r - 2, (r + 1) // 2]
        alpha = {e: special[i // 2 % 4] if i % 2 == 0 else rnd.randrange(1, r) for i, e in enumerate(sorted(expo))}
        # one more exponent z whose coefficient is solved for: at some index outside the targets exactly two products meet, one
        # of them linear in alpha_z, and they cancel
        self.cancel = None
        for z in [e for e in list(range(3, min(n, 40))) + [rnd.randrange(3, n) for _ in range(40)] if e not in alpha]:
            trial = dict(alpha)
            trial[z] = 1
            pairs = {}
            for e in trial:
                for e2 in trial:
                    if e >= e2 > 0:
                        pairs.setdefault(e - e2, []).append((e, e2))
            for t, pl in sorted(pairs.items()):
                with_z = [p for p in pl if z in p]
                if len(pl) == 2 and len(with_z) == 1 and t not in self.targets and t != 0:
                    (e, e2), = [p for p in pl if z not in p]
                    other = alpha[e] * alpha[e2] * pow(w, s * e2, r) % r
                    ze, ze2 = with_z[0]
                    unit = alpha[ze2 if ze == z else ze] * pow(w, s * ze2, r) % r     # the z product per unit of alpha_z
                    alpha[z] = (r - other) * pow(unit, -1, r) % r
                    self.cancel = t
                    break
            if self.cancel is not None:
                break
        assert self.cancel is not None, "no exponent gives a cancelling pair"
        self.alpha = alpha
        self.v = {(n - e) % n: x * pow(w, s * e, r) % r for e, x in alpha.items()}
        prods = _products(alpha, s, w, r)
        self.h = {t: sum(pl) % r for t, pl in prods.items()}
        # what the inputs promise, asserted here so that an empty support cannot pass silently
        assert all(0 < x < r for x in alpha.values()) and 6 <= len(alpha) <= 12
        assert all(self.h.get(t, 0) != 0 for t in self.targets), "a target index of h is zero"
        assert len(prods[self.cancel]) == 2 and all(prods[self.cancel]) and self.h[self.cancel] == 0
        assert max(self.h) <= n - 2, "h[n-1] must be zero"
        assert any(x in (r - 1, r - 2, (r + 1) // 2) for x in alpha.values())

    def coefficients(self):
        return sparse_limbs(self.n, self.alpha)

    def case(self, cid, a):
        """a = corc.ntt(coefficients()).  Returns (b, c, u, v, h) as limbs."""
        n = self.n
        b = np.ascontiguousarray(a[(self.s - np.arange(n)) % n])
        c = mul(cid, a, b)
        return b, c, self.coefficients(), sparse_limbs(n, self.v), sparse_limbs(n, self.h)


# ---- for the tests: a second reference for the closed forms, and a wrong entry for the divisibility flag ---------------------------
def schoolbook_high(u, v, r):
    """P_hi of the product of two coefficient lists (Python integers)"""
    n = len(u)
    out = [0] * n
    for i, x in enumerate(u):
        if x:
            for j, y in enumerate(v):
                if i + j >= n:
                    out[i + j - n] = (out[i + j - n] + x * y) % r
    return out


def flip_limb(c, index, r):
    """a copy of c with one limb of element `index` changed by one bit, still canonical"""
    val = corc.limbs_to_ints(c[index:index + 1])[0]
    for limb in range(4):
        new = val ^ (1 << (64 * ((index + limb) % 4)))
        if new < r:
            out = c.copy()
            out[index] = limbs([new])[0]
            return out
    raise AssertionError("no limb can be flipped")


def curve(name):
    return pyref.curve_by_name(name)
