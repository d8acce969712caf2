"""Integer model of the Bulletproofs range proof, single (reference python/zksnake/subprotocol/bulletproofs/range_proof.py:
108-317) and aggregated over m values, each weighted by its own power z^(2+j).  Nothing of the package's device path is used.

The protocol is written once, over a small group interface, and instantiated three ways:
  (a) PointGroup: the curve arithmetic of oracle.pyref on affine tuples.  H is rescaled into H'_k = y^-k H_k and G, H' are
      FOLDED every round as the reference does; the verifier is the reference's single multiexp.
  (b) ExponentGroup with a curve: a group element is its discrete logarithm to the generator P, so G_k = g_k P, H_k = h_k P,
      B = beta P, B~ = beta~ P are integers, every proof point is one scalar multiplication when it is encoded, and
      1024 positions cost what integers cost.
  (d) ExponentGroup without a curve: integers all the way, for fast checks at any size.
and (c) list-of-int restatements of the five kernel contracts of include/zkmi.h.
Randomness and the verifier's c are handed in."""

import hashlib
import itertools

import ipa_model
from oracle import pyref
from zksnake_amd.transcript import FiatShamirTranscript

RANDOMNESS_KEYS = ("s_L", "s_R", "a_blinding", "s_blinding", "v_blinding", "t1_blinding", "t2_blinding")


# ---- groups ----------------------------------------------------------------------------------------------------------------
class PointGroup:
    """G1 of a curve on affine tuples (None = the identity)"""

    def __init__(self, cv):
        self.cv, self.r, self.g = cv, cv.r, pyref.G1(cv)
        self.zero = None

    def add(self, p, q): return self.g.add(p, q)
    def mul(self, p, k): return self.g.mul(p, k)
    def msm(self, points, scalars): return self.g.msm(list(points), [x % self.r for x in scalars])
    def enc(self, p): return pyref.compress(self.cv, 1, p)


class ExponentGroup:
    """the group written additively on its exponents: element x stands for x P.  With a curve the encoding is the compressed
    point x P; without one it is x on 32 bytes."""

    def __init__(self, r, cv=None):
        self.cv, self.r, self.zero = cv, r, 0
        self._g = pyref.G1(cv) if cv is not None else None

    def add(self, p, q): return (p + q) % self.r
    def mul(self, p, k): return p * k % self.r
    def msm(self, points, scalars): return sum(p * k for p, k in zip(points, scalars)) % self.r

    def enc(self, p):
        if self.cv is None:
            return p.to_bytes(32, "little")
        return pyref.compress(self.cv, 1, self._g.mul(self._g.gen, p))


# ---- the proof ---------------------------------------------------------------------------------------------------------------
class Proof:
    def __init__(self, V, A, S, T1, T2, t, t_blinding, e_blinding, a, b, L, R):
        self.V, self.A, self.S, self.T1, self.T2 = list(V), A, S, T1, T2
        self.t, self.t_blinding, self.e_blinding = t, t_blinding, e_blinding
        self.a, self.b, self.L, self.R = a, b, list(L), list(R)

    def replace(self, **kw):
        fields = dict(self.__dict__)
        fields.update(kw)
        return Proof(**fields)


def proof_bytes(grp, proof):
    """the reference's layout (range_proof.py:32-44) with the m V's first"""
    out = b"".join(grp.enc(p) for p in proof.V + [proof.A, proof.S, proof.T1, proof.T2])
    out += b"".join(x.to_bytes(32, "little") for x in (proof.t, proof.t_blinding, proof.e_blinding))
    out += b"".join(grp.enc(L) + grp.enc(R) for L, R in zip(proof.L, proof.R))
    return out + proof.a.to_bytes(32, "little") + proof.b.to_bytes(32, "little")


def label(n, m):
    return n.to_bytes(32, "big") + (m.to_bytes(32, "big") if m > 1 else b"")


def generator_digest(grp, G, H):
    """the one transcript item that stands for the generators: blake2b over every G_k and then every H_k, unscaled"""
    return hashlib.blake2b(b"".join(grp.enc(p) for p in G) + b"".join(grp.enc(p) for p in H)).digest()


def powers(g, count, r, first=1):
    """first * g^k for k < count"""
    return list(itertools.accumulate(itertools.repeat(g, count - 1), lambda x, y: x * y % r, initial=first % r))


def bit_vector(n, m, values):
    return [(values[k // n] >> (k % n)) & 1 for k in range(n * m)]


def _dot(x, y, r):
    return sum(p * q for p, q in zip(x, y)) % r


def delta(n, m, y, z, r):
    """(z - z^2) sum_{k<N} y^k - (sum_{j<m} z^(3+j)) (2^n - 1), by the closed forms of the two geometric series"""
    N = n * m
    sum_y = N % r if y % r == 1 else (pow(y, N, r) - 1) * pow(y - 1, -1, r) % r
    sum_z = m * pow(z, 3, r) % r if z % r == 1 else pow(z, 3, r) * (pow(z, m, r) - 1) * pow(z - 1, -1, r) % r
    return ((z - z * z) * sum_y - sum_z * ((1 << n) - 1)) % r


def _challenges_yz(transcript):
    y = transcript.get_challenge_scalar()
    z = transcript.get_challenge_scalar()
    return y, z


def prove(grp, n, m, G, H, B, B_blinding, values, rnd, transcript=None, gen_digest=None):
    """Proof for `values` (m ints; only bits below n are read, V_j commits to values[j] mod r).  rnd: the mapping of
    RANDOMNESS_KEYS, s_L, s_R lists of n m ints and v_blinding a list of m.  ValueError when the transcript yields
    y = 0, z in {0, 1} or u = 0."""
    r, N = grp.r, n * m
    assert len(G) == len(H) == N and len(values) == m
    transcript = transcript or FiatShamirTranscript(label(n, m), field=r)
    a_l = bit_vector(n, m, values)
    a_r = [(x - 1) % r for x in a_l]
    s_l, s_r = [x % r for x in rnd["s_L"]], [x % r for x in rnd["s_R"]]
    gamma = [x % r for x in rnd["v_blinding"]]
    bases = list(G) + list(H)
    V = [grp.add(grp.mul(B, v % r), grp.mul(B_blinding, g)) for v, g in zip(values, gamma)]
    A = grp.add(grp.msm(bases, a_l + a_r), grp.mul(B_blinding, rnd["a_blinding"] % r))
    S = grp.add(grp.msm(bases, s_l + s_r), grp.mul(B_blinding, rnd["s_blinding"] % r))
    for p in V + [A, S]:
        transcript.append(grp.enc(p))
    y, z = _challenges_yz(transcript)
    if y == 0 or z in (0, 1):
        raise ValueError("degenerate challenge")
    yk = powers(y, N, r)
    zj = powers(z, m, r, first=z * z)
    l0 = [(x - z) % r for x in a_l]
    l1 = s_l
    r0 = [(yk[k] * (a_r[k] + z) + zj[k // n] * (1 << (k % n))) % r for k in range(N)]
    r1 = [yk[k] * s_r[k] % r for k in range(N)]
    t0, t2 = _dot(l0, r0, r), _dot(l1, r1, r)
    # the reference's expression (range_proof.py:171-174); <l0, r1> + <l1, r0> is the same number
    t1 = (_dot([p + q for p, q in zip(l0, l1)], [p + q for p, q in zip(r0, r1)], r) - t0 - t2) % r
    assert t1 == (_dot(l0, r1, r) + _dot(l1, r0, r)) % r
    tau1, tau2 = rnd["t1_blinding"] % r, rnd["t2_blinding"] % r
    T1 = grp.add(grp.mul(B, t1), grp.mul(B_blinding, tau1))
    T2 = grp.add(grp.mul(B, t2), grp.mul(B_blinding, tau2))
    transcript.append(grp.enc(T1))
    transcript.append(grp.enc(T2))
    x = transcript.get_challenge_scalar()
    lx = [(p + x * q) % r for p, q in zip(l0, l1)]
    rx = [(p + x * q) % r for p, q in zip(r0, r1)]
    t = (t0 + t1 * x + t2 * x * x) % r
    t_blinding = (sum(w * g for w, g in zip(zj, gamma)) + tau1 * x + tau2 * x * x) % r
    e_blinding = (rnd["a_blinding"] + x * rnd["s_blinding"]) % r
    for item in (t, t_blinding, e_blinding):
        transcript.append(item)
    w = transcript.get_challenge_scalar()
    Q = grp.mul(B, w)
    transcript.append(gen_digest if gen_digest is not None else generator_digest(grp, G, H))

    # the inner-product argument over G and H'_k = y^-k H_k, both folded every round (ipa.py:105-145)
    y_inv_k = powers(pow(y, -1, r), N, r)
    a, b = lx, rx
    Gf, Hf = list(G), [grp.mul(p, s) for p, s in zip(H, y_inv_k)]
    Ls, Rs = [], []
    while len(a) > 1:
        h = len(a) // 2
        a_lo, a_hi, b_lo, b_hi = a[:h], a[h:], b[:h], b[h:]
        G_lo, G_hi, H_lo, H_hi = Gf[:h], Gf[h:], Hf[:h], Hf[h:]
        L = grp.add(grp.msm(G_hi + H_lo, a_lo + b_hi), grp.mul(Q, _dot(a_lo, b_hi, r)))
        R = grp.add(grp.msm(G_lo + H_hi, a_hi + b_lo), grp.mul(Q, _dot(a_hi, b_lo, r)))
        Ls.append(L)
        Rs.append(R)
        transcript.append(grp.enc(L))
        transcript.append(grp.enc(R))
        u = transcript.get_challenge_scalar()
        if u == 0:
            raise ValueError("degenerate challenge")
        ui = pow(u, -1, r)
        a = [(p * u + q * ui) % r for p, q in zip(a_lo, a_hi)]
        b = [(p * ui + q * u) % r for p, q in zip(b_lo, b_hi)]
        Gf = [grp.add(grp.mul(p, ui), grp.mul(q, u)) for p, q in zip(G_lo, G_hi)]
        Hf = [grp.add(grp.mul(p, u), grp.mul(q, ui)) for p, q in zip(H_lo, H_hi)]
    return Proof(V, A, S, T1, T2, t, t_blinding, e_blinding, a[0], b[0], Ls, Rs)


def _replay(grp, n, m, G, H, proof, transcript, gen_digest):
    """the verifier's challenges (y, z, x, w, [u_t]), or None when one of them is degenerate"""
    r = grp.r
    for p in proof.V + [proof.A, proof.S]:
        transcript.append(grp.enc(p))
    y, z = _challenges_yz(transcript)
    transcript.append(grp.enc(proof.T1))
    transcript.append(grp.enc(proof.T2))
    x = transcript.get_challenge_scalar()
    for item in (proof.t, proof.t_blinding, proof.e_blinding):
        transcript.append(item)
    w = transcript.get_challenge_scalar()
    transcript.append(gen_digest if gen_digest is not None else generator_digest(grp, G, H))
    us = []
    for L, R in zip(proof.L, proof.R):
        transcript.append(grp.enc(L))
        transcript.append(grp.enc(R))
        us.append(transcript.get_challenge_scalar())
    if y == 0 or z in (0, 1) or 0 in us:
        return None
    return y, z, x, w, us


def verify(grp, n, m, G, H, B, B_blinding, proof, c, transcript=None, gen_digest=None):
    """the single multiexp of range_proof.py:282-317 with sum_j c z^(2+j) V_j for its c z^2 V"""
    r, N = grp.r, n * m
    log_n = N.bit_length() - 1
    if len(proof.V) != m or len(proof.L) != log_n or len(proof.R) != log_n:
        return False
    transcript = transcript or FiatShamirTranscript(label(n, m), field=r)
    ch = _replay(grp, n, m, G, H, proof, transcript, gen_digest)
    if ch is None:
        return False
    y, z, x, w, us = ch
    s = ipa_model.s_vector(us, log_n, r)
    a, b = proof.a, proof.b
    y_inv_k = powers(pow(y, -1, r), N, r)
    zj = powers(z, m, r, first=z * z)
    scal_g = [(-z - a * s[k]) % r for k in range(N)]
    scal_h = [(z + y_inv_k[k] * (zj[k // n] * (1 << (k % n)) - b * pow(s[k], -1, r))) % r for k in range(N)]
    points = [proof.A, proof.S] + proof.V + [proof.T1, proof.T2, B, B_blinding] + list(G) + list(H) + proof.L + proof.R
    scalars = ([1, x] + [c * w_j % r for w_j in zj]
               + [c * x % r, c * x * x % r, (w * (proof.t - a * b) + c * (delta(n, m, y, z, r) - proof.t)) % r,
                  (-proof.e_blinding - c * proof.t_blinding) % r]
               + scal_g + scal_h + [u * u % r for u in us] + [pow(u, -2, r) for u in us])
    return grp.msm(points, scalars) == grp.zero


def verify_single_as_the_reference_writes_it(grp, n, G, H, B, B_blinding, proof, c, transcript=None, gen_digest=None):
    """m = 1, term for term as range_proof.py:214-317 has it: z * z for the weight, delta from the two sums, s built by the
    reference's doubling recurrence.  Only the transcript's generator item is this project's."""
    r = grp.r
    transcript = transcript or FiatShamirTranscript(n.to_bytes(32, "big"), field=r)
    y, z, x, w, challenges_raw = _replay(grp, n, 1, G, H, proof, transcript, gen_digest)
    k = len(proof.L)
    challenges = [pow(u, 2, r) for u in challenges_raw]
    challenges_inv = [pow(u, -2, r) for u in challenges_raw]
    all_inv = 1
    for u in challenges_raw:
        all_inv *= pow(u, -1, r)
    s = [all_inv]
    for i in range(1, n):
        lg_i = 32 - 1 - (32 - i.bit_length())
        s.append(s[i - (1 << lg_i)] * challenges[(k - 1) - lg_i])
    a, b = proof.a, proof.b
    sum_pow_2_y = sum(pow(y, i, r) for i in range(n)) % r
    sum_2 = sum(pow(2, i, r) for i in range(n)) % r
    dlt = ((z - pow(z, 2, r)) * sum_pow_2_y - pow(z, 3, r) * sum_2) % r
    scalar_mul_g = [(-z - a * s[i]) % r for i in range(n)]
    scalar_mul_h = [(z + pow(y, -i, r) * (z * z * pow(2, i, r) - b * pow(s[i], -1, r))) % r for i in range(n)]
    points = [proof.A, proof.S, proof.V[0], proof.T1, proof.T2, B, B_blinding] + list(G) + list(H) + proof.L + proof.R
    scalars = [1, x, c * z * z % r, c * x % r, c * x * x % r, (w * (proof.t - a * b) + c * (dlt - proof.t)) % r,
               (-proof.e_blinding - c * proof.t_blinding) % r] + scalar_mul_g + scalar_mul_h + challenges + challenges_inv
    return grp.msm(points, scalars) == grp.zero


# ---- the kernels' contracts (include/zkmi.h), on lists of ints -----------------------------------------------------------------
def _positions(log_bits, log_N, values):
    n, N = 1 << log_bits, 1 << log_N
    assert len(values) == N >> log_bits
    bits = [(v >> i) & 1 for v in values for i in range(n)]
    return n, N, bits


def bits_contract(log_bits, log_N, values, r):
    """zk_rp_bits_dev: a_L || a_R"""
    _, _, bits = _positions(log_bits, log_N, values)
    return bits + [0 if b else r - 1 for b in bits]


def _r0_terms(log_bits, log_N, y, z, r):
    """(y^k, z^(2+j) 2^i) for every position"""
    n, N = 1 << log_bits, 1 << log_N
    yk = powers(y, N, r)
    zj = powers(z, N >> log_bits, r, first=z * z)
    two = [1 << i for i in range(n)]
    zt = [w * t % r for w in zj for t in two]
    return yk, zt


def poly_contract(log_bits, log_N, values, s, y, z, r):
    """zk_rp_poly_dev: (t0, t1, t2); s = s_L || s_R"""
    _, N, bits = _positions(log_bits, log_N, values)
    y, z = y % r, z % r
    yk, zt = _r0_terms(log_bits, log_N, y, z, r)
    l0 = [b - z for b in bits]
    l1, s_r = s[:N], s[N:]
    r0 = [(p * (b - 1 + z) + q) % r for p, b, q in zip(yk, bits, zt)]
    r1 = [p * q % r for p, q in zip(yk, s_r)]
    return (sum(p * q for p, q in zip(l0, r0)) % r,
            (sum(p * q for p, q in zip(l0, r1)) + sum(p * q for p, q in zip(l1, r0))) % r,
            sum(p * q for p, q in zip(l1, r1)) % r)


def eval_contract(log_bits, log_N, values, s, y, y_inv, z, x, r):
    """zk_rp_eval_dev: (l || r, [y_inv^k])"""
    _, N, bits = _positions(log_bits, log_N, values)
    y, y_inv, z, x = y % r, y_inv % r, z % r, x % r
    yk, zt = _r0_terms(log_bits, log_N, y, z, r)
    lx = [(b - z + x * p) % r for b, p in zip(bits, s[:N])]
    rx = [(p * (b - 1 + z + x * q) + t) % r for p, b, q, t in zip(yk, bits, s[N:], zt)]
    return lx + rx, powers(y_inv, N, r)


def verify_scalars_contract(log_bits, log_N, us, a, b, y_inv, z, r):
    """zk_rp_verify_scalars_dev: [-z - a s_k] + [z + y_inv^k (z^(2+j) 2^i - b / s_k)]"""
    N = 1 << log_N
    y_inv, z = y_inv % r, z % r
    ab = ipa_model.verify_scalars(log_N, [u % r for u in us], a, b, r)
    _, zt = _r0_terms(log_bits, log_N, 1, z, r)
    yi = powers(y_inv, N, r)
    return [(-z - p) % r for p in ab[:N]] + [(z + w * (t - q)) % r for w, t, q in zip(yi, zt, ab[N:])]


def seeded_round_contract(log_n, k, a, b, s, s_inv, h_weight, u, u_inv, r):
    """zk_ipa_round_seeded_dev: ipa_model.round_step, except that at k = 0 with weights s_inv starts at h_weight.  In place on
    a, b, s, s_inv; returns (scal_L, scal_R, cross) or None when k == log_n."""
    if k or h_weight is None:
        assert h_weight is None
        return ipa_model.round_step(log_n, k, a, b, s, s_inv, u, u_inv, r)
    n = 1 << log_n
    s[:] = [1] * n
    s_inv[:] = [w % r for w in h_weight]
    if log_n == 0:
        return None
    h = n // 2
    pa = [a[i ^ h] * x % r for i, x in enumerate(s)]
    pb = [b[i ^ h] * x % r for i, x in enumerate(s_inv)]
    scal_l = [x if i & h else 0 for i, x in enumerate(pa)] + [0 if i & h else x for i, x in enumerate(pb)]
    scal_r = [0 if i & h else x for i, x in enumerate(pa)] + [x if i & h else 0 for i, x in enumerate(pb)]
    cross = (sum(p * q for p, q in zip(a[:h], b[h:])) % r, sum(p * q for p, q in zip(a[h:], b[:h])) % r)
    return scal_l, scal_r, cross
