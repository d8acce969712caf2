"""Integer models of the polynomial commitment schemes (reference python/zksnake/commitment/polynomial/{base,kzg,ipa}.py) over
the group arithmetic of oracle.pyref: points are affine tuples (None = infinity), polynomials are lists of ints (low degree
first), and nothing of the package's device path is used.  The models follow the reference's equations the slow way: the IPA
generators ARE folded every round, b is a stored vector, the verifier's g is a product of polynomials, and the multi-opening
divides (q_i - r_i) by prod (X - z) by long division.  They use the package's fixed group order (groups by the lowest commitment
index of their members, members by index, points by first appearance).

Also here: the closed form for structured IPA generators G_i = g_i B, H = h B (one scalar multiplication per MSM), integer
restatements of the two kernels' contracts (include/zkmi.h, zk_pcs_round_dev / zk_pcs_verify_scalars_dev), and the check of the
never-folded identities the package relies on (`check_never_folded`)."""

from ipa_model import h2c
from oracle import pyref
from zksnake_amd.transcript import FiatShamirTranscript


# ---- polynomials as lists of ints ---------------------------------------------------------------------------------------
def strip(a):
    a = list(a)
    while a and a[-1] == 0:
        a.pop()
    return a


def poly_eval(a, x, r):
    acc = 0
    for c in reversed(a):
        acc = (acc * x + c) % r
    return acc


def poly_add(a, b, r):
    n = max(len(a), len(b))
    return [((a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0)) % r for i in range(n)]


def poly_scale(a, s, r):
    return [x * s % r for x in a]


def poly_mul(a, b, r):
    out = [0] * (len(a) + len(b) - 1) if a and b else []
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % r
    return out


def poly_divmod(a, d, r):
    """long division: (quotient, remainder) of a by d (d's leading coefficient non-zero)"""
    a, d = strip(x % r for x in a), strip(x % r for x in d)
    assert d
    q = [0] * max(len(a) - len(d) + 1, 0)
    lead_inv = pow(d[-1], -1, r)
    for k in range(len(a) - len(d), -1, -1):
        q[k] = a[k + len(d) - 1] * lead_inv % r
        for j, y in enumerate(d):
            a[k + j] = (a[k + j] - q[k] * y) % r
    return q, strip(a)


def div_linear(a, z, r):
    """(quotient, remainder) of a by X - z: the recurrence of zk_poly_div_linear_dev"""
    q, acc = [0] * max(len(a) - 1, 0), 0
    for k in range(len(a) - 1, -1, -1):
        acc = (acc * z + a[k]) % r
        if k:
            q[k - 1] = acc
    return q, acc


def div_chain(a, points, r):
    """the quotient of a by prod (X - z) as a chain of linear divisions, remainders ignored"""
    for z in points:
        a, _ = div_linear(a, z, r)
    return a


def vanishing(points, r):
    d = [1]
    for z in points:
        d = poly_mul(d, [-z % r, 1], r)
    return d


def lagrange(xs, ys, r):
    out = []
    for j, (xj, yj) in enumerate(zip(xs, ys)):
        term = [yj % r]
        for k, xk in enumerate(xs):
            if k != j:
                inv = pow(xj - xk, -1, r)
                term = poly_mul(term, [-xk * inv % r, inv], r)
        out = poly_add(out, term, r)
    return out


def dot(x, y, r):
    return sum(p * q for p, q in zip(x, y)) % r


# ---- the multi-point argument, scheme independent ------------------------------------------------------------------------------
def opening_points(asks):
    """asks: [(polynomial index, point)] in query order -> {point: [indices]} as MultiOpeningQuery keeps it"""
    out = {}
    for i, point in asks:
        out.setdefault(point, []).append(i)
    return out


def groups(points_of_query):
    """[(indices, points)] in the fixed order"""
    points_of = {}
    for point, idx in points_of_query.items():
        for i in idx:
            if point not in points_of.setdefault(i, []):
                points_of[i].append(point)
    order = list(points_of_query)
    by_set = {}
    for i in sorted(points_of):
        by_set.setdefault(frozenset(points_of[i]), []).append(i)
    out = [(members, sorted(key, key=order.index)) for key, members in by_set.items()]
    return sorted(out, key=lambda g: g[0][0])


def _append_points(cv, transcript, points):
    transcript.append(b"".join(pyref.compress(cv, 1, p) for p in points))


def multi_open(S, polys, commitments, blindings, asks, transcript=None, randomness=None):
    """(proof, {(point, index): evaluation}) for a scheme model S (KzgModel / IpaModel)"""
    cv, r = S.cv, S.cv.r
    t = transcript or FiatShamirTranscript(S.name, r)
    query = opening_points(asks)
    _append_points(cv, t, commitments)
    evaluations = {}
    for point, idx in query.items():
        for i in idx:
            evaluations[(point, i)] = poly_eval(polys[i], point, r)
            t.append(evaluations[(point, i)])
    x1, x2 = t.get_challenge_scalar(), t.get_challenge_scalar()
    q_polys, q_blinds, f = [], [], []
    for g, (members, points) in enumerate(groups(query)):
        q, blind = [], 0
        for j, i in enumerate(members):
            q = poly_add(q, poly_scale(polys[i], pow(x1, j, r), r), r)
            blind = (blind + pow(x1, j, r) * blindings[i]) % r
        rem_poly = lagrange(points, [poly_eval(q, z, r) for z in points], r)
        quotient, rem = poly_divmod(poly_add(q, poly_scale(rem_poly, r - 1, r), r), vanishing(points, r), r)
        assert not rem
        f = poly_add(f, poly_scale(quotient, pow(x2, g, r), r), r)
        q_polys.append(q)
        q_blinds.append(blind)
    f_commitment, f_blind = S.commit_f(f, randomness)
    _append_points(cv, t, [f_commitment])
    x3 = t.get_challenge_scalar()
    q_x3 = [poly_eval(q, x3, r) for q in q_polys]
    for v in q_x3:
        t.append(v)
    x4 = t.get_challenge_scalar()
    final, final_blind = f, f_blind
    for g, q in enumerate(q_polys):
        final = poly_add(final, poly_scale(q, pow(x4, g + 1, r), r), r)
        final_blind = (final_blind + pow(x4, g + 1, r) * q_blinds[g]) % r
    return [f_commitment] + q_x3 + [S.open_final(final, x3, final_blind, t, randomness)], evaluations


def multi_verify(S, commitments, asks, evaluations, proof, transcript=None):
    cv, r, grp = S.cv, S.cv.r, pyref.G1(S.cv)
    t = transcript or FiatShamirTranscript(S.name, r)
    query = opening_points(asks)
    _append_points(cv, t, commitments)
    for point, idx in query.items():
        for i in idx:
            t.append(evaluations[(point, i)])
    x1, x2 = t.get_challenge_scalar(), t.get_challenge_scalar()
    f_commitment, q_x3, opening = proof[0], list(proof[1:-1]), proof[-1]
    _append_points(cv, t, [f_commitment])
    x3 = t.get_challenge_scalar()
    for v in q_x3:
        t.append(v)
    x4 = t.get_challenge_scalar()
    grps = groups(query)
    if len(grps) != len(q_x3):
        return False
    f_x3, q_x4, final_commitment = 0, 0, f_commitment
    for g, (members, points) in enumerate(grps):
        q_commitment = None
        for j, i in enumerate(members):
            q_commitment = grp.add(q_commitment, grp.mul(commitments[i], pow(x1, j, r)))
        ys = [sum(pow(x1, j, r) * evaluations[(z, i)] for j, i in enumerate(members)) % r for z in points]
        denominator = poly_eval(vanishing(points, r), x3, r)
        f_x3 += pow(x2, g, r) * (q_x3[g] - poly_eval(lagrange(points, ys, r), x3, r)) * pow(denominator, -1, r)
        final_commitment = grp.add(final_commitment, grp.mul(q_commitment, pow(x4, g + 1, r)))
        q_x4 += pow(x4, g + 1, r) * q_x3[g]
    return S.verify_final(final_commitment, opening, x3, (f_x3 + q_x4) % r, t)


# ---- KZG ----------------------------------------------------------------------------------------------------------------
class KzgModel:
    """every commitment is p(tau) G1, so with tau known the model is integer evaluation; `srs()` has the points themselves"""
    name = b"KZG"

    def __init__(self, cv, degree, tau):
        self.cv, self.degree, self.tau = cv, degree, tau % cv.r
        self.g1, self.g2 = pyref.G1(cv), pyref.G2(cv)
        self.g2_tau = self.g2.mul(self.g2.gen, self.tau)

    def srs(self):
        return [self.g1.mul(self.g1.gen, pow(self.tau, i, self.cv.r)) for i in range(self.degree + 1)]

    def commit(self, poly):
        assert len(poly) <= self.degree + 1
        return self.g1.mul(self.g1.gen, poly_eval(poly, self.tau, self.cv.r))

    def open(self, poly, z):
        r = self.cv.r
        value = poly_eval(poly, z, r)
        quotient, rem = poly_divmod(poly_add(poly, [-value % r], r), [-z % r, 1], r)
        assert not rem
        return self.commit(quotient), value

    def verify(self, commitment, proof, z, value):
        """e(proof, tau G2 - z G2) == e(commitment - value G1, G2), as one product of two Miller loops"""
        g1, g2 = self.g1, self.g2
        lhs_q = g2.add(self.g2_tau, g2.neg(g2.mul(g2.gen, z)))
        rhs_p = g1.add(commitment, g1.neg(g1.mul(g1.gen, value)))
        if proof is None or lhs_q is None or rhs_p is None:
            return (proof is None or lhs_q is None) and rhs_p is None
        return pyref.multi_pairing(self.cv, [proof, g1.neg(rhs_p)], [lhs_q, g2.gen]) == pyref.Fp12.one(self.cv)

    # the scheme's part of the multi-point argument
    def commit_f(self, f, randomness):
        return self.commit(f), 0

    def open_final(self, final, x3, blind, transcript, randomness):
        return self.open(final, x3)[0]

    def verify_final(self, commitment, opening, x3, value, transcript):
        return self.verify(commitment, opening, x3, value)


# ---- IPA (BCMS20 appendix A), generators folded ------------------------------------------------------------------------------
class IpaModel:
    """G: n = 2^k affine points, H: one point.  `structured=(g, h)`: G_i = g_i B, H = h B with B the group generator and every MSM
    over G one scalar multiplication (g is folded as integers); G, H may then be None when `gen_bytes` (every compressed G_i,
    then H) is given."""
    name = b"IPA-PCS"

    def __init__(self, cv, G=None, H=None, structured=None, gen_bytes=None):
        self.cv, self.grp = cv, pyref.G1(cv)
        if structured is not None:
            self.gens, self.h = [x % cv.r for x in structured[0]], structured[1] % cv.r
            self.n = len(self.gens)
        else:
            self.gens, self.h, self.n = list(G), None, len(G)
        self.G, self.H = G, H
        assert self.n & (self.n - 1) == 0
        if gen_bytes is None:
            G = G if G is not None else [self.grp.mul(self.grp.gen, x) for x in self.gens]
            H = H if H is not None else self.grp.mul(self.grp.gen, self.h)
            gen_bytes = b"".join(pyref.compress(cv, 1, p) for p in list(G) + [H])
        self.gen_bytes = gen_bytes

    def _msm(self, gens, scalars):
        if self.h is not None:
            return self.grp.mul(self.grp.gen, dot(gens, scalars, self.cv.r))
        return self.grp.msm(gens, scalars)

    def _blind(self, t):
        return self.grp.mul(self.grp.gen, self.h * t) if self.h is not None else self.grp.mul(self.H, t)

    def _fold(self, lo, hi, u):
        if self.h is not None:
            return [(x + u * y) % self.cv.r for x, y in zip(lo, hi)]
        return [self.grp.add(x, self.grp.mul(y, u)) for x, y in zip(lo, hi)]

    def _pad(self, poly):
        assert len(poly) <= self.n
        return [x % self.cv.r for x in poly] + [0] * (self.n - len(poly))

    def _start(self, transcript):
        transcript = transcript or FiatShamirTranscript(self.name, self.cv.r)
        transcript.append(self.gen_bytes)
        return transcript

    def commit(self, poly, blinding):
        return self.grp.add(self._msm(self.gens, self._pad(poly)), self._blind(blinding))

    def open(self, poly, z, commitment, blinding, transcript=None, randomness=None):
        """([L list, R list, C_bar, c, t'], evaluation); randomness = {"poly_r": n ints, "t_bar": int}"""
        cv, grp, r, n = self.cv, self.grp, self.cv.r, self.n
        a = self._pad(poly)
        b = [pow(z, i, r) for i in range(n)]
        value = poly_eval(a, z, r)
        t = self._start(transcript)
        t.append(z)
        t.append(value)
        t.append(pyref.compress(cv, 1, commitment))
        a_bar = self._pad(randomness["poly_r"])
        a_bar[0] = (a_bar[0] - poly_eval(a_bar, z, r)) % r
        t_bar = randomness["t_bar"] % r
        commitment_bar = self.commit(a_bar, t_bar)
        t.append(pyref.compress(cv, 1, commitment_bar))
        alpha = t.get_challenge_scalar()
        c = [(x + alpha * y) % r for x, y in zip(a, a_bar)]
        t_prime = (blinding + alpha * t_bar) % r
        commitment_prime = self._msm(self.gens, c)
        t.append(pyref.compress(cv, 1, commitment_prime))
        h_prime = h2c(t.get_challenge(), b"U", cv)
        t.append(pyref.compress(cv, 1, grp.add(commitment_prime, grp.mul(h_prime, value))))
        Ls, Rs, G = [], [], list(self.gens)
        while n != 1:
            n //= 2
            c_lo, c_hi, b_lo, b_hi, G_lo, G_hi = c[:n], c[n:], b[:n], b[n:], G[:n], G[n:]
            L = grp.add(self._msm(G_lo, c_hi), grp.mul(h_prime, dot(c_hi, b_lo, r)))
            R = grp.add(self._msm(G_hi, c_lo), grp.mul(h_prime, dot(c_lo, b_hi, r)))
            Ls.append(L)
            Rs.append(R)
            t.append(pyref.compress(cv, 1, L))
            t.append(pyref.compress(cv, 1, R))
            u = t.get_challenge_scalar()
            u_inv = pow(u, -1, r)
            c = [(x + y * u_inv) % r for x, y in zip(c_lo, c_hi)]
            b = [(x + y * u) % r for x, y in zip(b_lo, b_hi)]
            G = self._fold(G_lo, G_hi, u)
        return [Ls, Rs, commitment_bar, c[0], t_prime], value

    def verify(self, commitment, proof, z, value, transcript=None):
        cv, grp, r, n = self.cv, self.grp, self.cv.r, self.n
        if len(proof) != 5:
            return False
        Ls, Rs, commitment_bar, c, t_prime = proof
        m = n.bit_length() - 1
        if len(Ls) != m or len(Rs) != m:
            return False
        if commitment is None or commitment_bar is None or t_prime % r == 0 or c % r == 0:
            return False
        t = self._start(transcript)
        t.append(z)
        t.append(value)
        t.append(pyref.compress(cv, 1, commitment))
        t.append(pyref.compress(cv, 1, commitment_bar))
        alpha = t.get_challenge_scalar()
        commitment_prime = grp.add(grp.add(commitment, grp.mul(commitment_bar, alpha)), grp.neg(self._blind(t_prime)))
        t.append(pyref.compress(cv, 1, commitment_prime))
        h_prime = h2c(t.get_challenge(), b"U", cv)
        C = grp.add(commitment_prime, grp.mul(h_prime, value))
        t.append(pyref.compress(cv, 1, C))
        us = []
        for L, R in zip(Ls, Rs):
            if L is None or R is None:
                return False
            t.append(pyref.compress(cv, 1, L))
            t.append(pyref.compress(cv, 1, R))
            u = t.get_challenge_scalar()
            us.append(u)
            C = grp.add(grp.add(grp.mul(L, pow(u, -1, r)), C), grp.mul(R, u))
        g = [1]
        for i in range(m):
            g = poly_mul(g, [1] + [0] * (2 ** i - 1) + [us[m - i - 1]], r)
        b = dot([pow(z, i, r) for i in range(n)], g, r)
        return C == grp.add(grp.mul(self._msm(self.gens, g), c), grp.mul(h_prime, c * b))

    # the scheme's part of the multi-point argument
    def commit_f(self, f, randomness):
        blind = randomness["f_blind"] % self.cv.r
        return self.commit(f, blind), blind

    def open_final(self, final, x3, blind, transcript, randomness):
        return self.open(final, x3, self.commit(final, blind), blind, transcript, randomness)[0]

    def verify_final(self, commitment, opening, x3, value, transcript):
        return self.verify(commitment, opening, x3, value, transcript)


# ---- the kernels' contracts (include/zkmi.h), on lists of ints -------------------------------------------------------------
def round_step(log_n, k, c, s, u, u_inv, z, r):
    """zk_pcs_round_dev: c, s (n ints each) are updated in place; returns (scal_L, scal_R, (eval_hi, eval_lo)), or None when
    k == log_n.  u, u_inv, z may be any non-negative integers (reduced here as on entry there)."""
    n = 1 << log_n
    m = n >> k
    h = m // 2
    if k == 0:
        s[:] = [1] * n
    else:
        u, u_inv = u % r, u_inv % r
        c[:m] = [(x + u_inv * y) % r for x, y in zip(c[:m], c[m:2 * m])]
        sh = log_n - k
        s[:] = [x * u % r if (i >> sh) & 1 else x for i, x in enumerate(s)]
    if k == log_n:
        return None
    z %= r
    pc = [c[(i & (m - 1)) ^ h] * x % r for i, x in enumerate(s)]
    scal_l = [0 if i & h else x for i, x in enumerate(pc)]
    scal_r = [x if i & h else 0 for i, x in enumerate(pc)]
    return scal_l, scal_r, (poly_eval(c[h:m], z, r), poly_eval(c[:h], z, r))


def verify_scalars(log_n, us, c, r):
    """zk_pcs_verify_scalars_dev: [c s_i], s_i = prod_t (bit (log_n-1-t) of i ? u_t : 1), built one bit at a time from the lowest
    (the last challenge) up"""
    out = [c % r]
    for u in reversed(us[:log_n]):
        out = out + [x * (u % r) % r for x in out]
    return out


# ---- the never-folded identities -----------------------------------------------------------------------------------------
def check_never_folded(log_n, r, rnd):
    """Runs the reference's folding of c, b and G (G_i = g_i, integers: the identities are linear in G) beside the kernel
    contract above with random challenges, and asserts round by round that
      <c_hi, G_lo^(k)> = <scal_L, G>,  <c_lo, G_hi^(k)> = <scal_R, G>,
      <c_hi, b_lo^(k)> = B_k eval_hi,  <c_lo, b_hi^(k)> = B_k z^h eval_lo,   b^(k)_j = B_k z^j,
    and at the end c[0], G^(log n) = <s, G>, b^(log n) = B_(log n), g's coefficients = s and <b, g> = prod (1 + u_(m-1-i) z^(2^i))."""
    n = 1 << log_n
    g0 = [rnd.randrange(r) for _ in range(n)]
    z = rnd.randrange(r)
    c_ref = [rnd.randrange(r) for _ in range(n)]
    b0 = [pow(z, i, r) for i in range(n)]
    c_dev, s = list(c_ref), [0] * n
    b_ref, g_ref = list(b0), list(g0)
    us, u, u_inv, b_scale = [], None, None, 1
    for k in range(log_n + 1):
        out = round_step(log_n, k, c_dev, s, u, u_inv, z, r)
        m = n >> k
        assert c_dev[:m] == c_ref and b_ref == [b_scale * pow(z, j, r) % r for j in range(m)]
        if out is None:
            break
        scal_l, scal_r, (e_hi, e_lo) = out
        h = m // 2
        assert dot(c_ref[h:], g_ref[:h], r) == dot(scal_l, g0, r)
        assert dot(c_ref[:h], g_ref[h:], r) == dot(scal_r, g0, r)
        assert dot(c_ref[h:], b_ref[:h], r) == b_scale * e_hi % r
        assert dot(c_ref[:h], b_ref[h:], r) == b_scale * pow(z, h, r) * e_lo % r
        u = rnd.randrange(1, r)
        u_inv = pow(u, -1, r)
        us.append(u)
        c_ref = [(x + y * u_inv) % r for x, y in zip(c_ref[:h], c_ref[h:])]
        b_ref = [(x + y * u) % r for x, y in zip(b_ref[:h], b_ref[h:])]
        g_ref = [(x + y * u) % r for x, y in zip(g_ref[:h], g_ref[h:])]
        b_scale = b_scale * (1 + u * pow(z, h, r)) % r
    assert len(c_ref) == 1 and c_dev[0] == c_ref[0] and g_ref[0] == dot(s, g0, r) and b_ref[0] == b_scale
    g = [1]
    for i in range(log_n):
        g = poly_mul(g, [1] + [0] * (2 ** i - 1) + [us[log_n - i - 1]], r)
    assert g == s == verify_scalars(log_n, us, 1, r)
    closed = 1
    for i in range(log_n):
        closed = closed * (1 + us[log_n - 1 - i] * pow(z, 2 ** i, r)) % r
    assert dot(b0, g, r) == closed == b_scale
