"""
Sumcheck with the reference's interface and transcript (python/zksnake/subprotocol/sumcheck.py:11-185): the label is
b"sumcheck", the claimed sum is appended first, every round appends the round polynomial's `coeffs()`, a challenge is
drawn between rounds and one more at the end.

The prover's per-round work -- fix one variable of every table, then sum f(X, x') over the rest of the hypercube at four
values of X -- is ONE pass on the GPU (zk_sumcheck_round_dev) for polynomials of the form
    f(x) = sum_t c_t * prod_j M_{t,j}(x),        at most 3 factors per term, 8 terms, 8 tables          (ProductPolynomial)
which covers a plain multilinear polynomial (one table, one factor) and both phases of the GKR round polynomial
add*(W_b + W_c) + mul*W_b*W_c as subprotocol/gkr.py builds them from per-gate sums (GkrPolynomial: tables of one layer's size;
broadcasting add, mul, W_b, W_c to the same 2k variables works too but costs 2^(2k) elements per table).  The reference evaluates s at the
four 4th roots of unity and runs an inverse FFT (sumcheck.py:49-58); here s(0), s(1), s(2), s(3) come back from the device
and are interpolated with Python integers -- the same polynomial of degree <= 3, hence the same `coeffs()`.

As in the reference, a round polynomial that is identically zero has `coeffs() == []`, which `transcript.append` rejects with
TypeError; that is left as it is.  The verifier is host-only.
"""

from ..mle import MLE_OBJECT, MultilinearPolynomial, sumcheck_round
from ..frvec import DevVec, FrOps
from ..polynomial import Polynomial
from ..transcript import FiatShamirTranscript
from .. import _native as N


class SumcheckPolynomial:
    """What `Sumcheck.prove_arbitrary` needs from a polynomial in `n` variables over the field `p`."""

    def __init__(self, n, p):
        self.n = n
        self.p = p

    def to_evaluations(self):
        """the values over the boolean hypercube"""
        raise NotImplementedError

    def evaluate(self, points):
        """the value at `points` (one field element per variable)"""
        raise NotImplementedError

    def first_round(self):
        """the univariate polynomial of round 1: variable 0 free, the others summed over {0,1}"""
        raise NotImplementedError

    def round_function(self, r):
        """the univariate polynomial of a later round: `r` is the list of all challenges so far, one per fixed variable"""
        raise NotImplementedError


def round_polynomial(s, p):
    """the polynomial of degree <= 3 through (0, s[0]) .. (3, s[3]) as the project's Polynomial (Newton forward differences)"""
    d1 = s[1] - s[0]
    d2 = s[2] - 2 * s[1] + s[0]
    d3 = s[3] - 3 * s[2] + 3 * s[1] - s[0]
    i2, i3, i6 = pow(2, -1, p), pow(3, -1, p), pow(6, -1, p)
    return Polynomial([s[0] % p, (d1 - d2 * i2 + d3 * i3) % p, (d2 * i2 - d3 * i2) % p, d3 * i6 % p], p)


class ProductPolynomial(SumcheckPolynomial):
    """f(x) = sum_t coeff_t * prod_{i in tables_t} mlpolys[i](x), device resident.

    mlpolys: MultilinearPolynomials over the same variables (at most 8); terms: [(coeff, (i, j, ..)), ..] with 1 .. 3 table
    indices per term (at most 8 terms); an index may repeat within a term and across terms.  The input polynomials are never
    modified: folded copies are kept between calls of `round_function`."""

    def __init__(self, mlpolys, terms, p=None):
        mlpolys = list(mlpolys)
        if not 1 <= len(mlpolys) <= 8:
            raise ValueError("1 .. 8 multilinear polynomials")
        p = p or mlpolys[0].p
        n = mlpolys[0].num_vars
        for m in mlpolys:
            if not isinstance(m, MultilinearPolynomial) or m.p != p or m.num_vars != n:
                raise ValueError("all tables must be MultilinearPolynomials over the same field and variables")
        terms = [(int(c) % p, tuple(int(i) for i in which)) for c, which in terms]
        if not 1 <= len(terms) <= 8:
            raise ValueError("1 .. 8 terms")
        for _, which in terms:
            if not 1 <= len(which) <= 3 or any(not 0 <= i < len(mlpolys) for i in which):
                raise ValueError("a term is a product of 1 .. 3 of the given tables")
        super().__init__(n, p)
        self.mlpolys, self.terms = mlpolys, terms
        self._ops = FrOps(p)
        self._fixed, self._cur = [], None   # challenges folded so far and the folded tables (None: the originals)

    def degree(self):
        return max(len(which) for _, which in self.terms)

    def to_evaluations(self):
        ops, size = self._ops, 1 << self.n
        acc, tmp = DevVec(size), DevVec(size, zero=False)
        for c, which in self.terms:
            first = self.mlpolys[which[0]].device_ptr()
            if len(which) == 1:
                ops.d_axpy(size, acc.ptr(), c, first)
                continue
            ops.d_mul(size, first, self.mlpolys[which[1]].device_ptr(), tmp.ptr())
            for i in which[2:]:
                ops.d_mul(size, tmp.ptr(), self.mlpolys[i].device_ptr(), tmp.ptr())
            ops.d_axpy(size, acc.ptr(), c, tmp.ptr())
        return ops.ints(acc.download(size))

    def sum(self):
        """sum over the hypercube, without the table: s(0) + s(1) of the first round"""
        s = self._round(self.n, [m.device_ptr() for m in self.mlpolys])
        return (s[0] + s[1]) % self.p if self.n else s[0]

    def evaluate(self, points):
        vals = [m.evaluate(points) for m in self.mlpolys]
        total = 0
        for c, which in self.terms:
            for i in which:
                c = c * vals[i] % self.p
            total += c
        return total % self.p

    def _round(self, log_n, ptrs, r=None, out=None):
        return sumcheck_round(self._ops, log_n, ptrs, self.terms, r, out)

    def first_round(self):
        return round_polynomial(self._round(self.n, [m.device_ptr() for m in self.mlpolys]), self.p)

    def round_function(self, r):
        r = [int(x) % self.p for x in r]
        if not r:
            return self.first_round()
        if len(r) > self.n:
            raise ValueError("more challenges than variables")
        k = len(r) - 1
        if self._cur is None or self._fixed != r[:k]:
            # restart from the untouched originals: fix the prefix in one chain per table
            if k == 0:
                self._cur = None
            else:
                lib, cur = N.load(), []
                pts = self._ops.limbs(r[:k])
                for m in self.mlpolys:
                    vec = DevVec(1 << (self.n - k), zero=False)
                    N.check(lib.zk_mle_fix_dev(self._ops.cid, self.n, m.device_ptr(), k, N.u64p(pts), vec.ptr(), None))
                    cur.append(vec)
                self._cur = cur
            self._fixed = r[:k]
        log_n = self.n - k
        src = [m.device_ptr() for m in self.mlpolys] if self._cur is None else [v.ptr() for v in self._cur]
        out = [DevVec(1 << (log_n - 1), zero=False) for _ in self.mlpolys]
        s = self._round(log_n, src, r[-1], [v.ptr() for v in out])   # fold the new challenge and sum in one pass
        self._cur, self._fixed = out, r
        return round_polynomial(s, self.p)


class Sumcheck:
    """Prove / verify that a polynomial in `n` variables over the field of size `order` sums to a claimed value over {0,1}^n."""

    def __init__(self, n, order):
        self.n = n
        self.order = order

    def prove(self, mlpoly, transcript=None):
        """(sum_claim, [round polynomials], challenges) for a MultilinearPolynomial: the one-table, one-factor ProductPolynomial"""
        assert mlpoly.num_vars == self.n
        return self.prove_arbitrary(ProductPolynomial([mlpoly], [(1, (0,))], self.order), transcript)

    def prove_arbitrary(self, poly, transcript=None):
        """(sum_claim, [round polynomials], challenges) for any SumcheckPolynomial.  Pass the caller's `transcript` when this
        runs inside a larger protocol, so that the challenges depend on what came before."""
        assert poly.n == self.n
        if callable(getattr(poly, "sum", None)):
            sum_claim = poly.sum()     # the same number as below, without moving the table to the host (ProductPolynomial, GkrPolynomial)
        else:
            sum_claim = sum(poly.to_evaluations()) % self.order
        transcript = transcript or FiatShamirTranscript(b"sumcheck", field=self.order)
        transcript.append(sum_claim)
        proof, challenges = [], []
        for rnd in range(self.n):
            if rnd == 0:
                uni = poly.first_round()
            else:
                r = transcript.get_challenge_scalar()
                challenges.append(r)
                uni = poly.round_function(list(challenges))
                assert proof[-1](r) == (uni(0) + uni(1)) % self.order
            transcript.append(uni.coeffs())
            proof.append(uni)
        challenges.append(transcript.get_challenge_scalar())
        return sum_claim, proof, challenges

    def verify(self, sum_claim, proof, degree_bound, transcript=None, mlpoly=None):
        """The list of challenges when `proof` is consistent with `sum_claim` and no round polynomial exceeds `degree_bound`,
        else False.  With `mlpoly` (anything with `evaluate(points)`) the last check -- the polynomial at the challenges equals
        the last round polynomial at the last challenge -- is made here; without it that check is the caller's."""
        assert len(proof) == self.n
        transcript = transcript or FiatShamirTranscript(b"sumcheck", field=self.order)
        transcript.append(sum_claim)
        challenges = []
        expected = sum_claim
        for rnd, uni in enumerate(proof):
            if uni.degree() > degree_bound:
                return False
            if rnd > 0:
                r = transcript.get_challenge_scalar()
                challenges.append(r)
                expected = proof[rnd - 1](r)
            if expected != (uni(0) + uni(1)) % self.order:
                return False
            transcript.append(uni.coeffs())
        r = transcript.get_challenge_scalar()
        challenges.append(r)
        if mlpoly is not None and mlpoly.evaluate(challenges) != proof[-1](r):
            return False
        return challenges


__all__ = ["MLE_OBJECT", "ProductPolynomial", "Sumcheck", "SumcheckPolynomial", "round_polynomial"]
