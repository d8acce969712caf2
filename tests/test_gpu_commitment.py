"""GPU: the four scenarios the reference tests its commitment package with (a KZG opening, a KZG multi-opening, an IPA opening,
an IPA multi-opening; degree 4 on BN254, drawn setup, blindings and points), through the same public calls of
zksnake_amd.commitment.polynomial.  The multi-opening set is three polynomials at two points: p1 at x, p2 and p3 at x and y."""

import secrets

import pytest

from zksnake_amd.commitment.polynomial import IPA, KZG, MultiOpeningQuery
from zksnake_amd.polynomial import Polynomial

pytestmark = pytest.mark.gpu

SINGLE = {"kzg": [1, 3, 3, 7], "ipa": [1, 2, 22, 7]}
MULTI = ([1, 3, 3, 7], [1, 2, 3, 4], [1, 2, 3, 0])
X, Y = 123, 1234
ASKS = ((0, X), (1, X), (1, Y), (2, X), (2, Y))


def drawn(order):
    return 1 + secrets.randbelow(order)


def multi_query(scheme, blindings=None):
    polys = [Polynomial(list(c), scheme.order) for c in MULTI]
    query = MultiOpeningQuery()
    for k, poly in enumerate(polys):
        if blindings is None:
            query.add_polynomial(poly, scheme.commit(poly))
        else:
            query.add_polynomial(poly, scheme.commit(poly, blindings[k]), blindings[k])
    for k, at in ASKS:
        query.prover_query(polys[k], at)
    return query


def test_kzg(gpu):
    scheme = KZG(4, "BN254")
    scheme.setup()
    poly = Polynomial(SINGLE["kzg"], scheme.order)
    at = drawn(scheme.order)
    proof, value = scheme.open(poly, at)
    assert scheme.verify(scheme.commit(poly), proof, at, value)


def test_multi_kzg(gpu):
    scheme = KZG(4, "BN254")
    scheme.setup()
    proof, for_verifier = scheme.multi_open(multi_query(scheme))
    assert scheme.multi_verify(for_verifier, proof)


def test_ipa_pcs(gpu):
    scheme = IPA(4, "BN254")
    scheme.setup()
    poly = Polynomial(SINGLE["ipa"], scheme.order)
    blinding, at = drawn(scheme.order), drawn(scheme.order)
    commitment = scheme.commit(poly, blinding)
    proof, value = scheme.open(poly, at, commitment, blinding)
    assert scheme.verify(commitment, proof, at, value)


def test_multi_ipa_pcs(gpu):
    scheme = IPA(4, "BN254")
    scheme.setup()
    proof, for_verifier = scheme.multi_open(multi_query(scheme, [drawn(scheme.order) for _ in MULTI]))
    assert scheme.multi_verify(for_verifier, proof)
