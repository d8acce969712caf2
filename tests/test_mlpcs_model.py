"""CPU: the integer model of the multilinear KZG commitment (tests/mlpcs_model.py) against the definitions, for both moduli."""

import random

import pytest

import mle_model
import mlpcs_model as M
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD

FIELDS = (("BN254", BN254_SCALAR_FIELD), ("BLS12_381", BLS12_381_SCALAR_FIELD))


@pytest.mark.parametrize("m", range(7))
@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_identity_and_evaluation_on_random_tables(name, p, m):
    rnd = random.Random(100 * m + (p & 0xFF))
    table = [rnd.randrange(p) for _ in range(1 << m)]
    z = [rnd.randrange(p) for _ in range(m)]
    tau = [rnd.randrange(p) for _ in range(m)]
    levels, v = M.quotient_chain(table, z, p)
    assert [len(q) for q in levels] == [1 << (m - 1 - k) for k in range(m)]
    assert v == M.evaluate(table, z, p) == mle_model.evaluate(table, z, p)
    assert M.identity_holds(table, z, tau, p)
    flat, v2 = M.flat_quotients(table, z, p)
    assert v2 == v and all(flat[M.level_offset(m, k):M.level_offset(m, k) + len(q)] == q for k, q in enumerate(levels))


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_identity_at_the_ends_of_the_range(name, p):
    table = [p - 1, 0, 1, p - 1, 0, 0, 1, 1]
    for z in ([0, 1, p - 1], [p - 1, 0, 1], [1, p - 1, 0], [0, 0, 0], [1, 1, 1]):
        levels, v = M.quotient_chain(table, z, p)
        assert v == M.evaluate(table, z, p)
        for tau in ([p - 1, 1, 0], [5, 7, 11], z):
            assert M.identity_holds(table, z, tau, p)
    # on the hypercube the evaluation is the table's entry
    assert [M.quotient_chain(table, [b & 1, (b >> 1) & 1, b >> 2], p)[1] for b in range(8)] == table
    assert M.quotient_chain([p - 1] * 8, [0, 1, p - 1], p) == ([[0] * 4, [0] * 2, [0]], p - 1)


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_scheme_in_the_exponent(name, p):
    """commit / open with a polynomial of fewer variables than the scheme: the pairing equation as an equation of scalars"""
    rnd = random.Random(9)
    n = 5
    tau = [rnd.randrange(p) for _ in range(n)]
    assert M.eq_basis(tau[3:], p) == [(1 - tau[3]) * (1 - tau[4]) % p, tau[3] * (1 - tau[4]) % p, (1 - tau[3]) * tau[4] % p, tau[3] * tau[4] % p]
    assert sum(M.eq_basis(tau, p)) % p == 1
    for m in range(n + 1):
        table = [rnd.randrange(p) for _ in range(1 << m)]
        z = [rnd.randrange(p) for _ in range(m)]
        c = M.commit(table, tau, p)
        qs, v = M.open_(table, z, tau, p)
        assert len(qs) == m
        assert (c - v - sum(q * (tau[n - m + k] - z[k]) for k, q in enumerate(qs))) % p == 0


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_batch_combination(name, p):
    rnd = random.Random(3)
    m, t = 4, 5
    tables = [[rnd.randrange(p) for _ in range(1 << m)] for _ in range(t)]
    z = [rnd.randrange(p) for _ in range(m)]
    rho = rnd.randrange(p)
    g = M.combine(tables, rho, p)
    assert g == [sum(pow(rho, i, p) * tb[b] for i, tb in enumerate(tables)) % p for b in range(1 << m)]
    assert M.evaluate(g, z, p) == M.combine_scalars([M.evaluate(tb, z, p) for tb in tables], rho, p)
    assert M.combine(tables[:1], rho, p) == tables[0]
