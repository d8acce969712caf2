"""CPU: the integer model of Poseidon (tests/poseidon_model.py) against values that do not come from this repository -- the
published hash of (1, 2, 3), circomlibjs's hash of (1, 2), and the reference's circom fixture solved on arbitrary inputs -- and
the structure of its parameters."""

import os
import random

import pytest

import poseidon_model as M
from zksnake_amd.arithmetization import R1CS

GOLD = os.path.join(os.path.dirname(__file__), "golden")
R_BN = M.R["BN254"]
HASH_1_2_3 = 0x0E7732D89E6939C0FF03D5E58DAB6302F3230E269DC5B968F725DF34AB36D732
HASH_1_2 = 7853200120776062878684798364095072458815029376092732009249414926327459813530


def test_hash_of_1_2_3_is_the_published_value():
    assert M.hash("BN254", [1, 2, 3]) == HASH_1_2_3


def test_hash_of_1_2_is_the_value_remembered_from_circomlibjs():
    """pins width 3: the same generator with t = 3 reproduces circomlibjs's poseidon([1, 2])"""
    assert M.hash("BN254", [1, 2]) == HASH_1_2


@pytest.fixture(scope="module")
def fixture_circuit():
    return R1CS.from_file(os.path.join(GOLD, "test_poseidon.r1cs"), os.path.join(GOLD, "test_poseidon.sym"))


def test_width_4_is_the_circom_fixture_on_arbitrary_inputs(fixture_circuit):
    """the public output of the reference's Poseidon(3) circuit, solved from its three inputs, for the all-zero and the
    all-(r - 1) triple and three seeded random ones"""
    rng = random.Random(4)
    triples = [(0, 0, 0), (R_BN - 1,) * 3] + [tuple(rng.randrange(R_BN) for _ in range(3)) for _ in range(3)]
    for a, b, c in triples:
        solved = fixture_circuit.solve({"main.a": a, "main.b": b, "main.c": c})
        assert solved["main.h"] == M.hash("BN254", [a, b, c]), (a, b, c)


@pytest.mark.parametrize("t", M.WIDTHS)
@pytest.mark.parametrize("curve", sorted(M.R))
def test_parameter_structure(curve, t):
    r, rf, rp, rc, mds = M.params(curve, t)
    flat, xs, ys = M.generate(curve, t)
    assert (rf, rp) == (8, {3: 57, 4: 56, 5: 60}[t]) and r == M.R[curve]
    assert len(flat) == (rf + rp) * t and len(rc) == rf + rp and all(len(row) == t for row in rc)
    assert all(0 <= c < r for c in flat) and len(set(flat)) == len(flat)
    # the Cauchy matrix of 2 t distinct points: M[i][j] (x_i + y_j) = 1
    assert len(set(xs + ys)) == 2 * t and all(0 <= v < r for v in xs + ys)
    assert len(mds) == t and all(len(row) == t for row in mds)
    assert all(mds[i][j] * (xs[i] + ys[j]) % r == 1 for i in range(t) for j in range(t))
    # invertible: Gaussian elimination mod r finds t pivots
    m, rank = [row[:] for row in mds], 0
    for col in range(t):
        piv = next((i for i in range(rank, t) if m[i][col]), None)
        assert piv is not None
        m[rank], m[piv] = m[piv], m[rank]
        inv = pow(m[rank][col], -1, r)
        for i in range(rank + 1, t):
            f = m[i][col] * inv % r
            m[i] = [(a - f * b) % r for a, b in zip(m[i], m[rank])]
        rank += 1
    assert rank == t


@pytest.mark.parametrize("curve", sorted(M.R))
def test_different_widths_and_curves_give_different_constants(curve):
    heads = {t: M.generate(curve, t)[0][:8] for t in M.WIDTHS}
    assert not set(heads[3]) & set(heads[4]) and not set(heads[4]) & set(heads[5]) and not set(heads[3]) & set(heads[5])
    assert M.generate("BN254", 3)[0][:8] != M.generate("BLS12_381", 3)[0][:8]


def test_grain_start_state():
    """the first round constant of BN254, t = 3, as circomlib's table has it"""
    assert M.params("BN254", 3)[3][0][0] == 0x0EE9A592BA9A9518D05986D656F40C2114C4993C11BB29938D21D47304CD8E6E


@pytest.mark.parametrize("curve", sorted(M.R))
def test_sponge_and_tree_definitions(curve):
    r = M.R[curve]
    # a one-block sponge is one permutation of [L, x_0, x_1]; a missing last element adds nothing
    assert M.sponge(curve, [5, 6]) == M.perm(curve, [2, 5, 6])[1] and M.sponge(curve, [5]) == M.perm(curve, [1, 5, 0])[1]
    assert M.sponge(curve, [5]) != M.sponge(curve, [5, 0])          # the length separates them
    s = M.perm(curve, [3, 5, 6])
    assert M.sponge(curve, [5, 6, 7]) == M.perm(curve, [s[0], (s[1] + 7) % r, s[2]])[1]
    assert M.hash(curve, [5, 6]) == M.perm(curve, [0, 5, 6])[0]
    # five leaves: 5 + 3 + 2 + 1 nodes, the odd node hashed with itself, and every path verifies
    leaves = [M.sponge(curve, [i]) for i in range(5)]
    lv = M.levels(curve, leaves)
    assert [len(level) for level in lv] == [5, 3, 2, 1] and lv[1][2] == M.hash(curve, [leaves[4], leaves[4]])
    for i in range(5):
        assert len(M.path(lv, i)) == 3 and M.verify(curve, M.root(lv), M.path(lv, i), i, leaves[i])
    assert M.path(lv, 4)[:2] == [leaves[4], lv[1][2]]
    assert not M.verify(curve, M.root(lv), M.path(lv, 1), 2, leaves[1])
    assert M.levels(curve, [7]) == [[7]] and M.path([[7]], 0) == []
