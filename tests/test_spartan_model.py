"""CPU: the integer model of Spartan (tests/spartan_model.py) against itself -- the protocol from the dense definition equals the
protocol in linear time, the model verifier accepts the model prover and rejects every single-field tamper, and the layout has
the properties the device code relies on."""

import copy
import random

import pytest

import mlpcs_model as M
import spartan_model as S
from oracle import pyref

FIELDS = tuple(pyref.curve_by_name(name).r for name in ("BN254", "BLS12_381"))
SHAPES = ((1, 2, 1), (2, 3, 1), (3, 5, 2), (5, 9, 3), (8, 6, 5), (16, 8, 1), (13, 10, 2), (4, 16, 8))   # n_row, n_col, n_public


@pytest.mark.parametrize("p", FIELDS, ids=("BN254", "BLS12_381"))
def test_dense_and_linear_formulations_agree(p):
    rnd = random.Random(p % 1000)
    for n_row, n_col, n_public in SHAPES:
        inst, public, private = S.random_instance(rnd, p, n_row, n_col, n_public)
        s_x, h, s = S.sizes(inst)
        assert s_x <= 4 and s <= 4 and S.satisfied(inst, public, private)
        ch, kzg_tau = S.random_challenges(rnd, inst)
        a, b = S.prove_dense(inst, public, private, ch, kzg_tau), S.prove_linear(inst, public, private, ch, kzg_tau)
        assert a == b
        assert all(len(c) == 4 for c in a["outer"]) and all(len(c) == 3 for c in a["inner"])
        assert len(a["outer"]) == s_x and len(a["inner"]) == s and len(a["opening"]) == h
        # the kernel contracts against the dense matrices
        _, z = S.tables(inst, public, private)
        A, B, C = S.dense(inst)
        assert S.products(*S.row_major(inst), z, p) == tuple([sum(x * y for x, y in zip(row, z)) % p for row in m] for m in (A, B, C))
        e = M.eq_basis(ch["rx"], p)
        ra, rb, rc = ch["r_abc"]
        assert S.bind(*S.col_major(inst), e, ch["r_abc"], p) == \
            [sum(e[i] * (ra * A[i][y] + rb * B[i][y] + rc * C[i][y]) for i in range(1 << s_x)) % p for y in range(1 << s)]


def tampers(proof, p):
    """(name, proof with one field moved by one)"""
    for key in ("outer", "inner"):
        for j, coeffs in enumerate(proof[key]):
            for i in range(len(coeffs)):
                t = copy.deepcopy(proof)
                t[key][j][i] = (coeffs[i] + 1) % p
                yield f"{key}[{j}][{i}]", t
    for i in range(3):
        t = copy.deepcopy(proof)
        t["evals"] = tuple((v + (k == i)) % p for k, v in enumerate(proof["evals"]))
        yield f"evals[{i}]", t
    for key in ("v_w", "commitment"):
        t = copy.deepcopy(proof)
        t[key] = (proof[key] + 1) % p
        yield key, t
    for k in range(len(proof["opening"])):
        t = copy.deepcopy(proof)
        t["opening"][k] = (proof["opening"][k] + 1) % p
        yield f"opening[{k}]", t


@pytest.mark.parametrize("p", FIELDS, ids=("BN254", "BLS12_381"))
def test_model_verifier_accepts_the_prover_and_rejects_every_tamper(p):
    rnd = random.Random(7 + p % 1000)
    for n_row, n_col, n_public in SHAPES:
        inst, public, private = S.random_instance(rnd, p, n_row, n_col, n_public)
        ch, kzg_tau = S.random_challenges(rnd, inst)
        proof = S.prove_linear(inst, public, private, ch, kzg_tau)
        assert S.verify(inst, public, proof, ch, kzg_tau)
        for name, bad in tampers(proof, p):
            assert not S.verify(inst, public, bad, ch, kzg_tau), name
        for j in range(n_public):
            moved = [(v + (k == j)) % p for k, v in enumerate(public)]
            assert not S.verify(inst, moved, proof, ch, kzg_tau), f"public[{j}]"
        assert not S.verify(inst, public + [0], proof, ch, kzg_tau)
        # another circuit of the same shape
        other = copy.deepcopy(inst)
        r, c, v = other["A"][0] if other["A"] else (0, 0, 0)
        other["A"] = [(r, c, (v + 1) % p)] + other["A"][1:]
        assert not S.verify(other, public, proof, ch, kzg_tau)
        # a witness that does not satisfy the system gives a proof that is refused
        wrong = list(private) if private else None
        if wrong:
            wrong[0] = (wrong[0] + 1) % p
            if not S.satisfied(inst, public, wrong):
                assert not S.verify(inst, public, S.prove_linear(inst, public, wrong, ch, kzg_tau), ch, kzg_tau)


def test_layout():
    p = FIELDS[0]
    # public wires land at 2^h + j, private ones at j - n_public
    inst = {"A": [], "B": [], "C": [], "n_row": 5, "n_col": 9, "n_public": 3, "p": p}
    s_x, h, s = S.sizes(inst)
    assert (s_x, h, s) == (3, 3, 4)
    assert [S.column(j, 3, h) for j in range(9)] == [8, 9, 10, 0, 1, 2, 3, 4, 5]
    w, z = S.tables(inst, [1, 20, 30], [4, 5, 6, 7, 8, 9])
    assert w == [4, 5, 6, 7, 8, 9, 0, 0] and z == w + [1, 20, 30, 0, 0, 0, 0, 0]
    # z~ splits on variable h
    rnd = random.Random(3)
    ry = [rnd.randrange(p) for _ in range(s)]
    assert M.evaluate(z, ry, p) == ((1 - ry[h]) * M.evaluate(w, ry[:h], p) + ry[h] * S.public_mle([1, 20, 30, 0, 0, 0, 0, 0], ry[:h], p)) % p
    # n_public > n_private sizes h by the public side
    wide = dict(inst, n_col=7, n_public=5)
    assert S.sizes(wide) == (3, 3, 4) and S.column(4, 5, 3) == 12 and S.column(5, 5, 3) == 0
    assert S.sizes(dict(inst, n_col=11, n_public=9)) == (3, 4, 5)
    # one constraint still gives s_x = 1, one private or public wire h = 1
    assert S.sizes(dict(inst, n_row=1, n_col=2, n_public=1)) == (1, 1, 2)
    assert S.sizes(dict(inst, n_row=2)) [0] == 1 and S.sizes(dict(inst, n_row=3))[0] == 2
    # the merged CSR: sub-segment 3 i + m, repeats kept, padding segments empty
    ptr, idx, val = S.merged_csr(4, [[(1, 7, 5), (1, 7, 6), (0, 2, 1)], [], [(3, 0, 9)]])
    assert ptr == [0, 1, 1, 1, 3, 3, 3, 3, 3, 3, 3, 3, 4] and idx == [2, 7, 7, 0] and val == [1, 5, 6, 9]
    assert S.products(ptr, idx, val, [2, 0, 3, 0, 0, 0, 0, 10], p) == ([3, 110, 0, 0], [0, 0, 0, 0], [0, 0, 0, 18])
    assert S.bind(ptr, idx, val, [2, 0, 3, 0, 0, 0, 0, 10], (p + 1, 5, p - 1), p) == [3, 110, 0, p - 18]
