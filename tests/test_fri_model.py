"""CPU: the integer model of the FRI polynomial commitment (tests/fri_model.py) is a sound yardstick -- honest proofs verify at
every shape, every single tampering is refused, and proofs of a wrong value built in evaluation space are refused."""

import copy
import random

import pytest

import fri_model as M

SHAPES = [(1, 1, 0), (2, 2, 1), (3, 2, 1), (4, 1, 0), (3, 3, 0), (6, 2, 2)]
CURVES = ["BN254", "BLS12_381"]
# seeds of the cheating proofs: fixed, so the outcome below is deterministic (all rejected; confirmed on the CPU)
CHEAT_SEEDS = [11, 12, 13, 14]


def rand_poly(rng, r, count):
    return [rng.randrange(r) for _ in range(count)]


def rand_point(rng, P):
    while True:
        z = rng.randrange(P.r)
        if not M.in_domain(P, z):
            return z


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("k,b,f", SHAPES)
def test_honest_proofs_verify(curve, k, b, f):
    P = M.Params(curve, k, b, f, queries=8)
    rng = random.Random(1000 * k + 10 * b + f)
    for count in (P.n, max(P.n - 1, 1)):
        poly, z = rand_poly(rng, P.r, count), rand_point(rng, P)
        root = M.commit(P, poly)[0]
        proof, values = M.prove(P, [poly], [(0, z)])
        assert values == [M.poly_eval(poly, z, P.r)]
        assert M.verify(P, [root], [(0, z)], values, proof)
        assert M.proof_bytes(proof)[:4] == M.MAGIC


def multi_case(curve, k=4, b=2, f=1, queries=8, seed=5):
    """3 polynomials at 2 points, one point shared: p0 at z0, p1 at z0 and z1, p2 at z1"""
    P = M.Params(curve, k, b, f, queries)
    rng = random.Random(seed)
    polys = [rand_poly(rng, P.r, P.n), rand_poly(rng, P.r, P.n - 3), rand_poly(rng, P.r, 1)]
    z0, z1 = rand_point(rng, P), rand_point(rng, P)
    pairs = [(0, z0), (1, z0), (1, z1), (2, z1)]
    return P, polys, pairs


@pytest.mark.parametrize("curve", CURVES)
def test_multi_opening_verifies(curve):
    P, polys, pairs = multi_case(curve)
    roots = [M.commit(P, p)[0] for p in polys]
    proof, values = M.prove(P, polys, pairs)
    assert values == [M.poly_eval(polys[i], z, P.r) for i, z in pairs]
    assert M.verify(P, roots, pairs, values, proof)
    assert not M.verify(P, roots[::-1], pairs, values, proof)
    assert not M.verify(P, roots, pairs[::-1], values[::-1], proof)


def flip(data, at=0):
    return data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]


def tamperings(P, roots, pairs, values, proof):
    """(name, roots, pairs, values, proof) of every single change that must be refused"""
    def changed(fn):
        p = copy.deepcopy(proof)
        fn(p)
        return p

    def leaf_byte(p):
        polys, layers = p["queries"][0]
        polys[0] = (flip(polys[0][0], 5), polys[0][1])

    def layer_leaf_byte(p):
        polys, layers = p["queries"][1]
        layers[0] = (flip(layers[0][0], 40), layers[0][1])

    def path_byte(p):
        polys, layers = p["queries"][2]
        polys[0] = (polys[0][0], [flip(polys[0][1][0], 63)] + polys[0][1][1:])

    def layer_path_byte(p):
        polys, layers = p["queries"][0]
        layers[0] = (layers[0][0], layers[0][1][:-1] + [flip(layers[0][1][-1])])

    def truncated(p):
        polys, layers = p["queries"][3]
        polys[0] = (polys[0][0], polys[0][1][:-1])

    z = pairs[0][1]
    out = [("leaf byte", roots, pairs, values, changed(leaf_byte)),
           ("path byte", roots, pairs, values, changed(path_byte)),
           ("truncated path", roots, pairs, values, changed(truncated)),
           ("commitment", [flip(roots[0], 7)] + roots[1:], pairs, values, proof),
           ("final coefficient", roots, pairs, values, changed(lambda p: p["final"].__setitem__(0, (p["final"][0] + 1) % P.r))),
           ("final length", roots, pairs, values, changed(lambda p: p["final"].append(0))),
           ("wrong value", roots, pairs, [(values[0] + 1) % P.r] + values[1:], proof),
           ("wrong point", roots, [(pairs[0][0], (z + 1) % P.r)] + pairs[1:], values, proof),
           ("dropped query", roots, pairs, values, changed(lambda p: p["queries"].pop())),
           ("query without polynomials", roots, pairs, values, changed(lambda p: p["queries"].__setitem__(0, ([], p["queries"][0][1])))),
           ("queries not a list", roots, pairs, values, changed(lambda p: p.__setitem__("queries", None)))]
    if proof["roots"]:
        out += [("layer root", roots, pairs, values, changed(lambda p: p["roots"].__setitem__(0, flip(p["roots"][0], 1)))),
                ("layer leaf byte", roots, pairs, values, changed(layer_leaf_byte)),
                ("layer path byte", roots, pairs, values, changed(layer_path_byte)),
                ("dropped root", roots, pairs, values, changed(lambda p: p["roots"].pop()))]
    return out


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("k,b,f", [(1, 1, 0), (3, 2, 1), (6, 2, 2)])
def test_every_single_tampering_is_refused(curve, k, b, f):
    P = M.Params(curve, k, b, f, queries=6)
    rng = random.Random(77 + k)
    poly, z = rand_poly(rng, P.r, P.n), rand_point(rng, P)
    roots, pairs = [M.commit(P, poly)[0]], [(0, z)]
    proof, values = M.prove(P, [poly], pairs)
    assert M.verify(P, roots, pairs, values, proof)
    for name, *case in tamperings(P, roots, pairs, values, proof):
        assert M.verify(P, *case) is False, name


@pytest.mark.parametrize("curve", CURVES)
def test_a_point_of_the_domain_is_refused(curve):
    P = M.Params(curve, 3, 2, 1, queries=4)
    x = P.g * pow(P.w0, 5, P.r) % P.r
    with pytest.raises(ValueError):
        M.prove(P, [[1, 2, 3]], [(0, x)])
    with pytest.raises(ValueError):
        M.commit(P, [1] * (P.n + 1))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("seed", CHEAT_SEEDS)
def test_cheating_proofs_are_refused(curve, seed):
    """a wrong value claimed, layer 0 built pointwise from it: every query that lands on an inconsistent pair refuses"""
    P = M.Params(curve, 4, 2, 1, queries=16)
    rng = random.Random(seed)
    poly, z = rand_poly(rng, P.r, P.n), rand_point(rng, P)
    root = M.commit(P, poly)[0]
    wrong = (M.poly_eval(poly, z, P.r) + 1 + rng.randrange(P.r - 1)) % P.r
    proof, values = M.prove(P, [poly], [(0, z)], cheat_value={0: wrong})
    assert values == [wrong]
    assert M.verify(P, [root], [(0, z)], values, proof) is False
    honest, true_values = M.prove(P, [poly], [(0, z)])
    assert M.verify(P, [root], [(0, z)], true_values, honest)
    assert M.verify(P, [root], [(0, z)], values, honest) is False


def test_bytes_layout():
    P, polys, pairs = multi_case("BN254", queries=3)
    proof, _ = M.prove(P, polys, pairs)
    raw = M.proof_bytes(proof)
    depth0 = P.k + P.b - 1
    per_query = 3 * (65 + 64 * depth0) + sum(65 + 64 * (depth0 - l) for l in range(1, P.L))
    assert len(raw) == 24 + 64 * (P.L - 1) + 32 * (1 << P.f) + 3 * per_query
    assert raw[4:24] == b"".join(x.to_bytes(4, "big") for x in (P.L - 1, 1 << P.f, 3, 3, P.L - 1))
