"""GPU: the FRI polynomial commitment end to end.  Commitments, values and whole proofs equal the integer model's
(tests/fri_model.py) with ==, the bytes equal the golden file, an oracle is reused without a second extension, the four input
kinds agree, and at 2^16 coefficients the proof verifies, a wrong value does not, and the root is hashlib's over the downloaded
pair-order evaluations.

One run above the capped grid of 2^18 threads is tied to the CPU oracle: 2^18 uniform coefficients at blowup 4, 64 queries and 16
final coefficients, the benchmark's shape at the smallest size (N = 2^20) at which both the scale pass and the permutation of
the extension take a second item per thread.  The committed evaluations equal, in whole, the oracle's transform of c[i] g^i
(tests/test_gpu_fri_kernels.py builds it, spot-checked by Horner's rule), the root is hashlib's over those 2^19 leaves, the
opened value is Horner's, and the host verifier accepts the proof and refuses a changed value, another polynomial's root and a
flipped byte in the first queried leaf; the folds from 2^20 values down to 64 and the final coefficients so run on layers
derived from checked data."""

import hashlib
import json
import os
import random

import numpy as np
import pytest

import fri_model as M
import merkle_model
from test_fri_model import multi_case, rand_point, rand_poly
from test_gpu_fri_kernels import lde_reference
from zksnake_amd import _native as N
from zksnake_amd.commitment.polynomial import FRI, FriOracle, FriProof, MultiOpeningQuery
from zksnake_amd.frvec import DevVec, FrOps
from zksnake_amd.polynomial import Polynomial

pytestmark = pytest.mark.gpu

CURVES = ["BN254", "BLS12_381"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fri_vectors.json")


def scheme_of(P):
    fri = FRI(P.n, P.curve, blowup=1 << P.b, queries=P.queries, final=1 << P.f)
    fri.setup()
    return fri


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("k", [1, 3, 6, 10])
def test_commit_and_open_equal_the_model(gpu, curve, k, b):
    P = M.Params(curve, k, b, min(k - 1, 2), queries=8)
    fri = scheme_of(P)
    rng = random.Random(100 * k + b)
    for count in (P.n, max(P.n - 3, 1)):
        poly, z = rand_poly(rng, P.r, count), rand_point(rng, P)
        root = M.commit(P, poly)[0]
        want, values = M.prove(P, [poly], [(0, z)])
        assert fri.commit(poly) == root
        proof, value = fri.open(poly, z)
        assert value == values[0] and isinstance(proof, FriProof)
        assert proof == FriProof(**want) and proof.to_bytes() == M.proof_bytes(want)
        assert M.verify(P, [root], [(0, z)], [value], {"roots": proof.roots, "final": proof.final, "queries": proof.queries})
        assert fri.verify(root, proof, z, value) and not fri.verify(root, proof, z, (value + 1) % P.r)


@pytest.mark.parametrize("curve", CURVES)
def test_multi_open_equals_the_model(gpu, curve):
    """3 polynomials (one a constant) at 2 points with a shared point; one of them handed in as an oracle"""
    P, polys, pairs = multi_case(curve)
    fri = scheme_of(P)
    roots = [M.commit(P, p)[0] for p in polys]
    want, values = M.prove(P, polys, pairs)
    held = fri.oracle(polys[1])
    objs = [polys[0], held, polys[2]]
    query = MultiOpeningQuery()
    for obj, root in zip(objs, roots):
        query.add_polynomial(obj, root)
    for i, z in pairs:
        query.prover_query(objs[i], z)
    proof, verifier_query = fri.multi_open(query)
    assert proof == FriProof(**want)
    assert [query.evaluations[z][i] for i, z in pairs] == values
    assert verifier_query.commitments == roots and held.tree is not None and held.root == roots[1]
    assert fri.multi_verify(verifier_query, proof)
    assert fri.multi_verify(verifier_query, FriProof.from_bytes(proof.to_bytes()))
    verifier_query.evaluations[pairs[2][1]][1] = (values[2] + 1) % P.r
    assert not fri.multi_verify(verifier_query, proof)
    held.release()
    with pytest.raises(ValueError):
        fri.open(held, 3)


def test_bytes_equal_the_golden_file(gpu):
    with open(GOLDEN) as f:
        golden = json.load(f)
    for curve, g in golden.items():
        P = M.Params(curve, g["k"], g["b"], g["f"], g["queries"])
        fri = scheme_of(P)
        poly, z = M.golden_poly(P.r, g["coefficients"], g["seed"]), int(g["point"], 16)
        proof, value = fri.open(poly, z)
        assert (fri.commit(poly).hex(), f"{value:x}", proof.to_bytes().hex()) == (g["root"], g["value"], g["proof"])


@pytest.mark.parametrize("curve", CURVES)
def test_an_oracle_is_reused_and_the_four_input_kinds_agree(gpu, curve):
    P = M.Params(curve, 8, 2, 2, queries=8)
    fri, r, ops = scheme_of(P), P.r, FrOps(P.r)
    poly = rand_poly(random.Random(7), r, 200)
    z = 0xABCDEF
    want = fri.commit(poly), fri.open(poly, z)
    oracle = fri.oracle(poly)
    assert isinstance(oracle, FriOracle) and oracle.root == want[0] and fri.oracle(oracle) is oracle
    assert fri.commit(oracle) == want[0] and (fri.open(oracle, z), fri.open(oracle, z + 1)[1]) == (want[1], M.poly_eval(poly, z + 1, r))
    assert oracle.tree is not None and oracle.evals.n == P.N and oracle.coeffs.n == 200      # still resident after three uses
    assert M.natural_order(ops.ints(oracle.evals.download())) == M.natural_order(M.lde(P, poly))
    oracle.release()
    limbs = N.ints_to_limbs([x + r if i % 3 == 0 and x + r < 1 << 256 else x for i, x in enumerate(poly)], 4)   # canonicalised on upload
    vec = ops.d_from(ops.limbs(poly))
    assert isinstance(vec, DevVec)
    before, limbs_before = vec.download(), limbs.copy()
    for kind in (Polynomial(poly, r), limbs, vec, tuple(poly)):
        assert fri.commit(kind) == want[0] and fri.open(kind, z) == want[1]
    assert (vec.download() == before).all() and (limbs == limbs_before).all()      # the caller's data is never modified


@pytest.mark.parametrize("curve", CURVES)
def test_two_to_the_sixteen(gpu, curve):
    """defaults (blowup 4, 64 queries, 16 final coefficients) at 2^16 coefficients: no model at this size, so the proof is checked
    by the host verifier, and the commitment by hashlib over the downloaded evaluations"""
    fri = FRI(1 << 16, curve)
    fri.setup()
    r, ops = fri.order, FrOps(fri.order)
    limbs = ops.random_vector(1 << 16)
    vec = ops.d_from(limbs)
    z = 0x1234567
    oracle = fri.oracle(vec)
    proof, value = fri.open(oracle, z)
    assert value == ops.eval(limbs, z)
    assert len(proof.roots) == 11 and len(proof.final) == 16 and len(proof.queries) == 64
    assert fri.verify(oracle.root, proof, z, value)
    assert not fri.verify(oracle.root, proof, z, (value + 1) % r)
    assert not fri.verify(oracle.root, proof, z + 1, value)
    level = [hashlib.blake2b(row.tobytes()).digest() for row in oracle.evals.download().reshape(-1, 8)]
    assert len(level) == fri.size // 2
    while len(level) > 1:
        level = [hashlib.blake2b(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
    assert level[0] == oracle.root == fri.commit(vec)
    oracle.release()


@pytest.mark.parametrize("curve", CURVES)
def test_above_one_grid_against_the_oracle(gpu, curve):
    """the benchmark's shape at 2^18 coefficients: N = 2^20, see the module docstring"""
    fri = FRI(1 << 18, curve, blowup=4, queries=64, final=16)
    fri.setup()
    r = fri.order
    ref = lde_reference(curve, "commit-2^20")
    assert ref.size == fri.size == 1 << 20 and ref.shift == fri.shift and len(ref.coeffs) == fri.n
    oracle = fri.oracle(ref.limbs)
    assert (oracle.evals.download() == ref.pairs).all(), "the committed evaluations differ from the oracle's transform"
    leaves = [hashlib.blake2b(ref.pairs[j:j + 2].tobytes()).digest() for j in range(0, fri.size, 2)]
    assert len(leaves) == 1 << 19 and oracle.root == merkle_model.levels(leaves)[-1][0]
    z = 0x1234567
    assert not fri._in_domain(z)
    proof, value = fri.open(oracle, z)
    assert value == M.poly_eval(ref.coeffs, z, r)
    assert len(proof.roots) == 13 and len(proof.final) == 16 and len(proof.queries) == 64
    assert fri.verify(oracle.root, proof, z, value)
    assert not fri.verify(oracle.root, proof, z, (value + 1) % r)
    second = ref.limbs.copy()
    second[5] = ref.limbs[6]
    other_root = fri.commit(second)
    assert other_root != oracle.root and not fri.verify(other_root, proof, z, value)
    bad = FriProof.from_bytes(proof.to_bytes())
    assert bad == proof and fri.verify(oracle.root, bad, z, value)
    leaf, path = bad.queries[0][0][0]
    bad.queries[0][0][0] = (bytes([leaf[0] ^ 1]) + leaf[1:], path)
    assert not fri.verify(oracle.root, bad, z, value)
    oracle.release()


def test_arguments(gpu):
    fri = FRI(8, "BN254", blowup=2, queries=4, final=2)
    ops = FrOps(fri.order)
    inside = fri.shift * pow(fri._omega0(), 5, fri.order) % fri.order
    for too_long in ([1] * 9, ops.d_from(ops.limbs([1] * 9)), np.ones((9, 4), dtype=np.uint64), Polynomial([1] * 9, fri.order)):
        with pytest.raises(ValueError):
            fri.commit(too_long)
        with pytest.raises(ValueError):
            fri.open(too_long, 3)
    with pytest.raises(ValueError):
        fri.open([1, 2, 3], inside)
    assert fri.commit([]) == fri.commit([0]) == fri.commit([0] * 8)
    proof, value = fri.open([], 11)
    assert value == 0 and fri.verify(fri.commit([]), proof, 11, 0)
    proof, value = fri.open([9], 11)
    assert value == 9 and fri.verify(fri.commit([9]), proof, 11, 9) and not fri.verify(fri.commit([9]), proof, 11, 8)
