"""CPU: what of the FRI polynomial commitment needs no GPU -- the verifier against the integer model's proofs (with the device
made unreachable), the argument rules, the bindings, the serialisation and its golden bytes, and the host side of csrc/fri.hip
under sanitizers."""

import copy
import json
import os
import random
import re

import pytest

import fri_model as M
from test_fri_model import multi_case, rand_point, rand_poly, tamperings
from helpers import run_host_program
from zksnake_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("zk_fri_lde_dev", "zk_fri_fold_dev", "zk_fri_rows_dev")
CURVES = ["BN254", "BLS12_381"]
GOLDEN = os.path.join(ROOT, "tests", "golden", "fri_vectors.json")


@pytest.fixture
def no_gpu(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(N, "ensure_gpu", refuse)


def scheme_of(P):
    from zksnake_amd.commitment.polynomial import FRI
    return FRI(P.n, P.curve, blowup=1 << P.b, queries=P.queries, final=1 << P.f)


def as_proof(model_proof):
    from zksnake_amd.commitment.polynomial import FriProof
    return FriProof(**copy.deepcopy(model_proof))


def test_fri_host_side_refuses_bad_arguments_under_sanitizers(tmp_path):
    """tests/native/fri_args_check.cpp, built by the recipe in its header (helpers.run_host_program, as tests/test_merkle_host.py
    builds merkle_args_check): a host-only compile, an EMPTY offload bundle for the __hip_fatbin_<hash> symbol the object refers to, link,
    run.  The sanitizer runtimes are linked into the program; nothing is loaded into Python.  The program sees no device on any
    machine, so the calls that pass the checks fail in the launch with ZK_ERR_HIP, which is what it expects."""
    res = run_host_program("fri_args_check", tmp_path)
    assert res.returncode == 0 and "fri_args_check: all ok" in res.stdout, res.stdout + res.stderr


def test_symbols_are_bound(lib):
    for name in SYMBOLS:
        assert name in N.SIGNATURES and hasattr(lib, name)
    with open(os.path.join(ROOT, "include", "zkmi.h")) as f:
        header = f.read()
    assert re.search(rf"#define ZK_FRI_MAX_LOG {N.FRI_MAX_LOG}\s", header)
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header)


def test_parameters_follow_the_model():
    from zksnake_amd.commitment.polynomial import FRI, PolynomialCommitmentScheme
    from zksnake_amd.commitment.polynomial.fri import COSET_SHIFT
    for curve in CURVES:
        P = M.Params(curve, 5, 2, 1, 7)
        scheme = scheme_of(P)
        assert isinstance(scheme, PolynomialCommitmentScheme) and not scheme.is_setup
        assert scheme.setup() is None and scheme.is_setup
        assert (scheme.order, scheme.shift, scheme._omega0(), scheme._header()) == (P.r, P.g, P.w0, P.header())
        assert COSET_SHIFT[P.cid] == P.g
        with pytest.raises(NotImplementedError):
            scheme.zero_commitment()
    default = FRI(1 << 10)
    assert (default.group, default.b, default.queries, default.f) == ("BN254", 2, 64, 4)


def test_constructor_and_arguments_are_refused_before_any_device_call(no_gpu):
    from zksnake_amd.commitment.polynomial import FRI, MultiOpeningQuery
    from zksnake_amd.commitment.polynomial.fri import FriOracle
    for args, kw in [((0,), {}), ((3,), {}), ((-4,), {}), ((1,), {"final": 1}), ((1 << 27,), {}), ((1 << 25,), {"blowup": 4}),
                     ((16,), {"blowup": 1}), ((16,), {"blowup": 3}), ((16,), {"blowup": 0}), ((16,), {"final": 16}), ((16,), {"final": 32}),
                     ((16,), {"final": 0}), ((16,), {"final": 3}), ((16,), {"queries": 0}), ((16,), {"queries": (1 << 16) + 1}),
                     ((16, "secp256k1"), {}), ((8,), {})]:
        with pytest.raises(ValueError):
            FRI(*args, **kw)
    with pytest.raises(TypeError):
        FRI(16.0)
    scheme = FRI(8, "BN254", blowup=2, queries=4, final=2)
    assert FRI(1 << 24, blowup=4).size == 1 << 26 and FRI(2, blowup=2, final=1).folds == 1
    inside = scheme.shift * pow(scheme._omega0(), 3, scheme.order) % scheme.order
    for z in (inside, inside + scheme.order, scheme.shift):
        with pytest.raises(ValueError):
            scheme.open([1, 2, 3], z)
    for too_long in ([1] * 9, tuple(range(20))):
        with pytest.raises(ValueError):
            scheme.commit(too_long)
        with pytest.raises(ValueError):
            scheme.open(too_long, 3)
    query = MultiOpeningQuery()
    query.prover_query([1, 2, 3], 11)
    query.prover_query([1, 2, 3, 4], inside)
    with pytest.raises(ValueError):
        scheme.multi_open(query)
    with pytest.raises(ValueError):
        scheme.oracle(FriOracle((0, 4, 1), None, None, type("T", (), {"root": b"", "release": lambda self: None})()))
    with pytest.raises(AssertionError, match="a device call"):
        scheme.commit([1, 2, 3])


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("k,b,f", [(1, 1, 0), (3, 2, 1), (6, 2, 2)])
def test_verify_accepts_the_models_proofs_and_refuses_tampered_ones(no_gpu, curve, k, b, f):
    P = M.Params(curve, k, b, f, queries=6)
    scheme = scheme_of(P)
    rng = random.Random(77 + k)
    poly, z = rand_poly(rng, P.r, P.n), rand_point(rng, P)
    roots, pairs = [M.commit(P, poly)[0]], [(0, z)]
    proof, values = M.prove(P, [poly], pairs)
    assert scheme.verify(roots[0], as_proof(proof), z, values[0]) is True
    assert scheme.verify(roots[0], as_proof(proof), z + P.r, values[0] + P.r) is True
    for name, t_roots, t_pairs, t_values, t_proof in tamperings(P, roots, pairs, values, proof):
        assert scheme.verify(t_roots[0], as_proof(t_proof), t_pairs[0][1], t_values[0]) is False, name
    for junk in (None, b"", 5, [], proof):
        assert scheme.verify(roots[0], junk, z, values[0]) is False
    other = scheme_of(M.Params(curve, k, b, f, queries=5))
    assert other.verify(roots[0], as_proof(proof), z, values[0]) is False


@pytest.mark.parametrize("curve", CURVES)
def test_multi_verify_accepts_the_models_multi_opening(no_gpu, curve):
    from zksnake_amd.commitment.polynomial import MultiOpeningQuery
    P, polys, pairs = multi_case(curve)
    scheme = scheme_of(P)
    roots = [M.commit(P, p)[0] for p in polys]
    proof, values = M.prove(P, polys, pairs)

    def query_of(values, roots=roots):
        query = MultiOpeningQuery()
        for (i, z), v in zip(pairs, values):
            query.verifier_query(bytes(roots[i]), z, v)   # equal bytes, not the same object
        return query

    query = query_of(values)
    assert query.commitments == roots
    assert scheme.multi_verify(query, as_proof(proof)) is True
    for at in range(len(pairs)):
        wrong = list(values)
        wrong[at] = (wrong[at] + 1) % P.r
        assert scheme.multi_verify(query_of(wrong), as_proof(proof)) is False
    assert scheme.multi_verify(query_of(values, roots[::-1]), as_proof(proof)) is False
    assert scheme.multi_verify(query_of(values[:-1] + [None]), as_proof(proof)) is False
    assert scheme.multi_verify(MultiOpeningQuery(), as_proof(proof)) is False
    # the caller's transcript: prover and verifier must have fed it the same bytes
    from zksnake_amd.transcript import FiatShamirTranscript
    mt = M.Transcript(P.r)
    mt.append(b"context")
    proof2, values2 = M.prove(P, polys, pairs, transcript=mt)
    vt = FiatShamirTranscript(field=P.r)
    vt.append(b"context")
    assert scheme.multi_verify(query_of(values2), as_proof(proof2), vt) is True
    assert scheme.multi_verify(query_of(values2), as_proof(proof2)) is False


@pytest.mark.parametrize("curve", CURVES)
def test_cheating_proofs_are_refused(no_gpu, curve):
    from test_fri_model import CHEAT_SEEDS
    P = M.Params(curve, 4, 2, 1, queries=16)
    scheme = scheme_of(P)
    for seed in CHEAT_SEEDS:
        rng = random.Random(seed)
        poly, z = rand_poly(rng, P.r, P.n), rand_point(rng, P)
        root = M.commit(P, poly)[0]
        wrong = (M.poly_eval(poly, z, P.r) + 1 + rng.randrange(P.r - 1)) % P.r
        proof, values = M.prove(P, [poly], [(0, z)], cheat_value={0: wrong})
        assert scheme.verify(root, as_proof(proof), z, wrong) is False


def test_bytes_round_trip_and_equality():
    from zksnake_amd.commitment.polynomial import FriProof
    for curve in CURVES:
        for queries in (1, 3):
            P, polys, pairs = multi_case(curve, queries=queries)
            model_proof, _ = M.prove(P, polys, pairs)
            proof = as_proof(model_proof)
            raw = proof.to_bytes()
            assert raw == M.proof_bytes(model_proof)
            back = FriProof.from_bytes(raw)
            assert back == proof and back.to_bytes() == raw and not (back != proof)
            changed = as_proof(model_proof)
            changed.final[0] ^= 1
            assert changed != proof and proof != "proof"
            for bad in (raw[:-1], raw + b"\0", b"FRI2" + raw[4:], raw[:20], b""):
                with pytest.raises(ValueError):
                    FriProof.from_bytes(bad)
    P = M.Params("BN254", 1, 1, 0, 2)
    model_proof, _ = M.prove(P, [[3, 4]], [(0, 9)])   # no committed layer: a query's second part is empty
    assert FriProof.from_bytes(M.proof_bytes(model_proof)) == as_proof(model_proof)
    assert FriProof.from_bytes(FriProof([], [], []).to_bytes()) == FriProof([], [], [])


def test_golden_bytes(no_gpu):
    """tests/golden/fri_vectors.json (written by tests/golden/gen_fri_golden.py from the model) pins the proof bytes"""
    from zksnake_amd.commitment.polynomial import FriProof
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(CURVES)
    for curve, g in golden.items():
        P = M.Params(curve, g["k"], g["b"], g["f"], g["queries"])
        poly = M.golden_poly(P.r, g["coefficients"], g["seed"])
        z = int(g["point"], 16)
        root = M.commit(P, poly)[0]
        proof, values = M.prove(P, [poly], [(0, z)])
        assert (root.hex(), f"{values[0]:x}", M.proof_bytes(proof).hex()) == (g["root"], g["value"], g["proof"])
        assert scheme_of(P).verify(root, FriProof.from_bytes(bytes.fromhex(g["proof"])), z, values[0]) is True
