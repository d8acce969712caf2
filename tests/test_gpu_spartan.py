"""GPU: the Spartan prover and verifier (zksnake_amd/spartan) against the integer model (tests/spartan_model.py) with the
transcript's own challenges replayed into the model, on circom fixtures, past one grid, under tampering, on an unsatisfied
witness, on a round polynomial that is identically zero, and twice on one object.  Every comparison is == on integers, bytes or
points."""

import copy
import os
import random

import pytest

import spartan_model as S
from helpers import CURVES
from zksnake_amd import frvec, workloads
from zksnake_amd.arithmetization import R1CS
from zksnake_amd.arithmetization.r1cs import Var
from zksnake_amd.ecc import EllipticCurve
from zksnake_amd.spartan import Spartan, SpartanProof

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDS = [c[0] for c in CURVES]


@pytest.fixture(scope="module", autouse=True)
def _drop_the_pool():
    yield
    frvec.release_pool()


def unzip(triplets):
    return tuple(list(t) for t in zip(*triplets)) if triplets else ([], [], [])


def build(inst, curve):
    r1cs = R1CS.from_triplets(unzip(inst["A"]), unzip(inst["B"]), unzip(inst["C"]), inst["n_row"], inst["n_col"], inst["n_public"], curve)
    return Spartan(r1cs)


def chain(n, curve):
    p = EllipticCurve(curve).order
    A, B, C, w, n_col = workloads.chain_circuit(n, p)
    inst = {"A": list(zip(*A)), "B": list(zip(*B)), "C": list(zip(*C)), "n_row": n, "n_col": n_col, "n_public": 2, "p": p}
    return inst, w[:2], w[2:]


def hand_circuit(p, x=3):
    """wires [1, out, x, y, z]: x x = y, y x = z, (z + x + 5) 1 = out"""
    y, z = x * x % p, x * x * x % p
    inst = {"A": [(0, 2, 1), (1, 3, 1), (2, 4, 1), (2, 2, 1), (2, 0, 5)], "B": [(0, 2, 1), (1, 2, 1), (2, 0, 1)],
            "C": [(0, 3, 1), (1, 4, 1), (2, 1, 1)], "n_row": 3, "n_col": 5, "n_public": 2, "p": p}
    return inst, [1, (z + x + 5) % p], [x, y, z]


def against_the_model(inst, public, private, curve, seed):
    """prove on the device, replay the challenges, and hold every message to the model's"""
    E = EllipticCurve(curve)
    p, G = E.order, E.G1()
    assert inst["p"] == p and S.satisfied(inst, public, private)
    sp = build(inst, curve)
    try:
        s_x, h, s = S.sizes(inst)
        assert (sp.s_x, sp.h, sp.s) == (s_x, h, s)
        kzg_tau = [random.Random(seed + k).randrange(1, p) for k in range(h)]
        sp.setup(tau=kzg_tau)
        proof = sp.prove(public, private)
        tau, rx, r_abc, ry = sp.challenges(proof, public)
        ch = {"tau": tau, "rx": rx, "r_abc": r_abc, "ry": ry}
        assert (len(tau), len(rx), len(ry)) == (s_x, s_x, s)
        want = S.prove_linear(inst, public, private, ch, kzg_tau)
        assert proof.outer == want["outer"] and proof.evals == want["evals"] and proof.inner == want["inner"] and proof.v_w == want["v_w"]
        assert proof.commitment == G * want["commitment"]
        assert len(proof.opening) == h and all(q == G * w for q, w in zip(proof.opening, want["opening"]))
        assert S.verify(inst, public, want, ch, kzg_tau)
        assert sp.verify(proof, public)
        data = proof.to_bytes()
        assert len(data) == SpartanProof.size(s_x, s, curve) and sp.verify(SpartanProof.from_bytes(data, curve), public)
        return sp.digest
    finally:
        sp.release()


@pytest.mark.parametrize("name,cid", CURVES, ids=IDS)
def test_hand_written_circuit_equals_the_model(gpu, name, cid):
    p = EllipticCurve(name).order
    against_the_model(*hand_circuit(p), name, 1)
    against_the_model(*hand_circuit(p, x=p - 2), name, 2)


@pytest.mark.parametrize("n", (2, 5, 300, 4200))     # 300: column 2 of B is a long sub-segment; 4200: it takes two work items
@pytest.mark.parametrize("name,cid", CURVES, ids=IDS)
def test_chain_circuit_equals_the_model(gpu, name, cid, n):
    against_the_model(*chain(n, name), name, n)


@pytest.mark.parametrize("name,cid", CURVES, ids=IDS)
def test_more_public_than_private_wires(gpu, name, cid):
    p = EllipticCurve(name).order
    inst, public, private = S.random_instance(random.Random(3 + cid), p, 5, 7, 5)
    assert S.sizes(inst) == (3, 3, 4)
    against_the_model(inst, public, private, name, 3)
    inst, public, private = S.random_instance(random.Random(4 + cid), p, 1, 2, 1)     # one constraint, one private wire
    against_the_model(inst, public, private, name, 4)


def from_file(r1cs):
    return {"A": r1cs.A.triplets, "B": r1cs.B.triplets, "C": r1cs.C.triplets, "n_row": r1cs.A.n_row, "n_col": r1cs.A.n_col,
            "n_public": r1cs.n_public, "p": r1cs.p}


def test_circom_poseidon_fixture(gpu):
    r1cs = R1CS.from_file(os.path.join(GOLD, "test_poseidon.r1cs"), os.path.join(GOLD, "test_poseidon.sym"))
    public, private = r1cs.generate_witness(r1cs.solve({"main.a": 1, "main.b": 2, "main.c": 3}))
    against_the_model(from_file(r1cs), public, private, "BN254", 5)


def test_circom_num2bits_fixture(gpu):
    r1cs = R1CS.from_file(os.path.join(GOLD, "num2bits.r1cs"), os.path.join(GOLD, "num2bits.sym"))
    for i in range(256):
        r1cs.constraint_system.unsafe_assign(Var(f"main.out[{i}]"), (lambda i: lambda **k: (k["main.in"] >> i) & 1)(i), ("main.in",))
    public, private = r1cs.generate_witness(r1cs.constraint_system.solve({"main.in": 0xDEADF00D}))
    against_the_model(from_file(r1cs), public, private, "BN254", 6)


def test_past_one_grid(gpu):
    """2^18 + 300 constraints: the lane-per-segment kernels stride, column 2 of B is 65 work items.  No model at this size: the
    proof round-trips through bytes and verifies, and a moved public input does not."""
    n = (1 << 18) + 300
    inst, public, private = chain(n, "BN254")
    sp = build(inst, "BN254")
    try:
        assert (sp.s_x, sp.h, sp.s) == (19, 19, 20) and sp._cols.n_long >= 1 and sp._cols.n_items >= 65
        sp.setup()
        proof = sp.prove(public, private)
        data = proof.to_bytes()
        back = SpartanProof.from_bytes(data, "BN254")
        assert back.to_bytes() == data and sp.verify(back, public)
        assert not sp.verify(back, [public[0], (public[1] + 1) % inst["p"]])
    finally:
        sp.release()


def tampered(proof, G, p):
    """(name, copy of the proof with one field moved)"""
    def clone():
        return SpartanProof(proof.commitment, copy.deepcopy(proof.outer), proof.evals, copy.deepcopy(proof.inner), proof.v_w,
                            list(proof.opening), proof.curve)
    for key in ("outer", "inner"):
        for j, coeffs in enumerate(getattr(proof, key)):
            for i in range(len(coeffs)):
                t = clone()
                getattr(t, key)[j][i] = (coeffs[i] + 1) % p
                yield f"{key}[{j}][{i}]", t
    for i in range(3):
        t = clone()
        t.evals = tuple((v + (k == i)) % p for k, v in enumerate(proof.evals))
        yield f"evals[{i}]", t
    t = clone()
    t.v_w = (proof.v_w + 1) % p
    yield "v_w", t
    t = clone()
    t.commitment = proof.commitment + G
    yield "C_w", t
    for k in range(len(proof.opening)):
        t = clone()
        t.opening[k] = proof.opening[k] + G
        yield f"opening[{k}]", t


@pytest.mark.parametrize("name,cid", CURVES, ids=IDS)
def test_tampering_is_refused_without_raising(gpu, name, cid):
    E = EllipticCurve(name)
    p, G = E.order, E.G1()
    inst, public, private = hand_circuit(p)
    sp = build(inst, name)
    other_inst = copy.deepcopy(inst)
    other_inst["A"][-1] = (2, 0, 6)                     # (z + x + 6) 1 = out: the same shape, another circuit
    other = build(other_inst, name)
    try:
        sp.setup(tau=[11, 12])
        other.setup(tau=[11, 12])                       # the same SRS: it does not depend on the circuit
        proof = sp.prove(public, private)
        assert sp.verify(proof, public)
        count = 0
        for what, bad in tampered(proof, G, p):
            assert sp.verify(bad, public) is False, what
            count += 1
        assert count == 4 * sp.s_x + 3 * sp.s + 3 + 1 + 1 + sp.h
        for j in range(2):
            assert sp.verify(proof, [(v + (k == j)) % p for k, v in enumerate(public)]) is False
        theirs = other.prove([1, (public[1] + 1) % p], private)
        assert other.digest != sp.digest and other.verify(theirs, [1, (public[1] + 1) % p])
        assert sp.verify(theirs, [1, (public[1] + 1) % p]) is False and sp.verify(theirs, public) is False
        assert other.verify(proof, public) is False
        # malformed but well-typed
        for bad in (SpartanProof(proof.commitment, proof.outer[:-1], proof.evals, proof.inner, proof.v_w, proof.opening, name),
                    SpartanProof(proof.commitment, proof.outer, proof.evals, proof.inner + [[0, 0, 0]], proof.v_w, proof.opening, name),
                    SpartanProof(proof.commitment, [c[:3] for c in proof.outer], proof.evals, proof.inner, proof.v_w, proof.opening, name),
                    SpartanProof(proof.commitment, proof.outer, proof.evals[:2], proof.inner, proof.v_w, proof.opening, name),
                    SpartanProof(proof.commitment, proof.outer, proof.evals, proof.inner, p, proof.opening, name),
                    SpartanProof(proof.commitment, proof.outer, proof.evals, proof.inner, proof.v_w, proof.opening[:-1], name),
                    SpartanProof(None, proof.outer, proof.evals, proof.inner, proof.v_w, proof.opening, name)):
            assert sp.verify(bad, public) is False
        assert sp.verify(proof, public + [0]) is False and sp.verify(None, public) is False
    finally:
        other.release()
        sp.release()


@pytest.mark.parametrize("name,cid", CURVES, ids=IDS)
def test_unsatisfied_witness_raises(gpu, name, cid):
    p = EllipticCurve(name).order
    for inst, public, private in (hand_circuit(p), chain(300, name)):
        sp = build(inst, name)
        try:
            sp.setup()
            for k in (0, len(private) - 1):
                wrong = list(private)
                wrong[k] = (wrong[k] + 1) % p
                with pytest.raises(ValueError, match="witness does not satisfy the R1CS"):
                    sp.prove(public, wrong)
            with pytest.raises(ValueError):
                sp.prove(public, private[:-1])
            with pytest.raises(ValueError):
                sp.prove(public + [0], private)
            assert sp.verify(sp.prove(public, private), public)
        finally:
            sp.release()


@pytest.mark.parametrize("name,cid", CURVES, ids=IDS)
def test_identically_zero_round(gpu, name, cid):
    """Az is constant over variable 0 (constraints 2 t and 2 t + 1 have the same A row), so the first outer round polynomial is
    the zero polynomial: four zero coefficients on the transcript, no exception, and the proof verifies"""
    p = EllipticCurve(name).order
    x = 5
    y, z = x * x % p, x * x * x % p
    # wires [1, out, x, y, z, t]: x x = y, x y = z, z x = t, z z = out
    four = {"A": [(0, 2, 1), (1, 2, 1), (2, 4, 1), (3, 4, 1)], "B": [(0, 2, 1), (1, 3, 1), (2, 2, 1), (3, 4, 1)],
            "C": [(0, 3, 1), (1, 4, 1), (2, 5, 1), (3, 1, 1)], "n_row": 4, "n_col": 6, "n_public": 2, "p": p}
    two = {"A": four["A"][:2], "B": four["B"][:2], "C": [(0, 3, 1), (1, 1, 1)], "n_row": 2, "n_col": 4, "n_public": 2, "p": p}
    for inst, public, private in ((four, [1, z * z % p], [x, y, z, z * x % p]), (two, [1, z], [x, y])):
        sp = build(inst, name)
        try:
            sp.setup(tau=list(range(21, 21 + sp.h)))
            proof = sp.prove(public, private)
            assert proof.outer[0] == [0, 0, 0, 0] and sp.verify(proof, public)
            assert inst is two or any(proof.outer[1])
        finally:
            sp.release()
        against_the_model(inst, public, private, name, 7)


@pytest.mark.parametrize("name,cid", CURVES, ids=IDS)
def test_no_state_is_carried_over(gpu, name, cid):
    inst, public, private = chain(300, name)
    p = inst["p"]
    sp = build(inst, name)
    sp.setup(tau=[31 + k for k in range(sp.h)])
    first = sp.prove(public, private).to_bytes()
    with pytest.raises(ValueError):
        sp.prove(public, [(private[0] + 1) % p] + private[1:])        # a failed call in between leaves nothing behind
    assert sp.verify(SpartanProof.from_bytes(first, name), public)
    assert sp.prove(public, private).to_bytes() == first
    sp.release()
    with pytest.raises(RuntimeError):
        sp.prove(public, private)
    with pytest.raises(RuntimeError):
        sp.verify(SpartanProof.from_bytes(first, name), public)
    sp.release()                                                      # a second release is a no-op
