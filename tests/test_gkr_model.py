"""CPU: the GKR integer model (tests/gkr_model.py) held to itself, and the host side of LayeredCircuit.

The bookkeeping tables, which the GPU kernels are compared with, must say what the dense definition says: phase 1's
P W + Q has the dense polynomial's sum and its round sums at every b-round, and phase 2's polynomial in c IS the dense
polynomial with b fixed to u.  The model's verifier accepts the model's proofs and rejects every single-field tampering."""

import copy
import random

import numpy as np
import pytest

import gkr_model as G
import mle_model as M
from zksnake_amd.arithmetization import LayeredCircuit
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD

FIELDS = (("BN254", BN254_SCALAR_FIELD), ("BLS12_381", BLS12_381_SCALAR_FIELD))
PHASE1_TERMS = [(1, (0, 1)), (1, (2,))]


def _layer(rnd, n_prev, n, p):
    gates = [(rnd.randrange(2), rnd.randrange(n_prev), rnd.randrange(n_prev)) for _ in range(n)]
    w = [rnd.randrange(1, p) for _ in range(n_prev)]
    w[0], w[-1] = 0, p - 1
    k, k_prev = G.num_vars(n), G.num_vars(n_prev)
    return gates, G.pad(w, k_prev), [rnd.randrange(p) for _ in range(k)], k_prev


@pytest.mark.parametrize("n_prev,n", [(2, 1), (3, 5), (8, 8), (17, 5), (5, 17)])
@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_phase_tables_say_what_the_dense_tables_say(name, p, n_prev, n):
    rnd = random.Random(1000 * n_prev + n)
    gates, w, r, k = _layer(rnd, n_prev, n, p)
    e = G.eq_table(r, p)
    assert sum(e) % p == 1
    dense = G.dense_tables(gates, k, w, r, p)
    p_tab, q_tab = G.phase1_tables(gates, k, w, e, p)
    # the claim: the layer's own extension at r
    outputs = G.pad([(w[b] * w[c] if t else w[b] + w[c]) % p for t, b, c in gates], len(r))
    claim = M.evaluate(outputs, r, p)
    assert sum(pw * x + q for pw, x, q in zip(p_tab, w, q_tab)) % p == claim
    s = M.round_sums(dense, G.DENSE_TERMS, p)
    assert (s[0] + s[1]) % p == claim
    # every b-round: the three small tables and the four dense ones, folded by the same challenges
    u = [rnd.randrange(p) for _ in range(k)]
    small = [p_tab, w, q_tab]
    for i in range(k):
        assert M.round_sums(small, PHASE1_TERMS, p) == M.round_sums(dense, G.DENSE_TERMS, p), i
        small = [M.fix(t, [u[i]], p) for t in small]
        dense = [M.fix(t, [u[i]], p) for t in dense]
    # b = u: what is left of the dense polynomial is phase 2's polynomial, point by point in c
    wu = small[1][0]
    assert wu == M.evaluate(w, u, p)
    a_add, a_mul = G.phase2_tables(gates, k, e, G.eq_table(u, p), p)
    for c in range(1 << k):
        want = (dense[0][c] * (dense[1][c] + dense[2][c]) + dense[3][c] * dense[1][c] * dense[2][c]) % p
        assert (wu * a_add[c] + a_add[c] * w[c] + wu * a_mul[c] * w[c]) % p == want
    v = [rnd.randrange(p) for _ in range(k)]
    assert G.wiring(gates, r, u, v, p) == (M.evaluate(a_add, v, p), M.evaluate(a_mul, v, p))
    assert G.wiring(gates, r, u, v, p) == (M.evaluate(dense[0], v, p), M.evaluate(dense[3], v, p))


def test_line_poly_is_the_table_along_the_line():
    p = BN254_SCALAR_FIELD
    rnd = random.Random(5)
    for k in (1, 2, 4):
        w = [rnd.randrange(p) for _ in range(1 << k)]
        u, v = [rnd.randrange(p) for _ in range(k)], [rnd.randrange(p) for _ in range(k)]
        q = G.line_poly(w, u, v, p)
        assert len(q) <= k + 1
        assert M.poly_at(q, 0, p) == M.evaluate(w, u, p) and M.poly_at(q, 1, p) == M.evaluate(w, v, p)
        t = rnd.randrange(p)
        assert M.poly_at(q, t, p) == M.evaluate(w, G.line_point(u, v, t, p), p)


def _circuits():
    out = [G.named_to_layers(inputs, named) for inputs, named in G.REFERENCE_CIRCUITS]
    rnd = random.Random("gkr model")
    return out + [G.random_circuit(rnd, depth) for depth in (1, 2, 3, 4)]


@pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
def test_the_verifier_accepts_and_rejects_every_single_change(name, p):
    rnd = random.Random(name)
    for n_inputs, layers in _circuits():
        inputs = [rnd.randrange(1, p) for _ in range(n_inputs)]
        outputs, proofs, trace = G.prove(layers, inputs, p)
        assert outputs == G.evaluate_circuit(layers, inputs, p)[-1]
        assert G.verify(n_inputs, layers, inputs, outputs, proofs, p) is True
        for i in range(len(inputs)):
            bad = list(inputs)
            bad[i] = (bad[i] + 1) % p
            assert not G.verify(n_inputs, layers, bad, outputs, proofs, p)
        for i in range(len(outputs)):
            bad = list(outputs)
            bad[i] = (bad[i] + 1) % p
            assert not G.verify(n_inputs, layers, inputs, bad, proofs, p)
        for li, layer_proof in enumerate(proofs):
            for ri, coeffs in enumerate(layer_proof[:-1]):
                for ci in range(len(coeffs)):
                    bad = copy.deepcopy(proofs)
                    bad[li][ri][ci] = (coeffs[ci] + 1) % p
                    assert not G.verify(n_inputs, layers, inputs, outputs, bad, p)
            q, z1, z2 = layer_proof[-1]
            k = (len(layer_proof) - 1) // 2
            changed = [([(c + (i == ci)) % p for i, c in enumerate(q)], z1, z2) for ci in range(len(q))]
            changed += [(q, (z1 + 1) % p, z2), (q, z1, (z2 + 1) % p)]
            changed.append((q + [0] * (k + 1 - len(q)) + [1], z1, (z2 + 1) % p))          # degree k + 1, consistent with z1, z2
            for last in changed:
                bad = copy.deepcopy(proofs)
                bad[li][-1] = last
                assert not G.verify(n_inputs, layers, inputs, outputs, bad, p)
        other = M.Transcript(b"gkr", p)
        other.append(7)
        assert not G.verify(n_inputs, layers, inputs, outputs, proofs, p, other)
        same = [M.Transcript(b"outer", p), M.Transcript(b"outer", p)]
        for tr in same:
            tr.append([3, 4])
        assert G.verify(n_inputs, layers, inputs, outputs, G.prove(layers, inputs, p, same[0])[1], p, same[1])


def test_a_high_degree_q_is_rejected_for_its_degree():
    """q + c t^k (t - 1) keeps q(0) and q(1): only the degree check stands between it and the next layer's claim"""
    p = BN254_SCALAR_FIELD
    n_inputs, layers = G.named_to_layers(*G.REFERENCE_CIRCUITS[0])
    inputs = [5, 11]
    outputs, proofs, _ = G.prove(layers, inputs, p)
    q, z1, z2 = proofs[-1][-1]
    k = 1
    padded = q + [0] * (k + 2 - len(q))
    padded[k] = (padded[k] - 1) % p
    padded[k + 1] = (padded[k + 1] + 1) % p
    assert M.poly_at(padded, 0, p) == z1 and M.poly_at(padded, 1, p) == z2
    bad = copy.deepcopy(proofs)
    bad[-1][-1] = (padded, z1, z2)
    assert not G.verify(n_inputs, layers, inputs, outputs, bad, p)


# ---- LayeredCircuit, host side ----
def _build(inputs, named):
    c = LayeredCircuit(inputs)
    for j, layer in enumerate(named):
        if j:
            c.add_layer()
        for gate in layer:
            c.add_gate(*gate)
    return c


def test_builder_numbering_labels_and_evaluate():
    p = BN254_SCALAR_FIELD
    for inputs, named in G.REFERENCE_CIRCUITS:
        c = _build(inputs, named)
        n_inputs, layers = G.named_to_layers(inputs, named)
        got = [[(int(t), int(b), int(x)) for t, b, x in zip(*arrays)] for arrays in c.gate_arrays()]
        assert got == layers
        rnd = random.Random(3)
        values = {name: rnd.randrange(1, p) for name in inputs}
        rows = c.evaluate(values, p)
        want = G.evaluate_circuit(layers, [values[name] for name in inputs], p)
        assert [list(r.values()) for r in rows] == want
        assert [list(r.keys()) for r in rows[1:]] == [[g[3] for g in layer] for layer in named]
    # the reference's labels: first use in the layer above, which is NOT the numbering (circuit 2 reads zzz before zz)
    c = _build(*G.REFERENCE_CIRCUITS[1])
    assert c.get_wire_label() == [["x", "y", "u", "v"], ["z1", "z2", "z3", "w", "xx"], ["zzz", "zz", "ww", "xxx"], ["a", "b", "xxxx"]]
    assert c.output_names() == ["a", "b", "xxxx"]
    assert [int(b) for b in c.gate_arrays()[2][1]] == [1, 1, 3]     # zzz is wire 1, xxx wire 3 of layer 2


def test_builder_refuses():
    c = LayeredCircuit(["x", "y"])
    with pytest.raises(ValueError):
        c.add_gate("SUB", "x", "y", "z")
    with pytest.raises(ValueError):
        c.add("x", "nope", "z")
    c.add("x", "y", "z")
    with pytest.raises(ValueError):
        c.mul("x", "y", "z")                  # the name is taken
    c.add_layer()
    with pytest.raises(ValueError):
        c.add("x", "z", "w")                  # x is two layers down
    with pytest.raises(ValueError):
        c.evaluate({"x": 1}, 97)
    with pytest.raises(ValueError):
        LayeredCircuit([])


def test_from_arrays_checks_every_index():
    u8, u32 = np.uint8, np.uint32
    ok = LayeredCircuit.from_arrays(3, [(np.array([0, 1], u8), np.array([0, 2], u32), np.array([2, 2], u32)),
                                        (np.array([1], u8), np.array([1], u32), np.array([0], u32))])
    assert ok.evaluate([2, 3, 5], 97) == [[2, 3, 5], [7, 25], [175 % 97]]
    with pytest.raises(TypeError):
        ok.add("a", "b", "c")
    for layers in ([(np.array([0], u8), np.array([3], u32), np.array([0], u32))],          # in1 == n_prev
                   [(np.array([0], u8), np.array([0], u32), np.array([2**32 - 1], u32))],  # in2 far out
                   [(np.array([0], u8), np.array([-1]), np.array([0]))],                   # negative
                   [(np.array([2], u8), np.array([0], u32), np.array([0], u32))],          # no such type
                   [(np.array([0, 1], u8), np.array([0], u32), np.array([0], u32))],       # lengths differ
                   [(np.array([], u8), np.array([], u32), np.array([], u32))],             # an empty layer
                   [(np.array([0], u8), np.array([0], u32), np.array([0], u32)),
                    (np.array([0], u8), np.array([1], u32), np.array([0], u32))]):         # wire 1 of a layer of one gate
        with pytest.raises(ValueError):
            LayeredCircuit.from_arrays(3, layers)
