"""GPU: the kernels of csrc/gkr.hip and the GKR prover / verifier against the integer model (tests/gkr_model.py), by ==.

The model runs each layer's sumcheck on the four dense tables of 2^(2k) entries; the prover under test never builds them.
Kernel tests call the C entry points themselves, with outputs pre-filled with garbage where "every row is written" is
the claim."""

import random

import numpy as np
import pytest

import gkr_model as G
import mle_model as M
from zksnake_amd import _native as N
from zksnake_amd.arithmetization import LayeredCircuit
from zksnake_amd.arithmetization.layered_circuit import CompiledLayer
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD
from zksnake_amd.device import DeviceBuffer
from zksnake_amd.frvec import DevVec, FrOps
from zksnake_amd.mle import MLE_OBJECT
from zksnake_amd.polynomial import Polynomial
from zksnake_amd.spmv import ITEM, LONG_ROW
from zksnake_amd.subprotocol import GKR, GkrPolynomial, ProductPolynomial, Sumcheck
from zksnake_amd.subprotocol.gkr import eq_table, wiring_eval
from zksnake_amd.transcript import FiatShamirTranscript

pytestmark = pytest.mark.gpu

T = N.MLE_TILE_LOG
FIELDS = (("BN254", BN254_SCALAR_FIELD), ("BLS12_381", BLS12_381_SCALAR_FIELD))
BY_FIELD = pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])


def upload(ops, values):
    return ops.d_from(N.ints_to_limbs(values, 4))


def ints(vec, count):
    return N.limbs_to_ints(vec.download(count))


def garbage(n, seed):
    """a DevVec of n elements that are no field elements at all"""
    vec = DevVec(n, zero=False)
    vec.upload(np.random.default_rng(seed).integers(1, 2**64, size=(n, 4), dtype=np.uint64))
    return vec


def arrays(gates):
    return (np.array([g[0] for g in gates], dtype=np.uint8), np.array([g[1] for g in gates], dtype=np.uint32),
            np.array([g[2] for g in gates], dtype=np.uint32))


def table(rnd, n, k, p):
    """n random values with 0 and p - 1 among them, padded to 2^k"""
    w = [rnd.randrange(1, p) for _ in range(n)]
    w[0] = 0
    w[-1] = p - 1 if n > 1 else w[-1]
    return G.pad(w, k)


# ---- eq table ----
@pytest.mark.parametrize("k", [0, 1, 2, T, T + 1, 13])
@BY_FIELD
def test_eq_table(gpu, name, p, k):
    ops = FrOps(p)
    rnd = random.Random(17 * k)
    points = [[rnd.randrange(p) for _ in range(k)]]
    if k:
        special = [rnd.randrange(p) for _ in range(k)]
        for i, v in zip(rnd.sample(range(k), min(k, 3)), (0, 1, p - 1)):
            special[i] = v
        points.append(special)
    for r in points:
        vec = eq_table(ops, r)
        assert ints(vec, 1 << k) == G.eq_table(r, p)
        total = np.zeros(4, dtype=np.uint64)
        N.check(gpu.zk_mle_sum_dev(ops.cid, 1 << k, vec.ptr(), N.u64p(total), None))
        assert N.limbs_to_ints(total.reshape(1, 4)) == [1]
    if k:   # a challenge above the modulus is reduced on entry
        raw = N.ints_to_limbs([points[0][0] + p] + points[0][1:], 4)
        out = garbage(1 << k, k)
        N.check(gpu.zk_gkr_eq_table_dev(ops.cid, k, N.u64p(raw), out.ptr(), None))
        assert ints(out, 1 << k) == G.eq_table(points[0], p)


# ---- layer evaluation ----
def _layer_eval(gpu, ops, gates, k_prev, w_vec, k):
    t, b, c = (DeviceBuffer.from_numpy(a) for a in arrays(gates))
    out = garbage(1 << k, 5)
    N.check(gpu.zk_gkr_layer_eval_dev(ops.cid, len(gates), t.ptr, b.ptr, c.ptr, k_prev, w_vec.ptr(), k, out.ptr(), None))
    return out


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2**18 + 1])
@BY_FIELD
def test_layer_eval(gpu, name, p, n):
    ops = FrOps(p)
    rnd = random.Random(n)
    n_prev = 300
    k_prev, k = G.num_vars(n_prev), G.num_vars(n)
    w = table(rnd, n_prev, k_prev, p)
    w_vec = upload(ops, w)
    mixes = ("mixed",) if n > 1000 else ("mixed", "add", "mul")
    for mix in mixes:
        gates = []
        for g in range(n):
            t = rnd.randrange(2) if mix == "mixed" else int(mix == "mul")
            b = rnd.randrange(n_prev)
            c = b if g % 3 == 0 else rnd.randrange(n_prev)            # b == c on a third of the gates
            if g % 7 == 0:
                b = rnd.choice((0, n_prev - 1))                       # the values 0 and p - 1
            gates.append((t, b, c))
        out = _layer_eval(gpu, ops, gates, k_prev, w_vec, k)
        got = out.download(1 << k)
        assert N.limbs_to_ints(got[:n]) == [(w[b] * w[c] if t else w[b] + w[c]) % p for t, b, c in gates], mix
        assert not got[n:].any(), "the padding up to 2^k is not zero"
    assert ints(w_vec, 1 << k_prev) == w


# ---- the bookkeeping passes and the wiring evaluation ----
def _skewed_layer(rnd):
    """8 wires below; the rows of BOTH CSRs have 0, 1, LONG_ROW, LONG_ROW + 1, ITEM, ITEM + 1, 2 ITEM + 1 and 2 entries"""
    lengths = [0, 1, LONG_ROW, LONG_ROW + 1, ITEM, ITEM + 1, 2 * ITEM + 1, 2]
    gates = []
    for b, count in enumerate(lengths):
        gates += [(rnd.randrange(2), b, (b + 3) % 8) for _ in range(count)]     # in2 is a rotation of in1: the same lengths
    rnd.shuffle(gates)
    return 8, gates


def _one_wire_layer(rnd):
    return 5, [(rnd.randrange(2), 2, 2) for _ in range(300)]


def _typed_layer(kind):
    def make(rnd):
        n_prev = 70
        return n_prev, [(kind, rnd.randrange(n_prev), rnd.randrange(n_prev)) for _ in range(LONG_ROW * 3)]
    return make


LAYERS = {"skewed rows": _skewed_layer, "one wire feeds everything": _one_wire_layer, "no ADD gate": _typed_layer(G.MUL),
          "no MUL gate": _typed_layer(G.ADD)}


@pytest.mark.parametrize("shape", list(LAYERS))
@BY_FIELD
def test_bookkeeping_passes_and_wiring(gpu, name, p, shape):
    ops = FrOps(p)
    rnd = random.Random(shape)
    n_prev, gates = LAYERS[shape](rnd)
    layer = CompiledLayer(n_prev, *arrays(gates))
    k, kp = layer.k, layer.k_prev
    assert (k, kp) == (G.num_vars(len(gates)), G.num_vars(n_prev))
    if shape == "skewed rows":
        for csr in (layer.by_b, layer.by_c):
            assert sorted(np.diff(csr.row_ptr.astype(np.int64)).tolist()) == sorted([0, 1, LONG_ROW, LONG_ROW + 1, ITEM, ITEM + 1, 2 * ITEM + 1, 2])
            assert csr.n_long == 4 and csr.n_items == 1 + 1 + 2 + 3
    w = table(rnd, n_prev, kp, p)
    r = [rnd.randrange(p) for _ in range(k)]
    u, v = [rnd.randrange(p) for _ in range(kp)], [rnd.randrange(p) for _ in range(kp)]
    e, e2 = G.eq_table(r, p), G.eq_table(u, p)
    w_vec, e_vec, e2_vec = upload(ops, w), upload(ops, e), upload(ops, e2)
    out = [garbage(1 << kp, s) for s in range(4)]
    N.check(gpu.zk_gkr_phase1_dev(ops.cid, *layer.by_b.args(), k, e_vec.ptr(), w_vec.ptr(), out[0].ptr(), out[1].ptr(), None))
    N.check(gpu.zk_gkr_phase2_dev(ops.cid, *layer.by_c.args(), k, e_vec.ptr(), e2_vec.ptr(), out[2].ptr(), out[3].ptr(), None))
    want = G.phase1_tables(gates, kp, w, e, p) + G.phase2_tables(gates, kp, e, e2, p)
    for got, expect, label in zip(out, want, ("P", "Q", "Aadd", "Amul")):
        assert ints(got, 1 << kp) == expect, label
    assert wiring_eval(ops, layer, r, u, v) == G.wiring(gates, r, u, v, p)
    assert (ints(w_vec, 1 << kp), ints(e_vec, 1 << k), ints(e2_vec, 1 << kp)) == (w, e, e2), "an input table was modified"


# ---- end to end ----
def _named(inputs, named):
    c = LayeredCircuit(inputs)
    for j, layer in enumerate(named):
        if j:
            c.add_layer()
        for gate in layer:
            c.add_gate(*gate)
    return c


def _from_layers(n_inputs, layers):
    return LayeredCircuit.from_arrays(n_inputs, [arrays(g) for g in layers])


def _plain(proofs):
    return [[u.coeffs() for u in proof[:-1]] + [(proof[-1][0].coeffs(), proof[-1][1], proof[-1][2])] for proof in proofs]


def _bump(poly, p, i=0):
    c = poly.coeffs()
    c[i] = (c[i] + 1) % p
    return Polynomial(c, p)


def _check_against_model(gkr, n_inputs, layers, inputs, p, output_names=None):
    outputs, proofs, trace = G.prove(layers, inputs, p)
    got_out, got = gkr.prove(dict(zip(gkr.circuit.inputs, inputs)) if output_names else inputs)
    assert (list(got_out.values()) if output_names else got_out) == outputs
    if output_names:
        assert list(got_out.keys()) == output_names
    assert _plain(got) == proofs
    assert [t["challenges"] for t in gkr.last_trace] == [t["challenges"] for t in trace]
    assert [(t["r"], t["claim"]) for t in gkr.last_trace] == [(t["r"], t["claim"]) for t in trace]
    return got_out, got


def _tamperings(gkr, inputs, out, proofs, p):
    """one output, one round coefficient, z1, q, one input: each alone must turn the verdict"""
    named = isinstance(out, dict)
    assert gkr.verify(inputs, out, proofs) is True
    bad_out = dict(out) if named else list(out)
    key = next(iter(out)) if named else 0
    bad_out[key] = (bad_out[key] + 1) % p
    assert gkr.verify(inputs, bad_out, proofs) is False
    bad_in = dict(inputs) if named else list(inputs)
    key = list(inputs)[-1] if named else len(inputs) - 1
    bad_in[key] = (bad_in[key] + 1) % p
    assert gkr.verify(bad_in, out, proofs) is False
    for li in {0, len(proofs) - 1}:
        q, z1, z2 = proofs[li][-1]
        for ri in {0, len(proofs[li]) - 2}:
            bad = [list(pr) for pr in proofs]
            bad[li][ri] = _bump(proofs[li][ri], p, len(proofs[li][ri].coeffs()) - 1)
            assert gkr.verify(inputs, out, bad) is False
        for last in ((q, (z1 + 1) % p, z2), (_bump(q, p), z1, z2), (_bump(q, p), (z1 + 1) % p, z2)):
            bad = [list(pr) for pr in proofs]
            bad[li][-1] = last
            assert gkr.verify(inputs, out, bad) is False
    prefixed = FiatShamirTranscript(b"gkr", field=p)
    prefixed.append(1)
    assert gkr.verify(inputs, out, proofs, prefixed) is False


@BY_FIELD
def test_the_references_circuits(gpu, name, p):
    rnd = random.Random("gkr")
    for inputs, named in G.REFERENCE_CIRCUITS:
        circuit = _named(inputs, named)
        n_inputs, layers = G.named_to_layers(inputs, named)
        values = [rnd.randrange(1, p - 1) for _ in inputs]
        gkr = GKR(circuit, p)
        out, proofs = _check_against_model(gkr, n_inputs, layers, values, p, [g[3] for g in named[-1]])
        input_map = dict(zip(inputs, values))
        assert out == circuit.evaluate(input_map, p)[-1]
        _tamperings(gkr, input_map, out, proofs, p)
        # the same circuit from arrays: the same proof, the output as a list
        plain = GKR(_from_layers(n_inputs, layers), p)
        out2, proofs2 = plain.prove(values)
        assert out2 == list(out.values()) and _plain(proofs2) == _plain(proofs)
        assert plain.verify(values, out2, proofs) is True and gkr.verify(input_map, out, proofs2) is True
        limbs = N.ints_to_limbs(values, 4)
        assert _plain(plain.prove(limbs)[1]) == _plain(proofs) and plain.verify(limbs, out2, proofs) is True


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@BY_FIELD
def test_random_circuits(gpu, name, p, depth):
    rnd = random.Random(f"{name} {depth}")
    for _ in range(3):
        n_inputs, layers = G.random_circuit(rnd, depth)
        values = [rnd.randrange(1, p) for _ in range(n_inputs)]
        gkr = GKR(_from_layers(n_inputs, layers), p)
        out, proofs = _check_against_model(gkr, n_inputs, layers, values, p)
        _tamperings(gkr, values, out, proofs, p)


@BY_FIELD
def test_a_callers_transcript_with_earlier_content(gpu, name, p):
    n_inputs, layers = G.named_to_layers(*G.REFERENCE_CIRCUITS[1])
    values = [3, 5, 7, 11]
    gkr = GKR(_from_layers(n_inputs, layers), p)
    ours, model, check, other = (FiatShamirTranscript(b"outer", field=p), M.Transcript(b"outer", p),
                                 FiatShamirTranscript(b"outer", field=p), FiatShamirTranscript(b"outer", field=p))
    for tr in (ours, model, check):
        tr.append([12345, p - 1])
    other.append([12345, p - 2])
    out, proofs = gkr.prove(values, ours)
    assert _plain(proofs) == G.prove(layers, values, p, model)[1]
    assert _plain(proofs) != G.prove(layers, values, p)[1]
    assert gkr.verify(values, out, proofs, check) is True
    assert gkr.verify(values, out, proofs, other) is False        # replayed under another prefix
    assert gkr.verify(values, out, proofs) is False               # and under none


@BY_FIELD
def test_gkr_polynomial_against_the_dense_broadcast_path(gpu, name, p):
    """k = 4: the round polynomials of the sparse prover are those of the four broadcast tables of 2^8 entries"""
    ops = FrOps(p)
    rnd = random.Random(44)
    n_prev, n = 16, 13
    gates = [(rnd.randrange(2), rnd.randrange(n_prev), rnd.randrange(n_prev)) for _ in range(n)]
    k, kp = G.num_vars(n), 4
    w = table(rnd, n_prev, kp, p)
    r = [rnd.randrange(p) for _ in range(k)]
    dense = G.dense_tables(gates, kp, w, r, p)
    broadcast = ProductPolynomial([MLE_OBJECT[p].from_evaluations(t, p) for t in dense], G.DENSE_TERMS, p)
    w_poly = MLE_OBJECT[p].from_evaluations(w, p)
    sparse = GkrPolynomial(CompiledLayer(n_prev, *arrays(gates)), w_poly, r, p)
    sc = Sumcheck(2 * kp, p)
    claim_d, proof_d, rs_d = sc.prove_arbitrary(broadcast)
    claim_s, proof_s, rs_s = sc.prove_arbitrary(sparse)
    assert claim_s == claim_d and rs_s == rs_d
    assert [u.coeffs() for u in proof_s] == [u.coeffs() for u in proof_d]
    assert sc.verify(claim_s, proof_s, 2, mlpoly=sparse) == rs_s
    assert sparse.evaluate(rs_s) == broadcast.evaluate(rs_s) == M.f_value(dense, G.DENSE_TERMS, rs_s, p)
    assert sparse.wu == M.evaluate(w, rs_s[:kp], p)
    # to_evaluations: the dense table's entries where a predicate is non-zero, walked b first as the reference walks them
    f_table = broadcast.to_evaluations()
    joined = [c << kp | b for b in range(1 << kp) for c in range(1 << kp) if dense[0][c << kp | b] or dense[3][c << kp | b]]
    assert sparse.to_evaluations() == [f_table[i] for i in joined]
    assert sum(sparse.to_evaluations()) % p == claim_s
    # a restart with another prefix, then back
    other = [(x + 1) % p for x in rs_s[:kp]] + rs_s[kp:kp + 2]
    fixed = [M.fix(t, other[:-1], p) for t in dense]
    assert sparse.round_function(other[:-1]).coeffs() == M.interpolate(M.round_sums(fixed, G.DENSE_TERMS, p), p)
    assert sparse.round_function(rs_s[:kp + 1]).coeffs() == proof_s[kp + 1].coeffs()
    assert sparse.round_function(rs_s[:2]).coeffs() == proof_s[2].coeffs()
    assert w_poly.to_evaluations() == w


@BY_FIELD
def test_one_wide_circuit(gpu, name, p):
    """depth 3, width 2^12 + 3, wire 0 of every layer read 2^12 times by the layer above (long rows in both CSRs)"""
    ops = FrOps(p)
    rnd = random.Random(name)
    width, fan = 2**12 + 3, 2**12
    layers = []
    for _ in range(3):
        gates = [(rnd.randrange(2), 0, rnd.randrange(width)) for _ in range(fan // 2)]
        gates += [(rnd.randrange(2), rnd.randrange(1, width), 0) for _ in range(fan // 2)]
        gates += [(rnd.randrange(2), rnd.randrange(1, width), rnd.randrange(1, width)) for _ in range(width - fan)]
        rnd.shuffle(gates)
        layers.append(gates)
    values = [rnd.randrange(1, p) for _ in range(width)]
    gkr = GKR(_from_layers(width, layers), p)
    assert all(layer.by_b.n_long >= 1 and layer.by_c.n_long >= 1 for layer in gkr.layers)
    out, proofs = gkr.prove(values)
    rows = G.evaluate_circuit(layers, values, p)
    assert out == rows[-1]
    assert gkr.verify(values, out, proofs) is True
    bad = list(out)
    bad[-1] = (bad[-1] + 1) % p
    assert gkr.verify(values, bad, proofs) is False
    tables = gkr.evaluate_layers(upload(ops, G.pad(values, 13)))
    for i, j in enumerate(range(3, 0, -1)):
        trace, layer, gates = gkr.last_trace[i], gkr.layers[j - 1], layers[j - 1]
        assert tables[j].to_evaluations() == G.pad(rows[j], 13)
        assert trace["claim"] == tables[j].evaluate(trace["r"])
        f = GkrPolynomial(layer, tables[j - 1], trace["r"], p)
        w, e = G.pad(rows[j - 1], 13), G.eq_table(trace["r"], p)
        assert (f.p_table.to_evaluations(), f.q_table.to_evaluations()) == G.phase1_tables(gates, 13, w, e, p)
        u = trace["challenges"][:13]
        f.round_function(u)
        assert (f.add_table.to_evaluations(), f.mul_table.to_evaluations()) == G.phase2_tables(gates, 13, e, G.eq_table(u, p), p)
        assert f.wu == proofs[i][-1][1]


# ---- arguments ----
def test_an_out_of_range_gate_is_refused_when_the_circuit_is_made(gpu):
    u8, u32 = np.uint8, np.uint32
    with pytest.raises(ValueError):
        LayeredCircuit.from_arrays(4, [(np.array([0, 1], u8), np.array([0, 4], u32), np.array([1, 1], u32))])
    with pytest.raises(ValueError):
        LayeredCircuit.from_arrays(4, [(np.array([0, 2], u8), np.array([0, 3], u32), np.array([1, 1], u32))])
    for bad in ((np.array([0], u8), np.array([0], u32), np.array([4], u32)), (np.array([0], u8), np.array([2**31], u32), np.array([0], u32))):
        with pytest.raises(ValueError):
            CompiledLayer(4, *bad)        # the last stop before the arrays reach the device


@BY_FIELD
def test_entry_points_refuse_bad_arguments(gpu, name, p):
    ops = FrOps(p)
    rnd = random.Random(9)
    gates = [(rnd.randrange(2), rnd.randrange(8), rnd.randrange(8)) for _ in range(8)]
    layer = CompiledLayer(8, *arrays(gates))
    big = N.GKR_MAX_LOG + 1
    buf = garbage(64, 1)
    before = buf.download(64)
    r = N.ints_to_limbs([rnd.randrange(p) for _ in range(big)], 4)
    t, b, c = layer.d_types.ptr, layer.d_in1.ptr, layer.d_in2.ptr
    E = N.ZK_ERR_ARG
    # eq table: k above the cap, negative, null
    assert gpu.zk_gkr_eq_table_dev(ops.cid, big, N.u64p(r), buf.ptr(), None) == E
    assert gpu.zk_gkr_eq_table_dev(ops.cid, -1, N.u64p(r), buf.ptr(), None) == E
    assert gpu.zk_gkr_eq_table_dev(ops.cid, 3, None, buf.ptr(), None) == E
    assert gpu.zk_gkr_eq_table_dev(ops.cid, 3, N.u64p(r), None, None) == E
    assert gpu.zk_gkr_eq_table_dev(2, 3, N.u64p(r), buf.ptr(), None) == E
    # layer evaluation: sizes, more gates than the table holds, the output inside the input
    assert gpu.zk_gkr_layer_eval_dev(ops.cid, 8, t, b, c, 3, buf.ptr(0), big, buf.ptr(8), None) == E
    assert gpu.zk_gkr_layer_eval_dev(ops.cid, 8, t, b, c, big, buf.ptr(0), 3, buf.ptr(8), None) == E
    assert gpu.zk_gkr_layer_eval_dev(ops.cid, 9, t, b, c, 3, buf.ptr(0), 3, buf.ptr(8), None) == E
    assert gpu.zk_gkr_layer_eval_dev(ops.cid, 8, t, b, c, 3, buf.ptr(0), 3, buf.ptr(7), None) == E
    assert gpu.zk_gkr_layer_eval_dev(ops.cid, 8, t, b, c, 3, buf.ptr(4), 3, buf.ptr(0), None) == E
    assert gpu.zk_gkr_layer_eval_dev(ops.cid, 8, None, b, c, 3, buf.ptr(0), 3, buf.ptr(8), None) == E
    # the passes: E | W | out0 | out1 at 0, 8, 16, 24
    for fn in (gpu.zk_gkr_phase1_dev, gpu.zk_gkr_phase2_dev):
        csr = layer.by_b.args() if fn is gpu.zk_gkr_phase1_dev else layer.by_c.args()
        assert fn(ops.cid, *csr, big, buf.ptr(0), buf.ptr(8), buf.ptr(16), buf.ptr(24), None) == E
        assert fn(ops.cid, big, *csr[1:], 3, buf.ptr(0), buf.ptr(8), buf.ptr(16), buf.ptr(24), None) == E
        assert fn(ops.cid, *csr, 2, buf.ptr(0), buf.ptr(8), buf.ptr(16), buf.ptr(24), None) == E      # 8 gates, a table of 4
        assert fn(ops.cid, *csr, 3, buf.ptr(0), buf.ptr(8), buf.ptr(16), buf.ptr(23), None) == E      # the outputs overlap
        assert fn(ops.cid, *csr, 3, buf.ptr(0), buf.ptr(8), buf.ptr(7), buf.ptr(24), None) == E       # an output inside E
        assert fn(ops.cid, *csr, 3, buf.ptr(0), buf.ptr(8), buf.ptr(16), buf.ptr(15), None) == E      # an output inside W / E2
        assert fn(ops.cid, *csr, 3, buf.ptr(0), buf.ptr(8), None, buf.ptr(24), None) == E
        assert fn(ops.cid, *csr[:6], 1, None, None, 1, None, None, 3, buf.ptr(0), buf.ptr(8), buf.ptr(16), buf.ptr(24), None) == E
    # wiring evaluation
    res = np.full((2, 4), 7, dtype=np.uint64)
    assert gpu.zk_gkr_wiring_eval_dev(ops.cid, 8, t, b, c, big, buf.ptr(0), 3, buf.ptr(8), buf.ptr(16), N.u64p(res), None) == E
    assert gpu.zk_gkr_wiring_eval_dev(ops.cid, 8, t, b, c, 3, buf.ptr(0), big, buf.ptr(8), buf.ptr(16), N.u64p(res), None) == E
    assert gpu.zk_gkr_wiring_eval_dev(ops.cid, 9, t, b, c, 3, buf.ptr(0), 3, buf.ptr(8), buf.ptr(16), N.u64p(res), None) == E
    assert gpu.zk_gkr_wiring_eval_dev(ops.cid, 8, t, b, c, 3, buf.ptr(0), 3, buf.ptr(8), buf.ptr(16), None, None) == E
    assert (res == 7).all()
    assert np.array_equal(buf.download(64), before), "a refused call wrote to its buffers"
    # and the same calls, put right, pass
    assert gpu.zk_gkr_layer_eval_dev(ops.cid, 8, t, b, c, 3, buf.ptr(0), 3, buf.ptr(8), None) == N.ZK_OK
    assert gpu.zk_gkr_phase1_dev(ops.cid, *layer.by_b.args(), 3, buf.ptr(0), buf.ptr(8), buf.ptr(16), buf.ptr(24), None) == N.ZK_OK
