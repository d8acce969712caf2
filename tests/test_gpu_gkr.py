"""GPU: the kernels of csrc/gkr.hip and the GKR prover / verifier against the integer model (tests/gkr_model.py), by ==.

The model runs each layer's sumcheck on the four dense tables of 2^(2k) entries; the prover under test never builds them.
Kernel tests call the C entry points themselves, with outputs pre-filled with garbage where "every row is written" is
the claim.

The sizes at which a thread takes a SECOND item are derived from the constants they sit on (GKR_MAX_BLOCKS of csrc/gkr.hip, read
from the source; MLE_TILE; ITEM of zksnake_amd/spmv.py) and the derivation is asserted: a changed constant fails there, then
the tests move.  At those sizes E is a table of powers g^i made on the device and pinned at about 64 indices, and every
expectation is one Python loop with a running power."""

import os
import random
import re

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
TILE = 1 << T
FIELDS = (("BN254", BN254_SCALAR_FIELD), ("BLS12_381", BLS12_381_SCALAR_FIELD))
BY_FIELD = pytest.mark.parametrize("name,p", FIELDS, ids=[f[0] for f in FIELDS])
with open(os.path.join(os.path.dirname(os.path.abspath(N.__file__)), "csrc", "gkr.hip")) as _f:
    MAX_BLOCKS = int(re.search(r"constexpr unsigned GKR_MAX_BLOCKS = (\d+);", _f.read()).group(1))   # read from the source
GRID = MAX_BLOCKS * TILE               # threads of a capped grid: item GRID is some thread's second
EQ_SECOND_LOG = GRID.bit_length()      # the smallest k whose 2^k entries do not fit one sweep of the grid
WIRING_SECOND = GRID + TILE + 1        # gates: the grid strides, and the workgroup of the last gate holds that gate alone
LONG_SECOND = TILE * ITEM + 1          # entries of one row: TILE + 1 work items, so a thread of gkr_phase_long_kernel takes two
assert (GRID, EQ_SECOND_LOG, WIRING_SECOND, LONG_SECOND) == (2**18, 19, 2**18 + 257, 256 * ITEM + 1)   # the sizes the tests were written for
TOP_SIZE = 2 * TILE + 1                # "every term at the top of the range": two workgroups and one element


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


def eq_table_by_doubling(r, p):
    """variable t doubles the table: the upper half is the lower half times r_t, and the lower half loses what the upper half got --
    one product per entry of the result"""
    tab = [1]
    for rt in r:
        hi = [e * rt % p for e in tab]
        tab = [(e - h) % p for e, h in zip(tab, hi)] + hi
    return tab


@BY_FIELD
def test_eq_table_where_a_thread_takes_a_second_item(gpu, name, p):
    k = EQ_SECOND_LOG
    ops = FrOps(p)
    rnd = random.Random(f"eq {name}")
    special = [rnd.randrange(p) for _ in range(k)]
    special[2], special[T + 1], special[k - 1] = 0, 1, p - 1       # among them the variable that is bit 18: the second item's
    for r in ([rnd.randrange(p) for _ in range(k)], special):
        out = garbage(1 << k, k)
        N.check(gpu.zk_gkr_eq_table_dev(ops.cid, k, N.u64p(N.ints_to_limbs(r, 4)), out.ptr(), None))
        assert np.array_equal(out.download(), N.ints_to_limbs(eq_table_by_doubling(r, p), 4))
        total = np.zeros(4, dtype=np.uint64)
        N.check(gpu.zk_mle_sum_dev(ops.cid, 1 << k, out.ptr(), N.u64p(total), None))
        assert N.limbs_to_ints(total.reshape(1, 4)) == [1]


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


def pin_indices(n, edges, seed):
    """about 64 indices: first, last, workgroup edges, both sides of every edge in `edges`, random ones"""
    fixed = {0, 1, n - 2, n - 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, n - TILE - 1, n - TILE}
    for e in edges:
        fixed |= {e - 1, e, e + 1}
    fixed = {i for i in fixed if 0 <= i < n}
    rnd = random.Random(seed)
    while len(fixed) < 64:
        fixed.add(rnd.randrange(n))
    return sorted(fixed)


def powers_table(ops, g, n, edges):
    """g^i for i < n, made on the device (zk_vec_powers_dev) and pinned against pow() before anyone uses it"""
    vec = ops.d_powers(g, n)
    for i in pin_indices(n, edges, n):
        assert N.limbs_to_ints(vec.download(1, i)) == [pow(g, i, ops.r)], f"the table of powers, index {i}"
    return vec


def random_gates(seed, n, n_prev):
    """(types, in1, in2) as numpy arrays, mixed types, wires 0 and n_prev - 1 among the inputs"""
    rng = np.random.default_rng(seed)
    types = rng.integers(0, 2, size=n, dtype=np.uint8)
    in1, in2 = rng.integers(0, n_prev, size=n, dtype=np.uint32), rng.integers(0, n_prev, size=n, dtype=np.uint32)
    in1[::7], in2[::5] = 0, n_prev - 1
    return types, in1, in2


def _wiring(gpu, ops, n, d_gates, k, er, kp, eu, ev):
    out = np.full((2, 4), 0x77, dtype=np.uint64)
    N.check(gpu.zk_gkr_wiring_eval_dev(ops.cid, n, *d_gates, k, er, kp, eu, ev, N.u64p(out), None))
    return tuple(N.limbs_to_ints(out))


@BY_FIELD
def test_wiring_where_a_thread_takes_a_second_item(gpu, name, p):
    """2^18 + 257 gates: gkr_wiring_kernel runs its capped grid of 1024 workgroups, 257 threads take a second gate, and
    mle_combine_kernel reads 1024 partial pairs.  The kernel takes any field elements for its three tables: E_r = g^i."""
    n, n_prev = WIRING_SECOND, 300
    assert -(-n // TILE) > MAX_BLOCKS and n - GRID == TILE + 1
    ops = FrOps(p)
    k, kp = G.num_vars(n), G.num_vars(n_prev)
    assert (k, kp) == (EQ_SECOND_LOG, 9)
    rnd = random.Random(f"wiring {name}")
    g = rnd.randrange(1 << 250, p)
    types, in1, in2 = random_gates(18, n, n_prev)
    d_gates = [DeviceBuffer.from_numpy(a) for a in (types, in1, in2)]
    eu, ev = table(rnd, n_prev, kp, p), table(rnd, n_prev, kp, p)
    er_vec = powers_table(ops, g, 1 << k, (GRID, n))
    eu_vec, ev_vec = upload(ops, eu), upload(ops, ev)
    got = _wiring(gpu, ops, n, [d.ptr for d in d_gates], k, er_vec.ptr(), kp, eu_vec.ptr(), ev_vec.ptr())
    acc, power = [0, 0], 1
    for t, b, c in zip(types.tolist(), in1.tolist(), in2.tolist()):
        acc[t] += power * eu[b] * ev[c]
        power = power * g % p
    assert got == (acc[0] % p, acc[1] % p)
    assert (ints(eu_vec, 1 << kp), ints(ev_vec, 1 << kp)) == (eu, ev), "an input table was modified"


@BY_FIELD
def test_phases_where_a_thread_of_the_long_rows_kernel_takes_a_second_item(gpu, name, p):
    """one row of 256 ITEM + 1 entries in both CSRs (every gate reads wire 0 twice): 257 work items, the smallest count at which
    gkr_phase_long_kernel strides.  With one row, each output is one sum over the gates: E = g^a, so one running power."""
    n, n_prev = LONG_SECOND, 8
    ops = FrOps(p)
    rng = np.random.default_rng(21)
    types = rng.integers(0, 2, size=n, dtype=np.uint8)
    zeros = np.zeros(n, dtype=np.uint32)
    layer = CompiledLayer(n_prev, types, zeros, zeros)
    k, kp = layer.k, layer.k_prev
    assert (k, kp) == (21, 3)
    for csr in (layer.by_b, layer.by_c):
        assert csr.n_long == 1 and csr.n_items == TILE + 1 == 257
        assert csr.items.tolist()[-2:] == [[(TILE - 1) * ITEM, TILE * ITEM], [TILE * ITEM, n]]
    rnd = random.Random(f"long {name}")
    g = rnd.randrange(1 << 250, p)
    w, e2 = table(rnd, n_prev, kp, p), table(rnd, n_prev, kp, p)
    w[0], e2[0] = rnd.randrange(1, p), p - 1           # the one entry of each that is read
    e_vec = powers_table(ops, g, 1 << k, (GRID, ITEM, TILE * ITEM, n))
    w_vec, e2_vec = upload(ops, w), upload(ops, e2)
    out = [garbage(1 << kp, s) for s in range(4)]
    N.check(gpu.zk_gkr_phase1_dev(ops.cid, *layer.by_b.args(), k, e_vec.ptr(), w_vec.ptr(), out[0].ptr(), out[1].ptr(), None))
    N.check(gpu.zk_gkr_phase2_dev(ops.cid, *layer.by_c.args(), k, e_vec.ptr(), e2_vec.ptr(), out[2].ptr(), out[3].ptr(), None))
    sums, power = [0, 0], 1
    for t in types.tolist():
        sums[t] += power
        power = power * g % p
    s_add, s_mul = sums[0] % p, sums[1] % p
    want = ((s_add + s_mul * w[0]) % p, s_add * w[0] % p, s_add * e2[0] % p, s_mul * e2[0] % p)
    for got, expect, label in zip(out, want, ("P", "Q", "Aadd", "Amul")):
        assert ints(got, 1 << kp) == [expect] + [0] * 7, label
    assert (ints(w_vec, 1 << kp), ints(e2_vec, 1 << kp)) == (w, e2), "an input table was modified"


@pytest.mark.parametrize("log_rows", [3, T + 1], ids=["8 rows", "two workgroups of rows"])
@BY_FIELD
def test_empty_layers_through_the_c_abi(gpu, name, p, log_rows):
    """no gate at all: an all-zero row_ptr and null gate arrays.  Every row is written as zero over garbage, and the wiring
    predicates are (0, 0)"""
    ops = FrOps(p)
    rnd = random.Random(31)
    n_rows = 1 << log_rows
    row_ptr = DeviceBuffer.from_numpy(np.zeros(n_rows + 1, dtype=np.uint32))
    e_vec, y_vec = upload(ops, table(rnd, 2, 1, p)), upload(ops, table(rnd, n_rows, log_rows, p))
    csr = (log_rows, 0, row_ptr.ptr, None, None, None, 0, None, None, 0, None, None)
    for fn in (gpu.zk_gkr_phase1_dev, gpu.zk_gkr_phase2_dev):
        out = [garbage(n_rows, s) for s in (7, 8)]
        N.check(fn(ops.cid, *csr, 1, e_vec.ptr(), y_vec.ptr(), out[0].ptr(), out[1].ptr(), None))
        assert not out[0].download().any() and not out[1].download().any()
    assert _wiring(gpu, ops, 0, (None, None, None), 1, e_vec.ptr(), log_rows, y_vec.ptr(), y_vec.ptr()) == (0, 0)


@BY_FIELD
def test_sums_with_every_term_at_the_top_of_the_range(gpu, name, p):
    """every entry of E, W, E2, E_r, E_u, E_v is p - 1, over 2 x 256 + 1 gates: wire 0 feeds 256 + 192 of them (a long row whose one
    item ends in a short sweep), wire 1 feeds LONG_ROW (the longest lane-per-row sum), wire 2 feeds one.  The wiring kernel runs
    three workgroups, the last with one gate, and its combine reads three partial pairs.  Every term is +-1, so each result is
    also a count of gates."""
    ops = FrOps(p)
    n, n_prev = TOP_SIZE, 8
    assert n == 513 and n - LONG_ROW - 1 > LONG_ROW
    types = np.random.default_rng(41).integers(0, 2, size=n, dtype=np.uint8)
    wire = np.array([0] * (n - LONG_ROW - 1) + [1] * LONG_ROW + [2], dtype=np.uint32)
    gates = list(zip(types.tolist(), wire.tolist(), wire.tolist()))
    layer = CompiledLayer(n_prev, types, wire, wire)
    k, kp = layer.k, layer.k_prev
    assert (k, kp) == (10, 3) and layer.by_b.n_long == layer.by_c.n_long == 1 and layer.by_b.n_items == 1
    e, y = [p - 1] * (1 << k), [p - 1] * (1 << kp)
    e_vec, y_vec = upload(ops, e), upload(ops, y)
    out = [garbage(1 << kp, s) for s in range(4)]
    N.check(gpu.zk_gkr_phase1_dev(ops.cid, *layer.by_b.args(), k, e_vec.ptr(), y_vec.ptr(), out[0].ptr(), out[1].ptr(), None))
    N.check(gpu.zk_gkr_phase2_dev(ops.cid, *layer.by_c.args(), k, e_vec.ptr(), y_vec.ptr(), out[2].ptr(), out[3].ptr(), None))
    got = [ints(o, 1 << kp) for o in out]
    assert got == list(G.phase1_tables(gates, kp, y, e, p)) + list(G.phase2_tables(gates, kp, e, y, p))
    n_mul = [int(types[wire == b].sum()) for b in range(n_prev)]
    n_add = [int((wire == b).sum()) - m for b, m in enumerate(n_mul)]
    # E W = E E2 = 1 and E = -1: P = -#ADD + #MUL, Q = #ADD, Aadd = #ADD, Amul = #MUL, row by row
    assert got == [[(m - a) % p for a, m in zip(n_add, n_mul)], n_add, n_add, n_mul]
    d_gates = (layer.d_types.ptr, layer.d_in1.ptr, layer.d_in2.ptr)
    wired = _wiring(gpu, ops, n, d_gates, k, e_vec.ptr(), kp, y_vec.ptr(), y_vec.ptr())
    model = [0, 0]
    for a, (t, b, c) in enumerate(gates):
        model[t] = (model[t] + e[a] * y[b] * y[c]) % p
    assert wired == tuple(model) == ((-sum(n_add)) % p, (-sum(n_mul)) % p)
    assert (ints(e_vec, 1 << k), ints(y_vec, 1 << kp)) == (e, y), "an input table was modified"


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
