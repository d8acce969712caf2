"""
GKR for layered circuits (Goldwasser, Kalai, Rothblum 2008; Thaler, "Proofs, Arguments, and Zero-Knowledge", section 4.6) with
the reference's interface, transcript order and proof shape (python/zksnake/subprotocol/gkr.py:95-355), and a prover that is
LINEAR in the number of gates: the wiring predicates add_j, mul_j have one non-zero entry per gate, so every sum over them is
a sum over gates through a static CSR (the two-phase bookkeeping of Libra, Xie et al. 2019; csrc/gkr.hip).

Protocol.  Layers 0 (inputs) .. d; layer j has n_j wires, k_j = max(1, ceil(log2 n_j)) variables and a dense table W_j of
2^k_j values, zero beyond n_j.  Variable 0 is the least significant index bit.  The transcript (label b"gkr") takes every
input value, then every output value; r in F^(k_d) is drawn and m = W~_d(r).  For j = d .. 1, with k = k_(j-1), a sumcheck in
2k variables (b_0 .. b_(k-1), c_0 .. c_(k-1)) with claim m runs on
    f(b, c) = sum_a eq(r, a) [ add_j(a, b, c) (W~_(j-1)(b) + W~_(j-1)(c)) + mul_j(a, b, c) W~_(j-1)(b) W~_(j-1)(c) ]
through Sumcheck.prove_arbitrary on the same transcript; u, v = the first and the last k challenges; q(t) = W~_(j-1)(u + t (v - u))
(degree <= k), z1 = q(0), z2 = q(1); every round polynomial's coeffs() is appended again, then q.coeffs(), then [z1, z2]; one
challenge r* gives the next r = u + r* (v - u) and the next m = q(r*).  A layer's proof is [round polynomials .., (q, z1, z2)].
The verifier makes the reference's checks in the reference's order (sumcheck with degree bound 2, q(0) == z1 and q(1) == z2,
the last round against add~_j(r, u, v) (z1 + z2) + mul~_j(r, u, v) z1 z2, at the end W~_0(r) == m) and rejects a q of degree
above k.

GKR PROOFS ARE NOT INTERCHANGEABLE WITH THE REFERENCE'S, for two reasons that cannot be kept:
 1. Variable count.  The reference gives a layer of n wires n variables, not ceil(log2 n) (gkr.py:148-150, :234-238): a layer
    of 64 wires would need a hypercube of 2^64 points.  Here a layer has k_j variables.
 2. Wire numbering.  The reference numbers a layer's wires by first use in the layer above (get_wire_label) and the same
    layer's gates by position (gkr.py:118-126); the two disagree whenever the layer above reads wires in another order or
    leaves one unread.  Here wire t of layer j is the output of gate t of layer j, wire t of layer 0 is circuit.inputs[t], and
    unread wires keep their slot.  `LayeredCircuit.get_wire_label()` still returns the reference's lists; nothing here
    indexes by them.
As in the reference, a round polynomial (or q) that is identically zero has coeffs() == [], which transcript.append rejects
with TypeError.

The prover.  With E[a] = eq(r, a):
  phase 1 (variables b)   P[b] = sum_ADD E[a] + sum_MUL E[a] W[c],  Q[b] = sum_ADD E[a] W[c]   (gates of row b = in1), and f summed
                          over c is P(b) W(b) + Q(b): ProductPolynomial([P, W, Q], [(1, (0, 1)), (1, (2,))]);
  phase 2 (variables c)   wu = W~(u), E2[b] = eq(u, b), Aadd[c] = sum_ADD E[a] E2[b], Amul[c] the same over MUL gates (row c = in2),
                          and f(u, c) = wu Aadd(c) + Aadd(c) W(c) + wu Amul(c) W(c):
                          ProductPolynomial([Aadd, W, Amul], [(wu, (0,)), (1, (0, 1)), (wu, (2, 1))]),
so all 2k rounds run on the fused sumcheck round kernel.  The tables never leave the device: challenges, s(0..3) per round, wu,
the k + 1 samples of q and the two predicate values are all that crosses the bus.
"""

import numpy as np

from .. import _native as N
from ..arithmetization.layered_circuit import LayeredCircuit
from ..constant import BN254_SCALAR_FIELD
from ..frvec import DevVec, FrOps
from ..mle import MLE_OBJECT
from ..polynomial import Polynomial
from ..transcript import FiatShamirTranscript
from .sumcheck import ProductPolynomial, Sumcheck, SumcheckPolynomial


def eq_table(ops, r):
    """DevVec of eq(r, x) over x in {0,1}^len(r): one launch, every entry written from the challenges"""
    r = list(r)
    out = DevVec(1 << len(r), zero=False)
    N.check(N.load().zk_gkr_eq_table_dev(ops.cid, len(r), N.u64p(ops.limbs(r)) if r else None, out.ptr(), None))
    return out


def wiring_eval(ops, layer, r, u, v):
    """(add~_j(r, u, v), mul~_j(r, u, v)) of a CompiledLayer, as a sum over its gates"""
    er, eu, ev = eq_table(ops, r), eq_table(ops, u), eq_table(ops, v)
    out = np.zeros((2, 4), dtype=np.uint64)
    N.check(N.load().zk_gkr_wiring_eval_dev(ops.cid, layer.n, layer.d_types.ptr, layer.d_in1.ptr, layer.d_in2.ptr, layer.k, er.ptr(),
                                            layer.k_prev, eu.ptr(), ev.ptr(), N.u64p(out), None))
    return tuple(ops.ints(out))


def interpolate(ys, p):
    """coefficients (lowest first) of the polynomial of degree < len(ys) through (t, ys[t]), t = 0 .. len(ys)-1"""
    n = len(ys)
    out = [0] * n
    for j, y in enumerate(ys):
        num, den = [1], 1
        for m in range(n):
            if m != j:
                num = [(a - m * b) % p for a, b in zip([0] + num, num + [0])]   # times (X - m)
                den = den * (j - m) % p
        scale = y * pow(den, -1, p) % p
        for i, c in enumerate(num):
            out[i] = (out[i] + scale * c) % p
    return out


class GkrPolynomial(SumcheckPolynomial):
    """f(b, c) of one layer (module docstring) in 2 k_prev variables, held as the two phases' ProductPolynomials.

    layer: a CompiledLayer; w_prev: the MultilinearPolynomial of the layer below (k_prev variables, never modified);
    r: the k challenges the layer's own wires are bound to.  `round_function` takes the whole challenge list; the call with
    k_prev challenges folds the last b-challenge (which leaves wu = W~(u)), runs the phase-2 pass and returns the first
    c-round."""

    def __init__(self, layer, w_prev, r, p):
        if w_prev.p != p or w_prev.num_vars != layer.k_prev or len(r) != layer.k:
            raise ValueError("the table below the layer or the layer's point has the wrong number of variables")
        super().__init__(2 * layer.k_prev, p)
        self.layer, self.w, self.r = layer, w_prev, [int(x) % p for x in r]
        self._ops = FrOps(p)
        self._e = eq_table(self._ops, self.r)
        k = layer.k_prev
        p_tab, q_tab = DevVec(1 << k, zero=False), DevVec(1 << k, zero=False)
        N.check(N.load().zk_gkr_phase1_dev(self._ops.cid, *layer.by_b.args(), layer.k, self._e.ptr(), w_prev.device_ptr(), p_tab.ptr(),
                                           q_tab.ptr(), None))
        cls = MLE_OBJECT[p]
        self.p_table, self.q_table = cls._wrap(k, p_tab), cls._wrap(k, q_tab)
        self.phase1 = ProductPolynomial([self.p_table, w_prev, self.q_table], [(1, (0, 1)), (1, (2,))], p)
        self.phase2, self.u, self.wu = None, None, None
        self.add_table = self.mul_table = None

    def sum(self):
        return self.phase1.sum()

    def first_round(self):
        return self.phase1.first_round()

    def _hand_over(self, u):
        """b is fixed to u: wu from the fold of phase 1's last variable, then the phase-2 pass"""
        k, ops, layer = self.layer.k_prev, self._ops, self.layer
        self.phase1.round_function(u)                       # folds u[-1]: every table of phase 1 is one element now
        self.wu = ops.int_at(self.phase1._cur[1].download(1), 0)
        e2 = eq_table(ops, u)
        a_add, a_mul = DevVec(1 << k, zero=False), DevVec(1 << k, zero=False)
        N.check(N.load().zk_gkr_phase2_dev(ops.cid, *layer.by_c.args(), layer.k, self._e.ptr(), e2.ptr(), a_add.ptr(), a_mul.ptr(), None))
        cls = MLE_OBJECT[self.p]
        self.add_table, self.mul_table = cls._wrap(k, a_add), cls._wrap(k, a_mul)
        self.phase2 = ProductPolynomial([self.add_table, self.w, self.mul_table],
                                        [(self.wu, (0,)), (1, (0, 1)), (self.wu, (2, 1))], self.p)
        self.u = u

    def round_function(self, r):
        r = [int(x) % self.p for x in r]
        k = self.layer.k_prev
        if len(r) > self.n:
            raise ValueError("more challenges than variables")
        if len(r) < k:
            return self.phase1.round_function(r)
        if self.u != r[:k]:
            self._hand_over(r[:k])
        return self.phase2.round_function(r[k:])

    def wiring(self, points):
        """(add~_j(r, u, v), mul~_j(r, u, v)) at points = u + v"""
        k = self.layer.k_prev
        return wiring_eval(self._ops, self.layer, self.r, points[:k], points[k:])

    def evaluate(self, points):
        points = [int(x) % self.p for x in points]
        if len(points) != self.n:
            raise ValueError("Evaluation requires points to be in the same size as the number of variables")
        k = self.layer.k_prev
        add, mul = self.wiring(points)
        wb, wc = self.w.evaluate(points[:k]), self.w.evaluate(points[k:])
        return (add * (wb + wc) + mul * wb * wc) % self.p

    def to_evaluations(self):
        """the non-zero contributions to the sum, one per pair (b, c) that a gate joins, in the order of the index
        (c << k) | b walked b first -- what the reference's to_evaluations returns (gkr.py:29-48); on the host"""
        p, layer = self.p, self.layer
        e = self._ops.ints(self._e.download(1 << layer.k))
        w = self.w.to_evaluations()
        weights = {}
        for a, (t, b, c) in enumerate(zip(layer.types.tolist(), layer.in1.tolist(), layer.in2.tolist())):
            pair = weights.setdefault((b, c), [0, 0])
            pair[t] = (pair[t] + e[a]) % p
        return [(wa * (w[b] + w[c]) + wm * w[b] * w[c]) % p for (b, c), (wa, wm) in sorted(weights.items()) if wa or wm]


def _int_bytes(values):
    """the transcript bytes of a list of ints, as `transcript.append` writes them one by one (transcript.py: big-endian on
    bit_length() BYTES), in one join"""
    return b"".join(v.to_bytes(v.bit_length(), "big") for v in values)


class GKR:
    """prove / verify the evaluation of a LayeredCircuit over the scalar field `field`.

    `input_map`: a dict by input name (named circuits), or a sequence of ints or an (n, 4) uint64 limb array in
    `circuit.inputs` order.  The output is a dict by name for a named circuit and a list in gate order otherwise."""

    polynomial_class = GkrPolynomial   # tools/gkr_bench.py times the phases through a subclass

    def __init__(self, circuit: LayeredCircuit, field=BN254_SCALAR_FIELD):
        self.circuit = circuit
        self.order = field
        self.layers = circuit.compile(field)
        self.depth = len(self.layers)
        self._ops = FrOps(field)
        self.last_trace = None   # per layer of the last prove(), top layer first: {"r", "claim", "challenges"} (tests and tools)

    # -- values in and out --
    def _table(self, values, n, k):
        """(DevVec of 2^k canonical elements, zero beyond n; the n values as ints) from ints or limbs"""
        ops = self._ops
        if isinstance(values, np.ndarray) and values.ndim == 2:
            if values.shape != (n, 4):
                raise ValueError(f"expected an ({n}, 4) limb array")
            vec = ops.d_from(values, 1 << k)
            N.check(N.load().zk_vec_canon_dev(ops.cid, n, vec.ptr(), None))
            return vec, ops.ints(vec.download(n))
        ints = [int(v) % self.order for v in values]
        if len(ints) != n:
            raise ValueError(f"expected {n} values, got {len(ints)}")
        return ops.d_from(ops.limbs(ints), 1 << k), ints

    def _ordered(self, mapping, names, what):
        if isinstance(mapping, dict):
            if not self.circuit.named or set(mapping.keys()) != set(names):
                raise ValueError(f"the {what} map does not name exactly the circuit's {what}s")
            return [mapping[name] for name in names]
        return mapping

    def _inputs(self, input_map):
        n = len(self.circuit.inputs)
        return self._table(self._ordered(input_map, self.circuit.inputs, "input"), n, self.layers[0].k_prev)

    def _start(self, inputs, outputs, transcript):
        transcript = transcript or FiatShamirTranscript(b"gkr", field=self.order)
        transcript.append(_int_bytes(inputs))
        transcript.append(_int_bytes(outputs))
        return transcript

    def evaluate_layers(self, w0):
        """[W_0, .., W_d] as MultilinearPolynomials on the device, from the input table"""
        lib, ops, cls = N.load(), self._ops, MLE_OBJECT[self.order]
        tables = [cls._wrap(self.layers[0].k_prev, w0)]
        for layer in self.layers:
            out = DevVec(1 << layer.k, zero=False)
            N.check(lib.zk_gkr_layer_eval_dev(ops.cid, layer.n, layer.d_types.ptr, layer.d_in1.ptr, layer.d_in2.ptr, layer.k_prev,
                                              tables[-1].device_ptr(), layer.k, out.ptr(), None))
            tables.append(cls._wrap(layer.k, out))
        return tables

    def _line(self, u, v, t):
        return [(a + t * (b - a)) % self.order for a, b in zip(u, v)]

    def _restrict_to_line(self, w, u, v):
        """q(t) = W~(u + t (v - u)): k + 1 evaluations on the device, interpolated here (gkr.py:197-215 recurses over the table)"""
        p = self.order
        return Polynomial(interpolate([w.evaluate(self._line(u, v, t)) for t in range(len(u) + 1)], p), p)

    def prove(self, input_map, transcript=None):
        """(output_map, proofs).  Pass the caller's `transcript` when this runs inside a larger protocol."""
        p, ops = self.order, self._ops
        w0, inputs = self._inputs(input_map)
        tables = self.evaluate_layers(w0)
        last = self.layers[-1]
        outputs = ops.ints(tables[-1].to_limbs()[: last.n])
        transcript = self._start(inputs, outputs, transcript)
        r = [transcript.get_challenge_scalar() for _ in range(last.k)]
        m = tables[-1].evaluate(r)
        proofs, self.last_trace = [], []
        for j in range(self.depth, 0, -1):
            layer, w = self.layers[j - 1], tables[j - 1]
            k = layer.k_prev
            f = self.polynomial_class(layer, w, r, p)
            claim, proof, challenges = Sumcheck(2 * k, p).prove_arbitrary(f, transcript)
            assert claim == m, "Wiring pattern of the circuit might be incorrect"
            u, v = challenges[:k], challenges[k:]
            q = self._restrict_to_line(w, u, v)
            z1, z2 = q(0), q(1)
            assert z1 == f.wu, "the line's start is not what phase 1 folded W down to"
            add, mul = f.wiring(challenges)
            assert (add * (z1 + z2) + mul * z1 * z2) % p == proof[-1](challenges[-1])
            for uni in proof:
                transcript.append(uni.coeffs())
            transcript.append(q.coeffs())
            transcript.append([z1, z2])
            proof.append((q, z1, z2))
            proofs.append(proof)
            self.last_trace.append({"r": r, "claim": claim, "challenges": challenges})
            r_star = transcript.get_challenge_scalar()
            r, m = self._line(u, v, r_star), q(r_star)
        if self.circuit.named:
            return dict(zip(self.circuit.output_names(), outputs)), proofs
        return outputs, proofs

    def verify(self, input_map, output_map, proofs, transcript=None) -> bool:
        p, ops, cls = self.order, self._ops, MLE_OBJECT[self.order]
        last = self.layers[-1]
        try:
            w0, inputs = self._inputs(input_map)
            names = self.circuit.output_names() if self.circuit.named else None
            wd, outputs = self._table(self._ordered(output_map, names, "output"), last.n, last.k)
        except ValueError:
            return False
        if len(proofs) != self.depth:
            return False
        transcript = self._start(inputs, outputs, transcript)
        r = [transcript.get_challenge_scalar() for _ in range(last.k)]
        m = cls._wrap(last.k, wd).evaluate(r)
        for i, j in enumerate(range(self.depth, 0, -1)):
            layer, round_proof = self.layers[j - 1], proofs[i]
            k = layer.k_prev
            if len(round_proof) != 2 * k + 1:
                return False
            challenges = Sumcheck(2 * k, p).verify(m, round_proof[:-1], 2, transcript)
            if not challenges:
                return False
            u, v = challenges[:k], challenges[k:]
            q, z1, z2 = round_proof[-1]
            if q.degree() > k:
                return False
            if q(0) != z1 or q(1) != z2:
                return False
            add, mul = wiring_eval(ops, layer, r, u, v)
            if (add * (z1 + z2) + mul * z1 * z2) % p != round_proof[-2](challenges[-1]):
                return False
            for uni in round_proof[:-1]:
                transcript.append(uni.coeffs())
            transcript.append(q.coeffs())
            transcript.append([z1, z2])
            r_star = transcript.get_challenge_scalar()
            r, m = self._line(u, v, r_star), q(r_star)
        return cls._wrap(self.layers[0].k_prev, w0).evaluate(r) == m


__all__ = ["GKR", "GkrPolynomial", "eq_table", "wiring_eval"]
