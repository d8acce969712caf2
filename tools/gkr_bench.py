#!/usr/bin/env python3
"""GKR prover timings on layered circuits with random mixed wiring (a record for EXPERIMENTS.md, not a gate).

  python tools/gkr_bench.py [--depth 8] [--log-width 20] [--curves BN254 BLS12_381] [--dense-log 10 12] [--reps 3]

Part 1, the sparse prover (subprotocol/gkr.py) on `depth` layers of 2^log_width gates, every input drawn uniformly from the
layer below.  Per layer, from one GKR.prove:
  p1_setup_ms     eq table + the phase-1 pass (P, Q), synchronised
  p1_rounds_ms    the claim and the k b-rounds
  p2_setup_ms     the fold that leaves wu, eq(u, .) + the phase-2 pass (Aadd, Amul), synchronised
  p2_rounds_ms    the k c-rounds
  line_ms         the k + 1 evaluations of W along the line, and the interpolation
  wiring_ms       the three eq tables and the predicate sums of the prover's last-round assertion
  host_ms         time of the sumcheck rounds spent OUTSIDE the round kernel's calls (transcript, interpolation, allocation):
                  every round call synchronises, so the clock around it is device time plus launch and copy-back
and, timed on their own with the device synchronised around each call (minimum over --reps):
  pass1_ms / pass2_ms and their gates per second.  Each gate reads two random 32-byte elements per pass (E[a] and W[c] or
  E2[b]) and 9 bytes of CSR; `gather_GBps` counts the 64 bytes of elements only.
Part 2, the baseline: the dense broadcast ProductPolynomial (four tables of 2^(2k) elements, three terms) -- what the library
could do before the sparse path -- against the sparse GkrPolynomial on the SAME layer at k in --dense-log, where the dense
tables still fit.  Both run Sumcheck.prove_arbitrary; their round polynomials are compared with ==.  The dense tables are
built on the host (not timed as proving time, reported as dense_build_s).
One JSON line per layer and per comparison."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from zksnake_amd import _native as N  # noqa: E402
from zksnake_amd.arithmetization import LayeredCircuit  # noqa: E402
from zksnake_amd.arithmetization.layered_circuit import CompiledLayer  # noqa: E402
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD  # noqa: E402
from zksnake_amd.frvec import DevVec, FrOps  # noqa: E402
from zksnake_amd.mle import MLE_OBJECT  # noqa: E402
from zksnake_amd.subprotocol import GKR, GkrPolynomial, ProductPolynomial, Sumcheck  # noqa: E402
from zksnake_amd.subprotocol import gkr as gkr_module  # noqa: E402
from zksnake_amd.subprotocol import sumcheck as sumcheck_module  # noqa: E402

FIELDS = {"BN254": BN254_SCALAR_FIELD, "BLS12_381": BLS12_381_SCALAR_FIELD}
DENSE_TERMS = [(1, (0, 1)), (1, (0, 2)), (1, (3, 1, 2))]   # A WB + A WC + Mu WB WC over [A, WB, WC, Mu]
_IN_ROUND_KERNEL = [0.0]


def _timed_round(fn):
    def call(*args, **kwargs):
        t0 = time.perf_counter()
        out = fn(*args, **kwargs)
        _IN_ROUND_KERNEL[0] += time.perf_counter() - t0
        return out
    return call


def sync():
    N.check(N.load().zk_dev_synchronize())


class TimedPolynomial(GkrPolynomial):
    log = []   # one dict per layer, appended on construction

    def __init__(self, *args):
        self.t = {"p1_setup": 0.0, "p1_rounds": 0.0, "p2_setup": 0.0, "p2_rounds": 0.0}
        sync()
        t0 = time.perf_counter()
        super().__init__(*args)
        sync()
        self.t["p1_setup"] = time.perf_counter() - t0
        self._kernel0 = _IN_ROUND_KERNEL[0]
        TimedPolynomial.log.append(self)

    def _clock(self, key, fn, *args):
        t0 = time.perf_counter()
        out = fn(*args)
        self.t[key] += time.perf_counter() - t0
        return out

    def sum(self):
        return self._clock("p1_rounds", super().sum)

    def first_round(self):
        return self._clock("p1_rounds", super().first_round)

    def _hand_over(self, u):
        t0, k0 = time.perf_counter(), _IN_ROUND_KERNEL[0]
        super()._hand_over(u)
        sync()
        self.t["p2_setup"] += time.perf_counter() - t0
        self.t["p2_rounds"] -= time.perf_counter() - t0   # it runs inside the first c-round's call
        self._kernel0 += _IN_ROUND_KERNEL[0] - k0         # and its fold is setup, not a round

    def round_function(self, r):
        return self._clock("p1_rounds" if len(r) < self.layer.k_prev else "p2_rounds", super().round_function, r)

    def wiring(self, points):
        if "wiring" not in self.t:   # the rounds are over when the prover asks for the predicates
            self.t["wiring"] = 0.0
            self.kernel_s = _IN_ROUND_KERNEL[0] - self._kernel0
        return self._clock("wiring", super().wiring, points)


class TimedGKR(GKR):
    polynomial_class = TimedPolynomial
    line_s = []

    def _restrict_to_line(self, w, u, v):
        t0 = time.perf_counter()
        q = super()._restrict_to_line(w, u, v)
        TimedGKR.line_s.append(time.perf_counter() - t0)
        return q


def random_limbs(rng, n):
    limbs = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    limbs[:, 3] >>= 4   # below 2^251: canonical in both fields
    limbs[:, 0] |= 1    # and not zero
    return limbs


def random_layer(rng, n_prev, n, distinct_pairs=False):
    types = rng.integers(0, 2, size=n, dtype=np.uint8)
    in1 = rng.integers(0, n_prev, size=n, dtype=np.uint32)
    in2 = rng.integers(0, n_prev, size=n, dtype=np.uint32)
    while distinct_pairs:   # the dense baseline is built by assignment: one gate per (b, c)
        key = in1.astype(np.int64) | (in2.astype(np.int64) << 32)
        _, first = np.unique(key, return_index=True)
        again = np.setdiff1d(np.arange(n), first)
        if again.size == 0:
            break
        in2[again] = rng.integers(0, n_prev, size=again.size, dtype=np.uint32)
    return types, in1, in2


def time_pass(fn, reps):
    best = None
    for _ in range(reps + 1):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    return best


def sparse_run(curve, depth, log_width, reps, rng):
    p = FIELDS[curve]
    ops, lib = FrOps(p), N.ensure_gpu()
    n = 1 << log_width
    t0 = time.perf_counter()
    circuit = LayeredCircuit.from_arrays(n, [random_layer(rng, n, n) for _ in range(depth)])
    gkr = TimedGKR(circuit, p)
    compile_s = time.perf_counter() - t0
    inputs = random_limbs(rng, n)
    TimedPolynomial.log, TimedGKR.line_s = [], []
    t0 = time.perf_counter()
    out, proofs = gkr.prove(inputs)
    prove_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ok = gkr.verify(inputs, out, proofs)
    verify_s = time.perf_counter() - t0
    if not ok:
        raise SystemExit("the proof does not verify")
    print(json.dumps({"curve": curve, "depth": depth, "log_width": log_width, "compile_s": round(compile_s, 3),
                      "prove_s": round(prove_s, 3), "verify_s": round(verify_s, 3)}), flush=True)
    for i, (f, line) in enumerate(zip(TimedPolynomial.log, TimedGKR.line_s)):
        layer, k = f.layer, f.layer.k_prev
        e2 = gkr_module.eq_table(ops, f.u)
        scratch = [DevVec(1 << k, zero=False) for _ in range(2)]
        pass1 = time_pass(lambda: N.check(lib.zk_gkr_phase1_dev(ops.cid, *layer.by_b.args(), layer.k, f._e.ptr(), f.w.device_ptr(),
                                                                scratch[0].ptr(), scratch[1].ptr(), None)), reps)
        pass2 = time_pass(lambda: N.check(lib.zk_gkr_phase2_dev(ops.cid, *layer.by_c.args(), layer.k, f._e.ptr(), e2.ptr(),
                                                                scratch[0].ptr(), scratch[1].ptr(), None)), reps)
        rounds = f.t["p1_rounds"] + f.t["p2_rounds"]
        res = {"curve": curve, "layer": depth - i, "gates": layer.n, "k": layer.k, "k_prev": k,
               "long_rows": [layer.by_b.n_long, layer.by_c.n_long]}
        for key in ("p1_setup", "p1_rounds", "p2_setup", "p2_rounds", "wiring"):
            res[key + "_ms"] = round(f.t[key] * 1e3, 3)
        res["line_ms"] = round(line * 1e3, 3)
        res["host_ms"] = round((rounds - f.kernel_s) * 1e3, 3)
        for label, t in (("pass1", pass1), ("pass2", pass2)):
            res[label + "_ms"] = round(t * 1e3, 4)
            res[label + "_Mgates_per_s"] = round(layer.n / t / 1e6, 1)
            res[label + "_gather_GBps"] = round(64 * layer.n / t / 1e9, 1)
        print(json.dumps(res), flush=True)


def dense_run(curve, k, reps, rng):
    """one layer of 2^k gates over 2^k wires: the four broadcast tables against the sparse polynomial"""
    p = FIELDS[curve]
    ops = FrOps(p)
    n = 1 << k
    types, in1, in2 = random_layer(rng, n, n, distinct_pairs=True)
    layer = CompiledLayer(n, types, in1, in2)
    w = random_limbs(rng, n)
    w_poly = MLE_OBJECT[p].from_evaluations(w, p)
    r = [int(x) for x in rng.integers(1, 1 << 62, size=k)]
    t0 = time.perf_counter()
    e = gkr_module.eq_table(ops, r).download(n)
    index = in1.astype(np.int64) | (in2.astype(np.int64) << k)
    tables = []
    for kind in (0, 1):
        tab = np.zeros((n * n, 4), dtype=np.uint64)
        tab[index[types == kind]] = e[types == kind]
        tables.append(tab)
    host = [tables[0], np.tile(w, (n, 1)), np.repeat(w, n, axis=0), tables[1]]
    polys = [MLE_OBJECT[p].from_evaluations(t, p) for t in host]
    del host, tables
    build_s = time.perf_counter() - t0
    sc = Sumcheck(2 * k, p)
    best = {"dense": None, "sparse": None}
    proofs = {}
    for _ in range(reps + 1):
        for label in ("dense", "sparse"):
            sync()
            t0 = time.perf_counter()
            poly = ProductPolynomial(polys, DENSE_TERMS, p) if label == "dense" else GkrPolynomial(layer, w_poly, r, p)
            claim, proof, challenges = sc.prove_arbitrary(poly)
            dt = time.perf_counter() - t0
            best[label] = dt if best[label] is None or dt < best[label] else best[label]
            proofs[label] = (claim, [u.coeffs() for u in proof], challenges)
    if proofs["dense"] != proofs["sparse"]:
        raise SystemExit("the dense and the sparse prover disagree")
    print(json.dumps({"curve": curve, "compare_k": k, "gates": n, "dense_table_MiB_each": (32 * n * n) >> 20,
                      "dense_build_s": round(build_s, 3), "dense_prove_ms": round(best["dense"] * 1e3, 3),
                      "sparse_prove_ms": round(best["sparse"] * 1e3, 3),
                      "speedup": round(best["dense"] / best["sparse"], 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--log-width", type=int, default=20)
    ap.add_argument("--curves", nargs="+", default=["BN254", "BLS12_381"], choices=list(FIELDS))
    ap.add_argument("--dense-log", type=int, nargs="*", default=[10, 12])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    sumcheck_module.sumcheck_round = _timed_round(sumcheck_module.sumcheck_round)
    rng = np.random.default_rng(11)
    for curve in args.curves:
        sparse_run(curve, args.depth, args.log_width, args.reps, rng)
    for curve in args.curves:
        for k in args.dense_log:
            dense_run(curve, k, args.reps, rng)


if __name__ == "__main__":
    main()
