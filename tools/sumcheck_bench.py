#!/usr/bin/env python3
"""Sumcheck and multilinear fix timings (a record for EXPERIMENTS.md, not a gate).

  python tools/sumcheck_bench.py [--log-n 20 24] [--curve BN254] [--reps 3]

Per size, on two random tables A, B and f = A*B (degree 2):
  prove       Sumcheck.prove_arbitrary end to end (transcript, host interpolation, one fused kernel per round)
  fused       the same rounds as bare library calls: round 1 without a challenge, then one fused fold-and-sum call per round
  unfused     the comparison: per round one fix call (k = 1) per table, then the round call without a challenge
  fix_all     one fix call with k = log_n on one table
Every call ends in a synchronise (the results come back to the host), so host clocks around the calls time the device work
plus the launch and copy-back overhead.  "table bytes" are the bytes the tables of a round hold (2 * 2^m * 32); the rate is
those bytes over the round's time -- an effective figure, not a count of the traffic (the fused round also writes half of
them back; the unfused round reads the folded half again).  fused and unfused alternate inside one process and the minimum
over --reps is printed; their s(0..3) are compared with ==."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from zksnake_amd import _native as N  # noqa: E402
from zksnake_amd.constant import BLS12_381_SCALAR_FIELD, BN254_SCALAR_FIELD  # noqa: E402
from zksnake_amd.frvec import DevVec, FrOps  # noqa: E402
from zksnake_amd.mle import MLE_OBJECT, sumcheck_round  # noqa: E402
from zksnake_amd.subprotocol import ProductPolynomial, Sumcheck  # noqa: E402

TERMS = [(1, (0, 1))]


def random_table(rng, n):
    limbs = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    limbs[:, 3] >>= 4   # below 2^251: canonical in both fields
    return limbs


def rounds_fused(ops, log_n, src, bufs, rs):
    """-> ([s per round], [seconds per round]); bufs: per level the two output vectors"""
    out_s, out_t = [], []
    cur = src
    for i in range(log_n):
        t0 = time.perf_counter()
        if i == 0:
            s = sumcheck_round(ops, log_n, cur, TERMS)
        else:
            nxt = [v.ptr() for v in bufs[i]]
            s = sumcheck_round(ops, log_n - i + 1, cur, TERMS, rs[i - 1], nxt)
            cur = nxt
        out_t.append(time.perf_counter() - t0)
        out_s.append(s)
    return out_s, out_t


def rounds_unfused(ops, lib, log_n, src, bufs, rs):
    out_s, out_t = [], []
    cur = src
    for i in range(log_n):
        t0 = time.perf_counter()
        if i:
            nxt = [v.ptr() for v in bufs[i]]
            r = N.u64p(ops.one(rs[i - 1]))
            for a, b in zip(cur, nxt):
                N.check(lib.zk_mle_fix_dev(ops.cid, log_n - i + 1, a, 1, r, b, None))
            cur = nxt
        s = sumcheck_round(ops, log_n - i, cur, TERMS)
        out_t.append(time.perf_counter() - t0)
        out_s.append(s)
    return out_s, out_t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--curve", default="BN254")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    p = {"BN254": BN254_SCALAR_FIELD, "BLS12_381": BLS12_381_SCALAR_FIELD}[args.curve]
    ops = FrOps(p)
    lib = N.ensure_gpu()
    rng = np.random.default_rng(7)
    for log_n in args.log_n:
        n = 1 << log_n
        polys = [MLE_OBJECT[p].from_evaluations(random_table(rng, n), p) for _ in range(2)]
        src = [m.device_ptr() for m in polys]
        rs = [int(x) for x in rng.integers(1, 1 << 62, size=log_n)]
        bufs = [None] + [[DevVec(n >> i, zero=False) for _ in range(2)] for i in range(1, log_n)]
        best = {}
        s_ref = None
        for rep in range(args.reps + 1):   # the first repetition warms up
            for label, fn in (("fused", lambda: rounds_fused(ops, log_n, src, bufs, rs)),
                              ("unfused", lambda: rounds_unfused(ops, lib, log_n, src, bufs, rs))):
                s, t = fn()
                if s_ref is None:
                    s_ref = s
                if s != s_ref:
                    raise SystemExit(f"{label}: round sums differ from the first run")
                if rep and (label not in best or sum(t) < sum(best[label])):
                    best[label] = t
        # fix of every variable of one table
        one = DevVec(1, zero=False)
        pts = N.u64p(ops.limbs(rs))
        fix_t = []
        for rep in range(args.reps + 1):
            lib.zk_dev_synchronize()
            t0 = time.perf_counter()
            N.check(lib.zk_mle_fix_dev(ops.cid, log_n, src[0], log_n, pts, one.ptr(), None))
            lib.zk_dev_synchronize()
            fix_t.append(time.perf_counter() - t0)
        # the protocol end to end
        sc = Sumcheck(log_n, p)
        prove_t = []
        for rep in range(args.reps + 1):
            poly = ProductPolynomial(polys, TERMS, p)
            t0 = time.perf_counter()
            claim, proof, challenges = sc.prove_arbitrary(poly)
            prove_t.append(time.perf_counter() - t0)
        if sc.verify(claim, proof, 2, mlpoly=poly) != challenges:
            raise SystemExit("the proof does not verify")
        table_bytes = [2 * 32 * (n >> i) for i in range(log_n)]
        res = {"curve": args.curve, "log_n": log_n, "tables": 2, "degree": 2, "reps": args.reps,
               "prove_ms": round(min(prove_t[1:]) * 1e3, 3), "prove_ms_per_round": round(min(prove_t[1:]) * 1e3 / log_n, 4),
               "fix_all_ms": round(min(fix_t[1:]) * 1e3, 3), "fix_all_table_GBps": round(32 * n / min(fix_t[1:]) / 1e9, 1)}
        for label, t in best.items():
            res[label + "_total_ms"] = round(sum(t) * 1e3, 3)
            res[label + "_ms_per_round"] = round(sum(t) * 1e3 / log_n, 4)
            res[label + "_first_rounds_ms"] = [round(x * 1e3, 3) for x in t[:4]]
            res[label + "_round2_table_GBps"] = round(table_bytes[0] / t[1] / 1e9, 1)   # round 2 folds and sums the full tables
            res[label + "_total_table_GBps"] = round(sum(table_bytes) / sum(t) / 1e9, 1)
        print(json.dumps(res), flush=True)
        del polys, bufs, src


if __name__ == "__main__":
    main()
