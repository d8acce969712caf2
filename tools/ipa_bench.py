#!/usr/bin/env python3
"""Inner-product argument timings (a record for EXPERIMENTS.md, not a gate).

  python tools/ipa_bench.py [--log-n 12 16 20] [--curves BN254 BLS12_381] [--reps 2] [--hash-up-to 12]

Per curve and size one JSON line:
  setup_s        generators (hashed on the host up to --hash-up-to, else s_i * B from the GPU batch multiplier: hashing 2^21
                 points takes tens of minutes of host time and says nothing about the argument), their compressed bytes, and
                 the MSM plan over G || H (2n bases)
  prove_ms / verify_ms   wall time, minimum over --reps after one warm-up run; prove_serial_ms: the profiled form of prove, which
                 runs the two MSMs of a round one after the other (the default puts them in flight together)
  rounds         of the profiled form, per round k: kernel_ms (zk_ipa_round_dev, host clock around the call, which ends in a synchronise), msm_ms (the
                 two plan runs, total of zk_msm_plan_timings), msm_wall_ms (host clock around them) and host_ms (cross * Q, the
                 transcript, the challenge's inverse)
  late_share     rounds k >= log_n / 2 as a share of all rounds' time: what folding the generators of the late rounds (m small,
                 the unfolded MSM still over n live scalars) could win at most
  composed_ms    log_n <= 12 only: the same proof through entry points that do not know the argument -- the reference's
                 algorithm with folded generators, batch_mul + point additions for the fold and multiexp per round; its bytes
                 are compared with the proof's
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from zksnake_amd import _native as N  # noqa: E402
from zksnake_amd._algebra import PointArray  # noqa: E402
from zksnake_amd.ecc import EllipticCurve  # noqa: E402
from zksnake_amd.subprotocol import InnerProductArgument, InnerProductProof  # noqa: E402
from zksnake_amd.transcript import FiatShamirTranscript, hash_to_curve  # noqa: E402


def random_limbs(rng, n):
    limbs = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    limbs[:, 3] >>= 4   # below 2^251: canonical in both fields
    return limbs


def add_rows(lib, cid, x, y):
    """row-wise point addition of two PointArrays on the host"""
    out = np.zeros_like(x.limbs)
    for i in range(len(x)):
        N.check(lib.zk_point_add(cid, 1, N.u64p(x.limbs[i]), N.u64p(y.limbs[i]), N.u64p(out[i])))
    return PointArray(cid, 1, out)


def composed_prove(E, G, H, a, b):
    """bulletproofs/ipa.py:73-150 over batch_mul, multiexp and point additions; a, b lists of ints"""
    lib, r, n = N.load(), E.order, len(G)
    transcript = FiatShamirTranscript(n.to_bytes(32, "big"), field=r)
    transcript.append(G.to_bytes())
    transcript.append(H.to_bytes())
    commitment = E.multiexp(PointArray(E.curve_id, 1, np.concatenate([G.limbs, H.limbs])), a + b)
    transcript.append(commitment)
    Q = hash_to_curve(transcript.get_challenge(), b"Q", E.name)
    Ls, Rs = [], []
    while n != 1:
        n //= 2
        a_lo, a_hi, b_lo, b_hi = a[:n], a[n:], b[:n], b[n:]
        G_lo, G_hi, H_lo, H_hi = G[:n], G[n:], H[:n], H[n:]
        dot = lambda x, y: sum(p * q for p, q in zip(x, y)) % r  # noqa: E731
        L = E.multiexp(G_hi, a_lo) + E.multiexp(H_lo, b_hi) + Q * dot(a_lo, b_hi)
        R = E.multiexp(G_lo, a_hi) + E.multiexp(H_hi, b_lo) + Q * dot(a_hi, b_lo)
        Ls.append(L)
        Rs.append(R)
        transcript.append(L)
        transcript.append(R)
        u = transcript.get_challenge_scalar()
        ui = pow(u, -1, r)
        a = [(x * u + y * ui) % r for x, y in zip(a_lo, a_hi)]
        b = [(x * ui + y * u) % r for x, y in zip(b_lo, b_hi)]
        G = add_rows(lib, E.curve_id, E.batch_mul(G_lo, [ui] * n, as_array=True), E.batch_mul(G_hi, [u] * n, as_array=True))
        H = add_rows(lib, E.curve_id, E.batch_mul(H_lo, [u] * n, as_array=True), E.batch_mul(H_hi, [ui] * n, as_array=True))
    return InnerProductProof(a[0], b[0], Ls, Rs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--curves", nargs="+", default=["BN254", "BLS12_381"])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--hash-up-to", type=int, default=12)
    args = ap.parse_args()
    N.ensure_gpu()
    rng = np.random.default_rng(11)
    for curve in args.curves:
        E = EllipticCurve(curve)
        for log_n in args.log_n:
            n = 1 << log_n
            t0 = time.perf_counter()
            if log_n <= args.hash_up_to:
                ipa, gens = InnerProductArgument(n, curve), "hashed"
            else:
                G = E.batch_mul(E.G1(), random_limbs(rng, n), as_array=True)
                H = E.batch_mul(E.G1(), random_limbs(rng, n), as_array=True)
                ipa, gens = InnerProductArgument(n, curve, generators=(G, H)), "batch_mul"
            t1 = time.perf_counter()
            ipa._gens.bytes()
            t2 = time.perf_counter()
            ipa._gens.bases().plan()
            N.load().zk_dev_synchronize()
            t3 = time.perf_counter()
            a, b = random_limbs(rng, n), random_limbs(rng, n)
            prove_t, serial_t, verify_t, rounds = [], [], [], None
            for rep in range(args.reps + 1):   # the first repetition warms up
                t = time.perf_counter()
                proof, com, ab = ipa.prove(a, b)
                prove_t.append(time.perf_counter() - t)
                t = time.perf_counter()
                profiled = ipa.prove(a, b, profile=True)
                serial_t.append(time.perf_counter() - t)
                if profiled[0].to_bytes() != proof.to_bytes():
                    raise SystemExit("the profiled run gives another proof")
                if rep and serial_t[-1] <= min(serial_t[1:]):
                    rounds = ipa.last_profile
                t = time.perf_counter()
                ok = ipa.verify(proof, com, ab)
                verify_t.append(time.perf_counter() - t)
                if not ok:
                    raise SystemExit("the proof does not verify")
            per = [r["kernel_ms"] + r["msm_wall_ms"] + r["host_ms"] for r in rounds]
            res = {"curve": curve, "log_n": log_n, "generators": gens, "setup_generators_s": round(t1 - t0, 3),
                   "setup_bytes_s": round(t2 - t1, 3), "setup_plan_s": round(t3 - t2, 3), "setup_s": round(t3 - t0, 3),
                   "prove_ms": round(min(prove_t[1:]) * 1e3, 3), "prove_serial_ms": round(min(serial_t[1:]) * 1e3, 3), "verify_ms": round(min(verify_t[1:]) * 1e3, 3),
                   "rounds_ms": round(sum(per), 3), "kernel_ms": round(sum(r["kernel_ms"] for r in rounds), 3),
                   "msm_ms": round(sum(r["msm_ms"] for r in rounds), 3), "msm_wall_ms": round(sum(r["msm_wall_ms"] for r in rounds), 3),
                   "host_ms": round(sum(r["host_ms"] for r in rounds), 3),
                   "late_share": round(sum(per[(log_n + 1) // 2:]) / sum(per), 3),
                   "rounds": [{k: round(v, 3) for k, v in r.items()} for r in rounds]}
            if log_n <= 12:
                la, lb = N.limbs_to_ints(a), N.limbs_to_ints(b)
                t = time.perf_counter()
                other = composed_prove(E, ipa.G, ipa.H, la, lb)
                res["composed_ms"] = round((time.perf_counter() - t) * 1e3, 3)
                if other.to_bytes() != proof.to_bytes():
                    raise SystemExit("the composed path gives another proof")
            print(json.dumps(res), flush=True)
            ipa.release()
            del ipa


if __name__ == "__main__":
    main()
