#!/usr/bin/env python3
"""Range-proof timings (a record for EXPERIMENTS.md, not a gate).

  python tools/range_proof_bench.py [--bitsize 64] [--values 1 16 1024 16384] [--curves BN254 BLS12_381] [--reps 2]

Generators are s_i * P from the GPU batch multiplier: hashing 2^21 points takes minutes of host time and says nothing about
the proof.  Per curve and number of values one JSON line:
  setup_s        generators, their digest (compressed bytes + blake2b) and the MSM plan over G || H (2N bases)
  random_ms      drawing s_L, s_R (2N scalars, uniform below r, from the OS CSPRNG) and the blinding factors: reported on its
                 own, and NOT part of prove_ms (the randomness is handed in)
  prove_ms / verify_ms   wall time, minimum over --reps after one warm-up run
  the profiled form of prove (device synchronised between parts, the two MSMs of a round one after the other), split into
    kernels_ms     zk_rp_bits_dev + zk_rp_poly_dev + zk_rp_eval_dev (each on its own under bits/poly/eval_kernel_ms)
    msm_pair_ms    A and S in flight together, and their blinding terms
    rounds_ms      the inner-product rounds (round kernels + MSM pairs + host), as tools/ipa_bench.py splits them
    host_ms        V_j, T1, T2, Q, the transcript and the scalars between the parts; upload_ms: values and s_L, s_R to HBM
  ipa_prove_ms / ipa_verify_ms   the inner-product argument alone over the same generators and the same l, r sizes: what a
                 range proof adds is prove_ms - ipa_prove_ms
  composed_ms    values <= 16 only: the same proof through entry points that do not know the protocol, as the reference
                 composes it -- multiexp for A and S, batch_mul for H' = y^-k H, list arithmetic for l, r and t(X), and the
                 folded-generator argument of tools/ipa_bench.py; its bytes are compared with the proof's
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tools.ipa_bench import add_rows, random_limbs  # noqa: E402
from zksnake_amd import _native as N  # noqa: E402
from zksnake_amd._algebra import PointArray  # noqa: E402
from zksnake_amd.ecc import EllipticCurve  # noqa: E402
from zksnake_amd.subprotocol import InnerProductArgument, InnerProductProof, RangeProof, RangeProofObject  # noqa: E402
from zksnake_amd.transcript import FiatShamirTranscript  # noqa: E402


def composed_prove(rp, values, rnd):
    """range_proof.py:108-212 for m values over multiexp, batch_mul and point additions, with this project's transcript"""
    E, r, n, m = rp.E, rp.E.order, rp.n, rp.m
    lib, size = N.load(), rp.n * rp.m
    transcript = FiatShamirTranscript(n.to_bytes(32, "big") + (m.to_bytes(32, "big") if m > 1 else b""), field=r)
    a_l = [(values[k // n] >> (k % n)) & 1 for k in range(size)]
    a_r = [(x - 1) % r for x in a_l]
    s_l, s_r = N.limbs_to_ints(rnd["s_L"]), N.limbs_to_ints(rnd["s_R"])
    V = [rp.B * v + rp.B_blinding * g for v, g in zip(values, rnd["v_blinding"])]
    A = E.multiexp(rp.G, a_l) + E.multiexp(rp.H, a_r) + rp.B_blinding * rnd["a_blinding"]
    S = E.multiexp(rp.G, s_l) + E.multiexp(rp.H, s_r) + rp.B_blinding * rnd["s_blinding"]
    for p in V + [A, S]:
        transcript.append(p)
    y, z = transcript.get_challenge_scalar(), transcript.get_challenge_scalar()
    l0, l1, r0, r1 = [], [], [], []
    exp_y = 1
    for k in range(size):
        l0.append((a_l[k] - z) % r)
        l1.append(s_l[k])
        r0.append((exp_y * (a_r[k] + z) + pow(z, 2 + k // n, r) * (1 << (k % n))) % r)
        r1.append(exp_y * s_r[k] % r)
        exp_y = exp_y * y % r
    dot = lambda p, q: sum(u * v for u, v in zip(p, q)) % r  # noqa: E731
    t0, t2 = dot(l0, r0), dot(l1, r1)
    t1 = (dot([p + q for p, q in zip(l0, l1)], [p + q for p, q in zip(r0, r1)]) - t0 - t2) % r
    T1 = rp.B * t1 + rp.B_blinding * rnd["t1_blinding"]
    T2 = rp.B * t2 + rp.B_blinding * rnd["t2_blinding"]
    transcript.append(T1)
    transcript.append(T2)
    x = transcript.get_challenge_scalar()
    a = [(p + x * q) % r for p, q in zip(l0, l1)]
    b = [(p + x * q) % r for p, q in zip(r0, r1)]
    t = (t0 + t1 * x + t2 * x * x) % r
    t_blinding = (sum(pow(z, 2 + j, r) * g for j, g in enumerate(rnd["v_blinding"])) + rnd["t1_blinding"] * x + rnd["t2_blinding"] * x * x) % r
    e_blinding = (rnd["a_blinding"] + x * rnd["s_blinding"]) % r
    for item in (t, t_blinding, e_blinding):
        transcript.append(item)
    Q = rp.B * transcript.get_challenge_scalar()
    transcript.append(rp._generator_digest())
    G = rp.G
    H = E.batch_mul(rp.H, [pow(y, -k, r) for k in range(size)], as_array=True)
    Ls, Rs, half = [], [], size
    while half != 1:
        half //= 2
        a_lo, a_hi, b_lo, b_hi = a[:half], a[half:], b[:half], b[half:]
        G_lo, G_hi, H_lo, H_hi = G[:half], G[half:], H[:half], H[half:]
        L = E.multiexp(G_hi, a_lo) + E.multiexp(H_lo, b_hi) + Q * dot(a_lo, b_hi)
        R = E.multiexp(G_lo, a_hi) + E.multiexp(H_hi, b_lo) + Q * dot(a_hi, b_lo)
        Ls.append(L)
        Rs.append(R)
        transcript.append(L)
        transcript.append(R)
        u = transcript.get_challenge_scalar()
        ui = pow(u, -1, r)
        a = [(p * u + q * ui) % r for p, q in zip(a_lo, a_hi)]
        b = [(p * ui + q * u) % r for p, q in zip(b_lo, b_hi)]
        G = add_rows(lib, E.curve_id, E.batch_mul(G_lo, [ui] * half, as_array=True), E.batch_mul(G_hi, [u] * half, as_array=True))
        H = add_rows(lib, E.curve_id, E.batch_mul(H_lo, [u] * half, as_array=True), E.batch_mul(H_hi, [ui] * half, as_array=True))
    return RangeProofObject(V[0] if m == 1 else V, A, S, T1, T2, t, t_blinding, e_blinding, InnerProductProof(a[0], b[0], Ls, Rs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bitsize", type=int, default=64)
    ap.add_argument("--values", type=int, nargs="+", default=[1, 16, 1024, 16384])
    ap.add_argument("--curves", nargs="+", default=["BN254", "BLS12_381"])
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    N.ensure_gpu()
    rng = np.random.default_rng(13)
    for curve in args.curves:
        E = EllipticCurve(curve)
        for m in args.values:
            size = args.bitsize * m
            t0 = time.perf_counter()
            G = E.batch_mul(E.G1(), random_limbs(rng, size), as_array=True)
            H = E.batch_mul(E.G1(), random_limbs(rng, size), as_array=True)
            rp = RangeProof(args.bitsize, curve, values=m, generators=(G, H))
            t1 = time.perf_counter()
            rp._generator_digest()
            t2 = time.perf_counter()
            rp._ipa._gens.bases().plan()
            N.load().zk_dev_synchronize()
            t3 = time.perf_counter()
            values = [int(v) for v in rng.integers(0, 1 << 63, size=m, dtype=np.uint64)] if args.bitsize >= 63 else \
                [int(v) % (1 << args.bitsize) for v in rng.integers(0, 1 << 62, size=m, dtype=np.uint64)]
            random_t, prove_t, verify_t, profile_t, profile = [], [], [], [], None
            for rep in range(args.reps + 1):   # the first repetition warms up
                t = time.perf_counter()
                rnd = rp.random()
                random_t.append(time.perf_counter() - t)
                t = time.perf_counter()
                proof = rp.prove(values if m > 1 else values[0], randomness=rnd)
                prove_t.append(time.perf_counter() - t)
                t = time.perf_counter()
                profiled = rp.prove(values if m > 1 else values[0], randomness=rnd, profile=True)
                profile_t.append(time.perf_counter() - t)
                if profiled.to_bytes() != proof.to_bytes():
                    raise SystemExit("the profiled run gives another proof")
                if rep and profile_t[-1] <= min(profile_t[1:]):
                    profile = rp.last_profile
                t = time.perf_counter()
                ok = rp.verify(proof)
                verify_t.append(time.perf_counter() - t)
                if not ok:
                    raise SystemExit("the proof does not verify")
            part = {k: round(v, 3) for k, v in profile.items() if k != "rounds"}
            res = {"curve": curve, "bitsize": args.bitsize, "values": m, "log_N": size.bit_length() - 1,
                   "setup_generators_s": round(t1 - t0, 3), "setup_digest_s": round(t2 - t1, 3), "setup_plan_s": round(t3 - t2, 3),
                   "random_ms": round(min(random_t[1:]) * 1e3, 3), "prove_ms": round(min(prove_t[1:]) * 1e3, 3),
                   "prove_profiled_ms": round(min(profile_t[1:]) * 1e3, 3), "verify_ms": round(min(verify_t[1:]) * 1e3, 3),
                   "kernels_ms": round(part["bits_kernel_ms"] + part["poly_kernel_ms"] + part["eval_kernel_ms"], 3)}
            res.update({k: v for k, v in part.items() if k != "random_ms"})
            res["round_kernels_ms"] = round(sum(r["kernel_ms"] for r in profile["rounds"]), 3)
            # the inner-product argument alone, over the same plan
            ipa = InnerProductArgument(size, curve, generators=(rp.G, rp.H))
            a, b = random_limbs(rng, size), random_limbs(rng, size)
            ipa_p, ipa_v = [], []
            for rep in range(args.reps + 1):
                t = time.perf_counter()
                got = ipa.prove(a, b)
                ipa_p.append(time.perf_counter() - t)
                t = time.perf_counter()
                ipa.verify(*got)
                ipa_v.append(time.perf_counter() - t)
            res["ipa_prove_ms"], res["ipa_verify_ms"] = round(min(ipa_p[1:]) * 1e3, 3), round(min(ipa_v[1:]) * 1e3, 3)
            ipa.release()
            del ipa
            if m <= 16:
                t = time.perf_counter()
                other = composed_prove(rp, values, rnd)
                res["composed_ms"] = round((time.perf_counter() - t) * 1e3, 3)
                if other.to_bytes() != proof.to_bytes():
                    raise SystemExit("the composed path gives another proof")
            print(json.dumps(res), flush=True)
            rp.release()
            del rp


if __name__ == "__main__":
    main()
