"""Polynomial commitments (zksnake_amd/commitment/polynomial): wall-clock times of KZG commit / open, IPA commit / open / verify
(an opening also split per round into kernel, MSM pair and host) and multi_open / multi_verify for 8 polynomials over 3
points, at n = 2^12, 2^16, 2^20 coefficients on both curves.  Every timed call ends in work the host waits for (an MSM result
or a sum comes back), is warmed up once, and is repeated; the report has the median and the spread (min, max).

At 2^12 the same operations are also timed as a user of the parent commit would have composed them from its public entry
points (--compose, on by default at that size only): host `Polynomial` arithmetic, `EllipticCurve.multiexp` over lists of scalars,
and point additions that fold G every round.

    python tools/pcs_bench.py [--logs 12 16 20] [--curves BN254 BLS12_381] [--repeats 5] [--out FILE]

The IPA generators are k_i B for random k_i (batch_mul), not hashed: hashing 2^20 points on the host takes minutes and does not
change what an opening costs."""

import argparse
import json
import os
import secrets
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zksnake_amd import _native as N  # noqa: E402
from zksnake_amd.commitment.polynomial import IPA, KZG, MultiOpeningQuery  # noqa: E402
from zksnake_amd.ecc import EllipticCurve  # noqa: E402
from zksnake_amd.frvec import FrOps  # noqa: E402
from zksnake_amd.polynomial import Polynomial  # noqa: E402
from zksnake_amd.transcript import FiatShamirTranscript, hash_to_curve  # noqa: E402
from zksnake_amd.utils import inner_product  # noqa: E402

COMPOSE_LOG = 12
POINTS_OF = ((0,), (0,), (0,), (0,), (0, 1), (0, 1), (1, 2), (1, 2))   # 8 polynomials over 3 points, 3 groups


def timed(fn, repeats, warm=1):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "repeats": repeats}


def multi_query(scheme, vecs, commitments, points, blindings=None):
    query = MultiOpeningQuery()
    for i, vec in enumerate(vecs):
        query.add_polynomial(vec, commitments[i], None if blindings is None else blindings[i])
    for i, vec in enumerate(vecs):
        for k in POINTS_OF[i]:
            query.prover_query(vec, points[k])
    return query


def bench_kzg(name, log_n, repeats):
    n = 1 << log_n
    kzg = KZG(n - 1, name)
    ops, r = FrOps(kzg.order), kzg.order
    t0 = time.perf_counter()
    kzg.setup(tau=secrets.randbelow(r))
    out = {"setup_ms": round((time.perf_counter() - t0) * 1e3, 1)}
    vecs = [ops.d_from(ops.random_vector(n)) for _ in range(8)]
    z = secrets.randbelow(r)
    out["commit"] = timed(lambda: kzg.commit(vecs[0]), repeats)
    out["open"] = timed(lambda: kzg.open(vecs[0], z), repeats)
    commitments = [kzg.commit(v) for v in vecs]
    points = [secrets.randbelow(r) for _ in range(3)]
    state = {}

    def run_open():
        state["proof"], state["query"] = kzg.multi_open(multi_query(kzg, vecs, commitments, points))

    out["multi_open"] = timed(run_open, repeats)
    out["multi_verify"] = timed(lambda: kzg.multi_verify(state["query"], state["proof"]) or sys.exit("multi_verify failed"), repeats)
    return out, kzg


def bench_ipa(name, log_n, repeats):
    n = 1 << log_n
    E = EllipticCurve(name)
    ipa = IPA(n, name)
    ops, r = FrOps(ipa.order), ipa.order
    ipa.G = E.batch_mul(E.G1(), ops.random_vector(n), as_array=True)
    ipa.H = E.G1() * secrets.randbelow(r)
    vecs = [ops.d_from(ops.random_vector(n)) for _ in range(8)]
    blindings = [1 + secrets.randbelow(r - 1) for _ in vecs]
    z = secrets.randbelow(r)
    randomness = ipa.random(multi=True)
    out = {"commit": timed(lambda: ipa.commit(vecs[0], blindings[0]), repeats)}
    commitment = ipa.commit(vecs[0], blindings[0])
    state = {}

    def run_open():
        state["proof"], state["value"] = ipa.open(vecs[0], z, commitment, blindings[0], randomness=randomness)

    out["open"] = timed(run_open, repeats)
    out["verify"] = timed(lambda: ipa.verify(commitment, state["proof"], z, state["value"]) or sys.exit("verify failed"), repeats)
    ipa.open(vecs[0], z, commitment, blindings[0], randomness=randomness, profile=True)
    rounds = ipa.last_profile
    out["open_rounds"] = {key: round(sum(x[key] for x in rounds), 3) for key in ("kernel_ms", "msm_wall_ms", "msm_ms", "host_ms")}
    out["open_rounds"]["rounds"] = len(rounds)
    commitments = [ipa.commit(v, t) for v, t in zip(vecs, blindings)]
    points = [secrets.randbelow(r) for _ in range(3)]

    def run_multi():
        state["mproof"], state["query"] = ipa.multi_open(multi_query(ipa, vecs, commitments, points, blindings), randomness=randomness)

    out["multi_open"] = timed(run_multi, repeats)
    out["multi_verify"] = timed(lambda: ipa.multi_verify(state["query"], state["mproof"]) or sys.exit("multi_verify failed"), repeats)
    return out, ipa


# ---- the same operations from the parent commit's public entry points -----------------------------------------------------
def composed_kzg(kzg, repeats):
    E, r = kzg.E, kzg.order
    coeffs = [secrets.randbelow(r) for _ in range(kzg.degree + 1)]
    poly = Polynomial(coeffs, r)
    z = secrets.randbelow(r)

    def open_():
        value = poly(z)
        quotient, _ = (poly - value) / Polynomial([-z % r, 1], r)
        return E.multiexp(kzg.G1_tau, quotient.coeffs()), value

    return {"commit": timed(lambda: E.multiexp(kzg.G1_tau, poly.coeffs()), repeats), "open": timed(open_, repeats)}


def composed_ipa(ipa, repeats):
    E, r, n = ipa.E, ipa.order, ipa.n
    G, H = ipa.G.to_list(), ipa.H
    bases = ipa.G.to_list() + [H]
    coeffs = [secrets.randbelow(r) for _ in range(n)]
    blinding, z = 1 + secrets.randbelow(r - 1), secrets.randbelow(r)
    commit = lambda: E.multiexp(bases, coeffs + [blinding])  # noqa: E731
    commitment = commit()
    state = {}

    def start(t, value, c_bar=None):
        t.append(G)
        t.append(H)
        t.append(z)
        t.append(value)
        t.append(commitment)

    def open_():
        poly = Polynomial(coeffs, r)
        value = poly(z)
        t = FiatShamirTranscript(b"IPA-PCS", r)
        start(t, value)
        rand = Polynomial([secrets.randbelow(r) for _ in range(n)], r)
        a_bar = (rand - rand(z)).coeffs()
        a_bar += [0] * (n - len(a_bar))
        t_bar = 1 + secrets.randbelow(r - 1)
        c_bar = E.multiexp(bases, a_bar + [t_bar])
        t.append(c_bar)
        alpha = t.get_challenge_scalar()
        c = [(x + alpha * y) % r for x, y in zip(coeffs, a_bar)]
        c_prime = E.multiexp(G, c)
        t.append(c_prime)
        h_prime = hash_to_curve(t.get_challenge(), b"U", E.name, 1)
        t.append(c_prime + h_prime * value)
        b = [pow(z, i, r) for i in range(n)]
        g, Ls, Rs, m = list(G), [], [], n
        while m > 1:
            m //= 2
            L = E.multiexp(g[:m], c[m:]) + h_prime * inner_product(c[m:], b[:m], r)
            R = E.multiexp(g[m:], c[:m]) + h_prime * inner_product(c[:m], b[m:], r)
            Ls.append(L)
            Rs.append(R)
            t.append(L)
            t.append(R)
            u = t.get_challenge_scalar()
            ui = pow(u, -1, r)
            c = [(x + y * ui) % r for x, y in zip(c[:m], c[m:])]
            b = [(x + y * u) % r for x, y in zip(b[:m], b[m:])]
            g = [x + y * u for x, y in zip(g[:m], g[m:])]          # the fold of G: m scalar multiplications and additions
        state["proof"], state["value"] = [Ls, Rs, c_bar, c[0], (blinding + alpha * t_bar) % r], value

    def verify_():
        Ls, Rs, c_bar, c, t_prime = state["proof"]
        value = state["value"]
        t = FiatShamirTranscript(b"IPA-PCS", r)
        start(t, value)
        t.append(c_bar)
        alpha = t.get_challenge_scalar()
        c_prime = commitment + c_bar * alpha - H * t_prime
        t.append(c_prime)
        h_prime = hash_to_curve(t.get_challenge(), b"U", E.name, 1)
        C = c_prime + h_prime * value
        t.append(C)
        us = []
        for L, R in zip(Ls, Rs):
            t.append(L)
            t.append(R)
            u = t.get_challenge_scalar()
            us.append(u)
            C = L * pow(u, -1, r) + C + R * u
        g = Polynomial([1], r)
        for i in range(len(us)):
            g = g * Polynomial([1] + [0] * (2 ** i - 1) + [us[len(us) - 1 - i]], r)
        gc = g.coeffs()
        b = inner_product([pow(z, i, r) for i in range(n)], gc, r)
        if C != E.multiexp(G, gc) * c + h_prime * (c * b % r):
            sys.exit("composed verify failed")

    return {"commit": timed(commit, repeats), "open": timed(open_, repeats), "verify": timed(verify_, repeats)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--curves", nargs="+", default=["BN254", "BLS12_381"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-compose", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    lib = N.ensure_gpu()
    report = {"library": lib.zk_version().decode(), "results": []}
    for name in args.curves:
        for log_n in args.logs:
            row = {"curve": name, "log_n": log_n}
            row["kzg"], kzg = bench_kzg(name, log_n, args.repeats)
            row["ipa"], ipa = bench_ipa(name, log_n, args.repeats)
            if log_n == COMPOSE_LOG and not args.no_compose:
                row["composed_from_parent_entry_points"] = {"kzg": composed_kzg(kzg, max(args.repeats // 2, 1)),
                                                            "ipa": composed_ipa(ipa, max(args.repeats // 2, 1))}
            kzg.G1_tau.release()
            ipa.release()
            report["results"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
