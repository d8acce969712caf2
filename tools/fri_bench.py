"""FRI polynomial commitment (zksnake_amd/commitment/polynomial/fri.py): wall-clock times of commit, open (from a resident
oracle, and from coefficients) and verify at n = 2^16, 2^20, 2^22 coefficients, blowup 4, 64 queries, on both curves, and the
pieces an opening is made of, each timed on its own between device synchronisations: the low-degree extension, the Merkle tree
of layer 0's size, the chain of folds without trees, the trees of the committed layers, the query gathers (leaves and paths of
every tree), and what is left of the opening's wall time (host: transcript, divisions' scalars, Python).  The fold kernel alone
is timed on the first layer and reported as effective bytes per second: 96 bytes per output (a 64-byte pair read, 32 bytes
written).  KZG commit / open and IPA commit / open are timed in the same run for comparison, up to --compare-max-log (IPA
takes at most 2^21 coefficients; its generators are k_i B as in tools/pcs_bench.py).  Every timed call ends in a
synchronisation or in a result the host waits for, is warmed up once and repeated; the report has the median and the spread.

    python tools/fri_bench.py [--logs 16 20 22] [--curves BN254 BLS12_381] [--repeats 5] [--no-compare] [--compare-max-log 20] [--out FILE]"""

import argparse
import json
import os
import secrets
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from zksnake_amd import _native as N  # noqa: E402
from zksnake_amd.commitment.polynomial import FRI, IPA, KZG  # noqa: E402
from zksnake_amd.commitment.polynomial.fri import _rows, _tree_over  # noqa: E402
from zksnake_amd.device import DeviceBuffer  # noqa: E402
from zksnake_amd.ecc import EllipticCurve  # noqa: E402
from zksnake_amd.frvec import DevVec, FrOps  # noqa: E402

FOLD_BYTES_PER_OUTPUT = 96


def timed(fn, repeats, warm=1):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "repeats": repeats}


def bench_fri(name, log_n, repeats):
    lib = N.load()
    sync = lambda: N.check(lib.zk_dev_synchronize())  # noqa: E731
    fri = FRI(1 << log_n, name)
    fri.setup()
    ops, r = fri._ops, fri.order
    vec = ops.d_from(ops.random_vector(fri.n))
    z = secrets.randbelow(r)
    out = {"blowup": 1 << fri.b, "queries": fri.queries, "final": 1 << fri.f, "folds": fri.folds}
    out["commit"] = timed(lambda: fri.commit(vec), repeats)
    oracle = fri.oracle(vec)
    state = {}

    def run_open(polynomial):
        state["proof"], state["value"] = fri.open(polynomial, z)

    out["open_from_oracle"] = timed(lambda: run_open(oracle), repeats)
    out["open_from_coefficients"] = timed(lambda: run_open(vec), repeats)
    out["verify"] = timed(lambda: fri.verify(oracle.root, state["proof"], z, state["value"]) or sys.exit("verify failed"), repeats)
    out["proof_bytes"] = len(state["proof"].to_bytes())

    # the pieces, each between synchronisations
    def lde():
        fri._extend(vec, vec.n)
        sync()

    def tree0():
        _tree_over(oracle.evals, fri.size // 2).release()

    layers = [oracle.evals] + [DevVec(fri.size >> (l + 1), zero=False) for l in range(fri.folds)]
    scalars = [(N.u64p(ops.one(secrets.randbelow(r))), N.u64p(ops.one(pow(pow(fri._omega0(), 1 << l, r), -1, r)))) for l in range(fri.folds)]

    def fold(l):
        N.check(lib.zk_fri_fold_dev(fri.cid, fri.k + fri.b - l, layers[l].ptr(), scalars[l][0], scalars[l][1], layers[l + 1].ptr(), None))

    def folds():
        for l in range(fri.folds):
            fold(l)
        sync()

    def first_fold():
        fold(0)
        sync()

    def layer_trees():
        for l in range(1, fri.folds):
            _tree_over(layers[l], fri.size >> (l + 1)).release()

    folds()
    trees = [oracle.tree] + [_tree_over(layers[l], fri.size >> (l + 1)) for l in range(1, fri.folds)]
    idx = [secrets.randbelow(fri.size // 2) for _ in range(fri.queries)]

    def gathers():
        for l, tree in enumerate(trees):
            at = np.array([i % tree.n for i in idx], dtype=np.uint64)
            d_idx = DeviceBuffer.from_numpy(at)
            _rows(layers[l].ptr(), tree.n, d_idx, len(idx))
            tree.open_many(at)
            d_idx.free()

    parts = {"lde": timed(lde, repeats), "tree_layer0_size": timed(tree0, repeats), "folds": timed(folds, repeats),
             "layer_trees": timed(layer_trees, repeats), "query_gathers": timed(gathers, repeats), "first_fold": timed(first_fold, repeats)}
    device = sum(parts[key]["median_ms"] for key in ("lde", "folds", "layer_trees", "query_gathers"))
    parts["host_and_divisions_ms"] = round(out["open_from_oracle"]["median_ms"] - device, 3)
    parts["first_fold_effective_GBps"] = round(FOLD_BYTES_PER_OUTPUT * (fri.size // 2) / (parts["first_fold"]["median_ms"] * 1e-3) / 1e9, 1)
    out["parts"] = parts
    for tree in trees[1:]:
        tree.release()
    oracle.release()
    return out


def bench_kzg(name, log_n, repeats):
    n = 1 << log_n
    kzg = KZG(n - 1, name)
    ops, r = FrOps(kzg.order), kzg.order
    kzg.setup(tau=secrets.randbelow(r))
    vec, z = ops.d_from(ops.random_vector(n)), secrets.randbelow(r)
    out = {"commit": timed(lambda: kzg.commit(vec), repeats), "open": timed(lambda: kzg.open(vec, z), repeats)}
    kzg.G1_tau.release()
    return out


def bench_ipa(name, log_n, repeats):
    n = 1 << log_n
    E = EllipticCurve(name)
    ipa = IPA(n, name)
    ops, r = FrOps(ipa.order), ipa.order
    ipa.G = E.batch_mul(E.G1(), ops.random_vector(n), as_array=True)
    ipa.H = E.G1() * secrets.randbelow(r)
    vec, blinding, z = ops.d_from(ops.random_vector(n)), 1 + secrets.randbelow(r - 1), secrets.randbelow(r)
    randomness = ipa.random(multi=True)
    commitment = ipa.commit(vec, blinding)
    out = {"commit": timed(lambda: ipa.commit(vec, blinding), repeats),
           "open": timed(lambda: ipa.open(vec, z, commitment, blinding, randomness=randomness), repeats)}
    ipa.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--curves", nargs="+", default=["BN254", "BLS12_381"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-compare", action="store_true", help="skip KZG and IPA")
    ap.add_argument("--compare-max-log", type=int, default=20, help="largest size at which KZG and IPA are timed too")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("medians of at least 5 runs")
    lib = N.ensure_gpu()
    report = {"library": lib.zk_version().decode(), "results": []}
    for name in args.curves:
        for log_n in args.logs:
            row = {"curve": name, "log_n": log_n, "fri": bench_fri(name, log_n, args.repeats)}
            if not args.no_compare and log_n <= args.compare_max_log:
                row["kzg"] = bench_kzg(name, log_n, args.repeats)
                if log_n <= N.PCS_MAX_LOG:
                    row["ipa"] = bench_ipa(name, log_n, args.repeats)
            report["results"].append(row)
            print(json.dumps(row), flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
