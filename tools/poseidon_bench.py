"""Poseidon on the GPU (csrc/poseidon.hip): wall-clock times of the width-3 permutation over 2^20 and 2^24 states, of the tree
build over 2^20 and 2^24 leaves beside the BLAKE2b tree at the same n, and of one host `Poseidon.hash` in Python integers.

    python tools/poseidon_bench.py [--logs 20 24] [--curves BN254] [--repeats 7] [--out FILE]

Every timed call is warmed up once and ends in a device synchronisation; a sample is as many calls as it takes to fill about 50 ms,
and the report has the median and the spread (min, max) of `--repeats` (at least 5) samples, per call.

Rates.  permutations/s is n over the median.  field products/s counts the PLAIN form of the permutation, 8 (3 t + t^2) +
R_P (3 + t^2) Montgomery products (828 at t = 3), whatever the kernel does: it sums the t products of a matrix row in one
reduction, which is fewer multiply-adds than t products, so this rate may exceed the ceiling.  The ceiling beside it is the rate of
dependent `fp_mul` chains on 9 limbs at 8 waves per SIMD from the project's microbenchmark (tools/ubench.hip, recorded in
profiles/r01b_ubench_field29.log); the kernels run 1 or 2 waves per SIMD and their table reads come on top.
"""

import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zksnake_amd import _native as N  # noqa: E402
from zksnake_amd.commitment.vector._tree import _layout  # noqa: E402
from zksnake_amd.device import DeviceBuffer  # noqa: E402
from zksnake_amd.hash import Poseidon  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_P = {3: 57, 4: 56, 5: 60}


def plain_products(t):
    return 8 * (3 * t + t * t) + R_P[t] * (3 + t * t)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def timed(fn, repeats, window_ms=50.0):
    """fn ends in a synchronisation.  One warm-up call, which also sizes a sample: enough calls for about window_ms"""
    fn()
    t0 = time.perf_counter()
    fn()
    once = (time.perf_counter() - t0) * 1e3
    inner = max(1, min(200, int(window_ms / max(once, 1e-3))))
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        ms.append((time.perf_counter() - t0) * 1e3 / inner)
    out = stats(ms)
    out["calls_per_sample"] = inner
    return out


def ubench_ceiling():
    """the best fp_mul rate on 9 limbs (BnFq) in the recorded microbenchmark, in products/s; None when the log is not there"""
    try:
        with open(os.path.join(ROOT, "profiles", "r01b_ubench_field29.log")) as f:
            rates = [float(m.group(1)) for m in re.finditer(r"^fp_mul BnFq\s+waves/SIMD=\d+\s+[\d.]+ ms\s+([\d.]+) Gop/s", f.read(), re.M)]
        return max(rates) * 1e9 if rates else None
    except OSError:
        return None


def fill(buf, elems, seed):
    """canonical elements of both fields, the same 2^20 random ones over and over: no kernel here branches on its data"""
    rng = np.random.default_rng(seed)
    chunk = rng.integers(0, 2**63, size=(min(elems, 1 << 20), 4), dtype=np.uint64)
    chunk[:, 3] >>= np.uint64(3)
    for b in range(0, elems, chunk.shape[0]):
        buf.upload(chunk[:min(chunk.shape[0], elems - b)], 32 * b)


def bench_perm(lib, cid, log_n, t, repeats, ceiling):
    n = 1 << log_n
    buf = DeviceBuffer(n * t * 32)
    fill(buf, n * t, log_n)

    def run():   # in place: a permutation of canonical elements is canonical elements
        N.check(lib.zk_poseidon_perm_dev(cid, t, n, buf.ptr, buf.ptr, None))
        N.check(lib.zk_dev_synchronize())

    row = {"log_n": log_n, "t": t, "perm": timed(run, repeats)}
    sec = row["perm"]["median_ms"] / 1e3
    row["permutations_per_s"] = round(n / sec)
    row["plain_field_products_per_s"] = round(n * plain_products(t) / sec)
    row["plain_products_per_permutation"] = plain_products(t)
    if ceiling:
        row["ubench_fp_mul_products_per_s"] = round(ceiling)
        row["share_of_ubench_rate"] = round(n * plain_products(t) / sec / ceiling, 3)
    buf.free()
    return row


def bench_tree(lib, cid, log_n, repeats):
    n = 1 << log_n
    nodes = _layout(n)[2]
    leaves = DeviceBuffer(n * 32)
    fill(leaves, n, 100 + log_n)
    ptree, btree = DeviceBuffer(nodes * 32), DeviceBuffer(nodes * 64)
    sync = lambda: N.check(lib.zk_dev_synchronize())  # noqa: E731

    def p_leaves():
        N.check(lib.zk_poseidon_sponge_rows_dev(cid, n, leaves.ptr, 1, ptree.ptr, None))
        sync()

    def p_build():
        N.check(lib.zk_poseidon_merkle_build_dev(cid, n, ptree.ptr, None))
        sync()

    def b_leaves():
        N.check(lib.zk_blake2b_rows_dev(n, leaves.ptr, 32, btree.ptr, None))
        sync()

    def b_build():
        N.check(lib.zk_merkle_build_dev(n, btree.ptr, None))
        sync()

    row = {"log_n": log_n, "poseidon_leaf_pass": timed(p_leaves, repeats), "poseidon_build": timed(p_build, repeats),
           "blake2b_leaf_pass": timed(b_leaves, repeats), "blake2b_build": timed(b_build, repeats)}
    row["poseidon_over_blake2b_build"] = round(row["poseidon_build"]["median_ms"] / row["blake2b_build"]["median_ms"], 2)
    row["poseidon_node_hashes_per_s"] = round((nodes - n) / (row["poseidon_build"]["median_ms"] / 1e3))
    for buf in (leaves, ptree, btree):
        buf.free()
    return row


def bench_host(curve, repeats):
    h = Poseidon(curve)
    h.hash([1, 2])   # the parameters are generated once
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for i in range(200):
            h.hash([i, i + 1])
        ms.append((time.perf_counter() - t0) * 1e3 / 200)
    return {"curve": curve, "host_hash_2_inputs": stats(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="*", default=[20, 24])
    ap.add_argument("--curves", nargs="*", default=["BN254"])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    repeats = max(args.repeats, 5)
    lib = N.ensure_gpu()   # no GPU, no numbers
    ceiling = ubench_ceiling()
    report = {"library": lib.zk_version().decode(), "perm": [], "tree": [], "host": []}

    def emit(key, row):
        print(json.dumps({key: row}), flush=True)
        report[key].append(row)

    for curve in args.curves:
        cid = N.curve_id(curve)
        for log_n in args.logs:
            emit("perm", dict(curve=curve, **bench_perm(lib, cid, log_n, 3, repeats, ceiling)))
        for log_n in args.logs:
            emit("tree", dict(curve=curve, **bench_tree(lib, cid, log_n, repeats)))
        emit("host", bench_host(curve, repeats))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
