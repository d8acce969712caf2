"""Merkle trees (zksnake_amd/commitment/vector): wall-clock times of the leaf pass, the build and open_many(2^10 indices) over
2^16, 2^20 and 2^24 leaves of 32 bytes resident in a DevVec, of a commit from a host list of 2^20 bytes items with the host's share
(join and offsets, upload) apart, and -- the baseline, since the parent commit has no Merkle tree -- of the reference's path on the
same machine: a hashlib commit and one hashlib open at 2^16 and 2^20.  Every timed call is warmed up once, ends in a device
synchronisation or a download, and is repeated; the report has the median and the spread (min, max).

    python tools/merkle_bench.py [--logs 16 20 24] [--host-log 20] [--baseline-logs 16 20] [--repeats 7] [--out FILE]
                                 [--variant-lib OTHER_LIBZKMI --variant-logs 12 16 20 --variant-path-logs 16 20]

The build is also timed from every level upwards (the tree above level l is itself a tree over that level's nodes, in place), which
lists what each launch costs; "launches" names them by the rule of csrc/merkle.hip, one launch per level.

--variant-lib: another build of the library (an experiment on csrc/merkle.hip) whose zk_merkle_build_dev is timed against this
one's on the same device memory, alternated run by run, at least six runs each.  This is how the one-workgroup tail kernel was
decided (EXPERIMENTS.md "Merkle trees"): the variant finished every level of at most 1024 nodes in one workgroup.  The two path
gathers, zk_merkle_paths_dev and zk_poseidon_merkle_paths_dev at 2^10 indices, are alternated in the same way; they only copy, so
the tree they read is random bytes and the two libraries' outputs are compared with ==."""

import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zksnake_amd import _native as N  # noqa: E402
from zksnake_amd.commitment.vector import Merkle  # noqa: E402
from zksnake_amd.commitment.vector._tree import _layout  # noqa: E402
from zksnake_amd.commitment.vector.merkle import _host_leaves  # noqa: E402
from zksnake_amd.device import DeviceBuffer  # noqa: E402
from zksnake_amd.frvec import DevVec  # noqa: E402

D = 64


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def timed(fn, repeats, warm=1):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def launches(n):
    out, width = [], n
    while width > 1:
        out.append(f"level({width}->{(width + 1) // 2}: {min((((width + 1) // 2) + 255) // 256, 1024)} workgroups)")
        width = (width + 1) // 2
    return out


def random_vec(n, seed):
    vec = DevVec(n, zero=False)
    rng = np.random.default_rng(seed)
    step = 1 << 22
    for b in range(0, n, step):
        limbs = rng.integers(0, 2**63, size=(min(step, n - b), 4), dtype=np.uint64)
        limbs[:, 3] >>= np.uint64(3)   # below 2^252: canonical in both fields (the hash does not care)
        vec.upload(limbs, b)
    return vec


def bench_resident(lib, log_n, repeats):
    n = 1 << log_n
    vec = random_vec(n, log_n)
    depth, offsets, nodes = _layout(n)
    tree = DeviceBuffer(nodes * D)
    sync = lambda: N.check(lib.zk_dev_synchronize())  # noqa: E731

    def leaves():
        N.check(lib.zk_blake2b_rows_dev(n, vec.ptr(), 32, tree.ptr, None))
        sync()

    def build_from(level):
        def run():
            N.check(lib.zk_merkle_build_dev(n_of[level], tree.ptr + offsets[level] * D, None))
            sync()
        return run

    n_of = [(offsets[l + 1] if l < depth else nodes) - offsets[l] for l in range(depth + 1)]
    row = {"log_n": log_n, "leaf_pass": timed(leaves, repeats), "build": timed(build_from(0), repeats), "launches": launches(n)}
    row["build_from_level_ms"] = [timed(build_from(l), max(repeats // 2, 3))["median_ms"] for l in range(depth) if n_of[l] > 1]
    scheme = Merkle()
    row["tree_end_to_end"] = timed(lambda: scheme.tree(vec).release(), repeats)
    t = scheme.tree(vec)
    rng = np.random.default_rng(1)
    indices = [int(x) for x in rng.integers(0, n, size=1 << 10)]
    row["open_many_1024"] = timed(lambda: t.open_many(indices), repeats)
    row["open_one"] = timed(lambda: t.open(indices[0]), repeats)
    proof = t.open(5)
    assert scheme.verify(t.root, proof, 5, vec.download(1, 5).tobytes()), "an opening does not verify"
    t.release()
    tree.free()
    return row


def bench_host_list(log_n, repeats):
    n = 1 << log_n
    raw = np.random.default_rng(2).integers(0, 256, size=n * 32, dtype=np.uint8).tobytes()
    items = [raw[32 * i:32 * i + 32] for i in range(n)]
    mixed = [x[:1 + i % 32] for i, x in enumerate(items)]   # lengths 1..32: the items kernel with offsets
    scheme = Merkle()
    row = {"log_n": log_n}
    for name, vector in (("equal_lengths", items), ("mixed_lengths", mixed)):
        data = _host_leaves(vector)[1]
        row[name] = {"commit": timed(lambda: scheme.commit(vector), repeats),
                     "host_join_and_offsets": timed(lambda: _host_leaves(vector), repeats),
                     "upload": timed(lambda: DeviceBuffer.from_numpy(data).free(), repeats)}
    return row, items


# ---- the reference's path: hashlib, one call per leaf and per node, the whole tree again for an open ---------------------------
def hashlib_tree(vector):
    level = [hashlib.blake2b(x).digest() for x in vector]
    tree = [level]
    while len(level) > 1:
        level = [hashlib.blake2b(level[i] + (level[i + 1] if i + 1 < len(level) else level[i])).digest() for i in range(0, len(level), 2)]
        tree.append(level)
    return tree


def hashlib_open(vector, index):
    proof = []
    for level in hashlib_tree(vector)[:-1]:
        if index ^ 1 < len(level):
            proof.append(level[index ^ 1])
        index //= 2
    return proof


def bench_baseline(log_n, repeats, items=None):
    n = 1 << log_n
    if items is None or len(items) != n:
        raw = np.random.default_rng(3).integers(0, 256, size=n * 32, dtype=np.uint8).tobytes()
        items = [raw[32 * i:32 * i + 32] for i in range(n)]
    scheme = Merkle()
    assert hashlib_tree(items)[-1][0] == scheme.commit(items), "the device root differs from hashlib's"
    return {"log_n": log_n, "hashlib_commit": timed(lambda: hashlib_tree(items)[-1][0], repeats, warm=0),
            "hashlib_open": timed(lambda: hashlib_open(items, 7), repeats, warm=0),
            "device_commit_from_host_list": timed(lambda: scheme.commit(items), repeats),
            "device_open_from_host_list": timed(lambda: scheme.open(items, 7), repeats)}


def variant_lib(path):
    other = ctypes.CDLL(path)
    for name in ("zk_init", "zk_merkle_build_dev", "zk_merkle_paths_dev", "zk_poseidon_merkle_paths_dev"):
        getattr(other, name).restype, getattr(other, name).argtypes = N.SIGNATURES[name]
    if other.zk_init(0) != N.ZK_OK:
        sys.exit("the variant library does not initialise")
    return other


def alternate(lib, other, call, result, repeats):
    """call(l) on this library and on the variant, run by run, each run ended by a device synchronisation; two warm-up rounds.
    result() is what the last call left behind, and must be the same for both"""
    ms, left = {"this": [], "variant": []}, {}
    for rep in range(repeats + 2):
        for name, l in (("this", lib), ("variant", other)):
            t0 = time.perf_counter()
            if call(l) != N.ZK_OK:
                sys.exit(f"{name}: the call failed")
            N.check(lib.zk_dev_synchronize())
            if rep >= 2:
                ms[name].append((time.perf_counter() - t0) * 1e3)
            left[name] = result()
    assert left["this"] == left["variant"], "the two libraries give different results"
    a, b = stats(ms["this"]), stats(ms["variant"])
    return {"this": a, "variant": b, "gain_of_this_ms": round(b["median_ms"] - a["median_ms"], 4),
            "spread_of_variant_ms": round(b["max_ms"] - b["min_ms"], 4), "this_inside_variant_spread_or_below": a["median_ms"] <= b["max_ms"]}


def bench_variant(lib, other, logs, repeats):
    """zk_merkle_build_dev of this library and of the variant, alternated, on one tree"""
    rows = []
    for log_n in logs:
        n = 1 << log_n
        nodes = _layout(n)[2]
        tree = DeviceBuffer(nodes * D)
        tree.upload(np.random.default_rng(log_n).integers(0, 256, size=n * D, dtype=np.uint8))
        rows.append({"log_n": log_n, **alternate(lib, other, lambda l: l.zk_merkle_build_dev(n, tree.ptr, None),
                                                 lambda: tree.download((D,), np.uint8, (nodes - 1) * D).tobytes(), repeats)})
        tree.free()
    return rows


def bench_variant_paths(lib, other, logs, repeats, k=1 << 10):
    """the two gathers of this library and of the variant, alternated, k indices into one tree of each node size"""
    rows = []
    for log_n in logs:
        n = 1 << log_n
        depth, _, nodes = _layout(n)
        d_idx = DeviceBuffer.from_numpy(np.random.default_rng(log_n).integers(0, n, size=k, dtype=np.uint64))
        for entry, node in (("zk_merkle_paths_dev", 64), ("zk_poseidon_merkle_paths_dev", 32)):
            tree = DeviceBuffer.from_numpy(np.random.default_rng(node + log_n).integers(0, 256, size=nodes * node, dtype=np.uint8))
            paths = DeviceBuffer(k * depth * node)
            rows.append({"entry": entry, "log_n": log_n, "indices": k,
                         **alternate(lib, other, lambda l: getattr(l, entry)(n, tree.ptr, k, d_idx.ptr, paths.ptr, None),
                                     lambda: paths.download((k * depth * node,), np.uint8).tobytes(), repeats)})
            tree.free()
            paths.free()
        d_idx.free()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="*", default=[16, 20, 24])
    ap.add_argument("--host-log", type=int, default=20)
    ap.add_argument("--baseline-logs", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--variant-lib")
    ap.add_argument("--variant-logs", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--variant-path-logs", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--out")
    args = ap.parse_args()
    lib = N.ensure_gpu()
    report = {"library": lib.zk_version().decode(), "resident": [], "baseline": []}

    def emit(key, row):
        print(json.dumps({key: row}), flush=True)
        return row

    if args.variant_lib:
        other = variant_lib(args.variant_lib)
        report["build_this_against_variant"] = emit("build_this_against_variant", bench_variant(lib, other, args.variant_logs, max(args.repeats, 6)))
        report["paths_this_against_variant"] = emit("paths_this_against_variant", bench_variant_paths(lib, other, args.variant_path_logs, max(args.repeats, 6)))
    for log_n in args.logs:
        report["resident"].append(emit("resident", bench_resident(lib, log_n, args.repeats)))
    items = None
    if args.host_log:
        report["host_list"], items = bench_host_list(args.host_log, args.repeats)
        emit("host_list", report["host_list"])
    for log_n in args.baseline_logs:
        report["baseline"].append(emit("baseline", bench_baseline(log_n, max(args.repeats // 2, 3), items)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
