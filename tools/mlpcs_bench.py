"""Multilinear KZG (zksnake_amd/commitment/polynomial/mkzg.py): wall-clock times of setup, commit, open and verify at 2^20 and 2^24
evaluations on both curves, with an opening split into the quotient kernel chain (zk_mlpcs_quotients_dev), each level's MSM and
the host's remainder, and two comparators from the same run: the univariate `KZG.open` over as many coefficients, and the fix
chain `zk_mle_fix_dev` with k = log_n over the same table.  The quotient chain moves the fix chain's traffic plus one write of the
table's size (every quotient once), so both are reported with their effective bytes/s.  Every timed call ends in work the host
waits for, is warmed up once, and is repeated; the report has the median and the spread (min, max).

    python tools/mlpcs_bench.py [--logs 20 24] [--curves BN254 BLS12_381] [--repeats 5] [--no-kzg] [--out FILE]

Also printed: how much of an opening goes to the MSMs of levels below 2^10 entries (a plan run has a floor of launches and a
host tail whatever its size, and an opening runs log n of them)."""

import argparse
import json
import os
import secrets
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from tools.pcs_bench import timed  # noqa: E402
from zksnake_amd import _native as N  # noqa: E402
from zksnake_amd.commitment.polynomial import KZG, MultilinearKZG  # noqa: E402
from zksnake_amd.frvec import DevVec, FrOps  # noqa: E402

SMALL_LEVEL = 1 << 10
T = N.MLE_TILE_LOG


def chain_bytes(log_n, quotients):
    """bytes the tiled chain over log_n variables moves: every pass reads its table and writes the 2^T times smaller one; with
    `quotients` every entry of every level is written once more (2^log_n - 1 elements)"""
    total, cur = 0, log_n
    while cur > 0:
        f = min(T, cur)
        total += 32 * ((1 << cur) + (1 << (cur - f)))
        cur -= f
    return total + (32 * ((1 << log_n) - 1) if quotients else 0)


def rate(nbytes, t):
    return round(nbytes / (t["median_ms"] * 1e-3) / 1e9, 1)   # GB/s


def bench(name, log_n, repeats, with_kzg):
    n = 1 << log_n
    s = MultilinearKZG(log_n, name)
    ops, r, lib = FrOps(s.order), s.order, N.load()
    t0 = time.perf_counter()
    s.setup()
    row = {"curve": name, "log_n": log_n, "setup_ms": round((time.perf_counter() - t0) * 1e3, 1)}
    table = ops.d_from(ops.random_vector(n))
    z = [secrets.randbelow(r) for _ in range(log_n)]
    state = {}

    def run_open():
        state["proof"], state["value"] = s.open(table, z)

    row["commit"] = timed(lambda: s.commit(table), repeats)
    row["open"] = timed(run_open, repeats)
    commitment = s.commit(table)
    row["verify"] = timed(lambda: s.verify(commitment, state["proof"], z, state["value"]) or sys.exit("verify failed"), repeats)

    # the opening's parts: the kernel chain alone, then every level's MSM over its slice of the one quotient buffer
    row["quotient_kernel"] = timed(lambda: s._quotients(table.ptr(), log_n, z), repeats)
    row["quotient_kernel"]["GB_per_s"] = rate(chain_bytes(log_n, True), row["quotient_kernel"])
    quotients, _ = s._quotients(table.ptr(), log_n, z)
    levels = []
    for k in range(log_n):
        entries, device_ms = 1 << (log_n - 1 - k), []
        level = s._levels[k + 1]
        t = timed(lambda: level.msm(quotients.ptr(n - (1 << (log_n - k))), entries, timings=device_ms), repeats)
        levels.append({"level": k, "entries": entries, "wall_ms": t["median_ms"], "device_ms": round(float(np.median(device_ms)), 3)})
    row["level_msms"] = levels
    msm_ms = sum(x["wall_ms"] for x in levels)
    small_ms = sum(x["wall_ms"] for x in levels if x["entries"] < SMALL_LEVEL)
    row["open_split_ms"] = {"kernel": row["quotient_kernel"]["median_ms"], "msms": round(msm_ms, 3),
                            "host": round(row["open"]["median_ms"] - row["quotient_kernel"]["median_ms"] - msm_ms, 3),
                            "msms_below_2^10_entries": round(small_ms, 3),
                            "share_of_open_below_2^10": round(small_ms / row["open"]["median_ms"], 3)}

    # comparator: the fix chain over the same table (what MultilinearPolynomial.evaluate runs, without the download)
    out = DevVec(1, zero=False)
    zl = ops.limbs(z)
    row["fix_chain"] = timed(lambda: (N.check(lib.zk_mle_fix_dev(ops.cid, log_n, table.ptr(), log_n, N.u64p(zl), out.ptr(), None)),
                                      N.check(lib.zk_dev_synchronize())), repeats)
    row["fix_chain"]["GB_per_s"] = rate(chain_bytes(log_n, False), row["fix_chain"])
    row["kernel_over_fix_chain"] = round(row["quotient_kernel"]["median_ms"] / row["fix_chain"]["median_ms"], 2)
    s.release()

    # comparator: a univariate KZG opening of as many coefficients
    if with_kzg:
        kzg = KZG(n - 1, name)
        kzg.setup(tau=secrets.randbelow(r))
        x = secrets.randbelow(r)
        row["kzg_open"] = timed(lambda: kzg.open(table, x), repeats)
        row["kzg_commit"] = timed(lambda: kzg.commit(table), repeats)
        kzg.G1_tau.release()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[20, 24])
    ap.add_argument("--curves", nargs="+", default=["BN254", "BLS12_381"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-kzg", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    lib = N.ensure_gpu()
    report = {"library": lib.zk_version().decode(), "results": []}
    for name in args.curves:
        for log_n in args.logs:
            row = bench(name, log_n, args.repeats, not args.no_kzg)
            report["results"].append(row)
            print(json.dumps(row), flush=True)
            split = row["open_split_ms"]
            print(f"# {name} 2^{log_n}: open {row['open']['median_ms']} ms = kernel {split['kernel']} + MSMs {split['msms']} + host {split['host']}; "
                  f"levels below 2^10 entries take {split['msms_below_2^10_entries']} ms ({100 * split['share_of_open_below_2^10']:.0f} % of the opening); "
                  f"kernel / fix chain = {row['kernel_over_fix_chain']}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
