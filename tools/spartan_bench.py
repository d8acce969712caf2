"""Spartan (zksnake_amd/spartan) on the benchmark chain circuit at 2^16, 2^20 and 2^22 constraints, both curves: wall-clock medians of
prove -- split into commit, the witness products, the outer rounds, row binding, the inner rounds, the opening and the rest (uploads,
the satisfaction check, transcript: "host") -- and of verify, the proof size, and `Groth16.prove` on the same circuit in the same run.

Two comparisons decide whether the fused kernels of csrc/spartan.hip earn their place; both use the same matrices in the same run and
alternate the two sides repeat by repeat:
    zk_r1cs_products_dev   against   three `DeviceCsr.apply` (A z, B z, C z)
    zk_r1cs_bind_dev       against   three transposed `DeviceCsr.apply` on E_x, a clear and one zk_vec_lincomb_dev
Each side is checked against the other by == on the downloaded tables before it is timed.  Every timed call ends in a device
synchronise, is warmed up once and repeated; the report has the median and the spread (min, max) with the run count.

    python tools/spartan_bench.py [--logs 16 20 22] [--curves BN254 BLS12_381] [--repeats 7] [--no-groth16] [--out FILE]
"""

import argparse
import json
import os
import secrets
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from tools.pcs_bench import timed  # noqa: E402
from zksnake_amd import _native as N  # noqa: E402
from zksnake_amd import workloads as W  # noqa: E402
from zksnake_amd.arithmetization import R1CS  # noqa: E402
from zksnake_amd.frvec import DevVec  # noqa: E402
from zksnake_amd.spartan import Spartan  # noqa: E402
from zksnake_amd.spmv import DeviceCsr  # noqa: E402
from zksnake_amd.subprotocol.gkr import eq_table  # noqa: E402


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "repeats": len(ms)}


def alternate(fused, composed, repeats):
    """the two sides timed turn by turn in one loop; both end in a device synchronise"""
    sync = N.load().zk_dev_synchronize
    out = {"fused": [], "composed": []}
    for fn in (fused, composed):
        fn()
        N.check(sync())
    for _ in range(repeats):
        for key, fn in (("fused", fused), ("composed", composed)):
            t0 = time.perf_counter()
            fn()
            N.check(sync())
            out[key].append((time.perf_counter() - t0) * 1e3)
    row = {k: stats(v) for k, v in out.items()}
    row["composed_over_fused"] = round(row["composed"]["median_ms"] / row["fused"]["median_ms"], 3)
    # faster beyond the spread of this run: the slowest fused repeat still beats the fastest composed one
    row["fused_faster_beyond_spread"] = row["fused"]["max_ms"] < row["composed"]["min_ms"]
    return row


def permuted_csrs(sp):
    """A, B, C with Spartan's column permutation as three DeviceCsr, row-major (rows = constraints, 2^s_x of them) and transposed
    (rows = permuted columns, 2^s of them): the composition the fused kernels are held against"""
    rows, cols = [], []
    for mat in (sp.r1cs.A, sp.r1cs.B, sp.r1cs.C):
        row_ptr, c, v = mat.to_csr()
        r = np.repeat(np.arange(sp.n_row, dtype=np.int64), np.diff(row_ptr.astype(np.int64)))
        c = sp.column(c.astype(np.int64))
        for seg, idx, n_seg, dst in ((r, c, 1 << sp.s_x, rows), (c, r, 1 << sp.s, cols)):
            order = np.argsort(seg, kind="stable")
            ptr = np.zeros(n_seg + 1, dtype=np.uint32)
            np.cumsum(np.bincount(seg, minlength=n_seg), out=ptr[1:])
            dst.append(DeviceCsr(sp._ops.cid, ptr, idx[order].astype(np.uint32), np.ascontiguousarray(v[order])))
    return rows, cols


def bench(curve, log_n, repeats, with_groth16):
    n = 1 << log_n
    r = W.scalar_field(curve)
    A, B, C, w, n_col = W.chain_circuit(n, r)
    r1cs = R1CS.from_triplets(A, B, C, n, n_col, 2, curve)
    public, private = w[:2], N.ints_to_limbs(w[2:], 4)
    t0 = time.perf_counter()
    sp = Spartan(r1cs)
    row = {"curve": curve, "constraints": n, "s_x": sp.s_x, "s": sp.s, "compile_ms": round((time.perf_counter() - t0) * 1e3, 1),
           "long_segments": {"rows": [sp._rows.n_long, sp._rows.n_items], "columns": [sp._cols.n_long, sp._cols.n_items]}}
    t0 = time.perf_counter()
    sp.setup()
    row["setup_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    ops = sp._ops

    state = {}
    row["prove"] = timed(lambda: state.update(proof=sp.prove(public, private)), repeats)
    phases = []
    for _ in range(repeats):
        t = {}
        sp.prove(public, private, timings=t)
        phases.append(t)
    row["prove_split_ms"] = {k: round(statistics.median(p[k] for p in phases), 3) for k in phases[0]}
    row["prove_split_repeats"] = repeats
    proof = state["proof"]
    row["verify"] = timed(lambda: sp.verify(proof, public) or sys.exit("verify failed"), repeats)
    row["proof_bytes"] = len(proof.to_bytes())

    # the fused kernels against their compositions, on the prover's own tables
    rows, cols = permuted_csrs(sp)
    z = DevVec(1 << sp.s)
    z.upload(private, 0)
    z.upload(ops.limbs(public), 1 << sp.h)
    n_x, n_y = 1 << sp.s_x, 1 << sp.s
    fused = [DevVec(n_x, zero=False) for _ in range(3)]
    composed = [DevVec(n_x, zero=False) for _ in range(3)]
    run_fused = lambda: sp._rows.products(sp.s, z.ptr(), *[v.ptr() for v in fused])  # noqa: E731
    run_composed = lambda: [m.apply(z.ptr(), v.ptr()) for m, v in zip(rows, composed)]  # noqa: E731
    run_fused(), run_composed()
    assert all(np.array_equal(a.download(), b.download()) for a, b in zip(fused, composed)), "products: fused != composed"
    row["products"] = alternate(run_fused, run_composed, repeats)

    ex = eq_table(ops, [secrets.randbelow(r) for _ in range(sp.s_x)])
    coeff = [secrets.randbelow(r) for _ in range(3)]
    coeff_limbs = ops.limbs(coeff)
    out_fused, out_composed = DevVec(n_y, zero=False), DevVec(n_y, zero=False)
    parts = [DevVec(n_y, zero=False) for _ in range(3)]
    run_fused = lambda: sp._cols.bind(sp.s_x, ex.ptr(), coeff_limbs, out_fused.ptr())  # noqa: E731

    def run_composed():
        for m, v in zip(cols, parts):
            m.apply(ex.ptr(), v.ptr())
        N.check(N.load().zk_dev_memset_async(out_composed.ptr(), 0, 32 * n_y, None))
        ops.d_lincomb(out_composed, [(n_y, c, v.ptr()) for c, v in zip(coeff, parts)])

    run_fused(), run_composed()
    assert np.array_equal(out_fused.download(), out_composed.download()), "bind: fused != composed"
    row["bind"] = alternate(run_fused, run_composed, repeats)
    sp.release()

    if with_groth16:
        from zksnake_amd.groth16 import Groth16
        g = Groth16(r1cs, curve)
        t0 = time.perf_counter()
        g.setup()
        row["groth16_setup_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["groth16_prove"] = timed(lambda: g.prove(public, private), repeats)
        row["groth16_proof_bytes"] = len(g.prove(public, private).to_bytes())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--curves", nargs="+", default=["BN254", "BLS12_381"])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-groth16", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    lib = N.ensure_gpu()
    report = {"library": lib.zk_version().decode(), "results": []}
    for curve in args.curves:
        for log_n in args.logs:
            row = bench(curve, log_n, args.repeats, not args.no_groth16)
            report["results"].append(row)
            print(json.dumps(row), flush=True)
            split = row["prove_split_ms"]
            print(f"# {curve} 2^{log_n}: prove {row['prove']['median_ms']} ms ({', '.join(f'{k} {v}' for k, v in split.items())}); verify "
                  f"{row['verify']['median_ms']} ms; proof {row['proof_bytes']} bytes; products composed/fused "
                  f"{row['products']['composed_over_fused']}, bind composed/fused {row['bind']['composed_over_fused']}"
                  + (f"; Groth16.prove {row['groth16_prove']['median_ms']} ms" if "groth16_prove" in row else ""), flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
