#!/usr/bin/env python3
"""
bench.py -- headline benchmark of the MI355X proving backend.

One "step" = one BN254 G1 Pippenger MSM over 2^20 (scalar, point) pairs (BASELINE.json configs[1]),
scalars and the Montgomery-form bases already resident in HBM when the timed region starts; the
result (one affine point) lands in host memory, as the reference's `multiscalar_mul_g1` returns it.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

N > 1 (launched through torch.distributed.run, one rank per GPU): the MSM is sharded by window
across ranks (north star), each rank reduces its windows to one partial point, the partials are
exchanged with an RCCL all_gather over xGMI and summed on the host: strong scaling of one MSM.

Rank 0 prints ONE JSON line (metric, value, ms_per_step, roofline, ...).  A plain run does only what the headline needs:
set-up, W warm-up steps, K timed steps, the closed-form check of the result.  --dump-outputs DIR writes the result of the
last timed step to DIR/msm_result.npy.  --full adds `cpu_baseline` and `extra`: the second half of BASELINE.json's metric
-- Groth16.prove at 2^20 BN254 constraints (median, own roofline and cpu_baseline, proof bytes compared with the
committed closed-form proof) -- and the other configs (NTT 2^22, the other three groups' MSMs).
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from zksnake_amd import _native as N  # noqa: E402
from zksnake_amd import workloads as W  # noqa: E402
from zksnake_amd import constant  # noqa: E402
from zksnake_amd.parallel import all_gather_sum, window_ranges  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec
# chip-wide v_mad_u64_u32 issue rate, measured (tools/ubench2.hip, profiles/r03_ubench2_valu.log): 4.74 cycles per
# wave-instruction per SIMD at eight waves per SIMD = 33.2 T/s at 2.4 GHz.  Rounds 1-2 quoted 26.4 T/s from a loop that
# carried an extra add per multiply-add; the fractions reported against it were too flattering by a quarter.
MAD_PEAK_T = 33.2
BYTES_PER_PAIR = 96     # 32 B scalar + 64 B affine base (BN254 G1)


# v_mad_u64_u32 per XYZZ mixed addition over a 9-limb field, as the compiled kernel has them (1467 in the ISA of the hot
# path): 6 products (81 + 81), 2 squarings (45 + 81) and the Y3 double product with one reduction (162 + 81); the 9
# reduction quotients of every product are v_mul_lo_u32 and are not counted
MADS_PER_MIXED_ADD = 6 * 162 + 2 * 126 + 243


def launch_ranks(n_ranks, argv):
    """start `n_ranks` ranks of this script under torch.distributed.run (one process per GPU, rendezvous on 127.0.0.1 at a
    free port) and return their exit code.  Runs in a process that has not touched the GPU and does not import torch."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: what RCCL needs on this driver
    env.setdefault("OMP_NUM_THREADS", "1")              # torchrun's own default, set here so that it does not warn
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--window-bits", type=int, default=0)
    ap.add_argument("--full", action="store_true", help="beside the headline, also measure the CPU baselines and the secondary "
                    "numbers reported under 'extra' (each can be left out with --no-cpu-baseline / --no-extra)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the MSM result of the last timed step to DIR/msm_result.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the secondary numbers reported under 'extra': "
                    "fixed-base MSM, NTT 2^22, Groth16 prove 2^20")
    ap.add_argument("--prove-log-n", type=int, default=20)
    ap.add_argument("--precompute", action="store_true", help="plan flag ZK_MSM_PRECOMPUTE (fixed-base table 2^(cw) P_i, shared buckets)")
    ap.add_argument("--plonk-log-n", type=int, default=18, help="gates (log2) of the PlonK prove in `extra`")
    ap.add_argument("--large-log-n", type=int, default=24, help="size (log2) of the large MSM reported in `extra` at every N")
    ap.add_argument("--config5-log-n", type=int, default=23, help="constraints (log2) of the BLS12-381 prove of BASELINE configs[4] in "
                    "`extra`, at every N; 0 skips it")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL; gloo only to rehearse "
                    "the multi-rank path on a box with fewer GPUs than ranks)")
    ap.add_argument("--rendezvous-only", action="store_true", help="launcher check (runs without a GPU, gloo): the ranks form their "
                    "group, count themselves with one all_reduce and rank 0 prints n_gpus / ranks_in_group; nothing is measured")
    args = ap.parse_args()

    if args.gpus < 1:
        raise SystemExit("--gpus must be at least 1")
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")
    cpu_baseline = args.full and not args.no_cpu_baseline
    extra = args.full and not args.no_extra
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # started plainly (`python bench.py --gpus N`, the shape of the driver's N = 1 command): this process becomes the
        # launcher.  It has made no GPU call (torch is not even imported yet) and never will; the N ranks are fresh children
        # of torch.distributed.run, which hands each its RANK / LOCAL_RANK / WORLD_SIZE.  The exit code is theirs.
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        # never report a run under a rank count it did not have (round-3 verdict: `--gpus 8` used to print "n_gpus": 1)
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with `python bench.py --gpus {args.gpus}` (starts its own "
                         f"ranks) or `python -m torch.distributed.run --nproc-per-node {args.gpus} bench.py --gpus {args.gpus}`")

    import torch
    import torch.distributed as dist

    if args.rendezvous_only:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        counted = 1
        if world > 1:
            dist.init_process_group("gloo")
            t = torch.ones(1, dtype=torch.int64)
            dist.all_reduce(t)
            counted = int(t.item())
        if rank == 0:
            print(json.dumps({"rendezvous_only": True, "n_gpus": world, "ranks_in_group": dist.get_world_size() if world > 1 else 1,
                              "ranks_counted": counted}), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return

    n_dev = torch.cuda.device_count()
    dev_index = local_rank if args.backend == "nccl" else local_rank % max(1, n_dev)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.backend)
    lib = N.ensure_gpu(dev_index)
    gather_dev = dev if args.backend == "nccl" else None

    cid, grp = N.CURVE_BN254, N.G1
    r = constant.BN254_SCALAR_FIELD
    n = 1 << args.log_n
    PW = N.point_limbs(cid, grp)

    # ---- synthetic workload: SplitMix64 scalars, bases k_i * G with known k_i
    sc_limbs, sc_ints = W.field_stream(W.SEED_MSM_SCALARS, n, r)
    k_limbs, k_ints = W.field_stream(W.SEED_MSM_BASES, n, r)
    gen = np.zeros(PW, dtype=np.uint64)
    N.check(lib.zk_point_generator(cid, grp, N.u64p(gen)))
    bases = np.zeros((n, PW), dtype=np.uint64)
    N.check(lib.zk_batch_mul(cid, grp, n, N.u64p(k_limbs), N.u64p(gen), 1, N.u64p(bases)))
    # closed-form expectation: (sum s_i k_i mod r) * G
    dot = sum(a * b for a, b in zip(sc_ints, k_ints)) % r
    expected = np.zeros(PW, dtype=np.uint64)
    N.check(lib.zk_point_mul(cid, grp, N.u64p(gen), N.u64p(N.ints_to_limbs([dot])), N.u64p(expected)))

    handle = N._u64(0)
    N.check(lib.zk_msm_plan_create(cid, grp, n, bases.ctypes.data, 0, N.MSM_PRECOMPUTE if args.precompute else 0, args.window_bits, handle))
    c_bits, nwin = N._i(0), N._i(0)
    N.check(lib.zk_msm_plan_windows(handle, c_bits, nwin))
    entries = N._u64(0)
    N.check(lib.zk_msm_plan_entries(handle, entries))   # per window: 2n when the plan runs on endomorphism pairs
    ranges = window_ranges(nwin.value, world)
    w_first, w_count = ranges[rank]

    d_scalars = torch.from_numpy(sc_limbs.view(np.int64)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    out = np.zeros(PW, dtype=np.uint64)
    tm = (N.ctypes.c_float * 5)()

    def step():
        if w_count > 0:
            N.check(lib.zk_msm_plan_run(handle, n, d_scalars.data_ptr(), 1, w_first, w_count, N.u64p(out), stream))
        else:
            out[:] = 0
        if world == 1:
            return out.copy()
        return all_gather_sum(cid, grp, out, gather_dev)

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(max(1, args.warmup)):
        res = step()
    if not (res == expected).all():
        raise SystemExit("MSM result does not match the closed-form expectation (sum s_i k_i) * G")

    acc_ms = []
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = step()
        lib.zk_msm_plan_timings(handle, tm, 5)
        acc_ms.append(list(tm))
    sync()
    elapsed = time.perf_counter() - t0
    if not (res == expected).all():
        raise SystemExit("MSM result changed during the timed loop")
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, res)

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = n / (elapsed / args.steps) / 1e6  # Mscalar/s, whole job
        stage = np.array(acc_ms).mean(axis=0)
        # dominant kernel = bucket accumulation; algorithmic bytes it covers in one launch:
        # every (scalar, base) pair once = 96 B x n (at N>1 each rank's launch covers its windows of all pairs)
        acc_s = float(stage[1]) * 1e-3
        achieved = BYTES_PER_PAIR * n / acc_s / 1e9 if acc_s > 0 else 0.0
        # HBM bytes of one launch from the PMC passes (FETCH_SIZE / WRITE_SIZE, tools/collect_profiles.sh); only reported
        # while the kernel sources are the ones it was measured on (tools/fingerprint.py)
        from tools.fingerprint import load_profiled, load_traffic
        traffic, traffic_src = load_traffic("msm_traffic.json", "msm")
        kernel_ms_profiled = load_profiled("msm_traffic.json", "msm", "kernel_avg_ms_profiled")
        if args.log_n != 20 or args.precompute or args.window_bits or world > 1:
            traffic, traffic_src, kernel_ms_profiled = None, "the committed figure is for the default 2^20 single-GPU run", None
        # two fractions, because they answer different questions (round-3 advisor finding: one object carried both kinds of
        # number): `frac` prices the ALGORITHMIC 96 B per pair (what the contract asks for), `frac_measured` the bytes the
        # counters saw -- signed-digit Pippenger reads a base once per WINDOW, and a 64-byte row costs a 128-byte line
        measured = traffic / acc_s / 1e9 if traffic and acc_s > 0 else None
        line = {
            "metric": "BN254 G1 MSM throughput",
            "value": round(value, 3),
            "unit": "Mscalar/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "u32 limbs (254-bit modular integers)",
            "data": "synthetic",
            "config": {
                "workload": f"BN254 G1 Pippenger MSM, 2^{args.log_n} SplitMix64 (scalar, point) pairs, bit-exact vs (sum s_i k_i) G",
                "curve": "BN254",
                "log_n": args.log_n,
                "window_bits": c_bits.value,
                "windows": nwin.value,
                "entries_per_window": entries.value,
                "endomorphism_split": bool(entries.value == 2 * n),
                "precompute": bool(args.precompute),
                "parallelism": f"window-sharded x{world}" if world > 1 else "single GPU",
                "collective_backend": (dist.get_backend() if world > 1 else None),
                "ranks_in_group": (dist.get_world_size() if world > 1 else 1),
            },
            "roofline": {
                "kernel": "accumulate_kernel<Bn254G1>",
                "bound": "hbm",
                "achieved": round(achieved, 3),
                "peak": HBM_PEAK_GBPS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBPS, 6),
                "traffic": traffic,
                "traffic_source": traffic_src,
                "kernel_ms": round(float(stage[1]), 4),
                "kernel_ms_profiled": kernel_ms_profiled,
                "achieved_measured": round(measured, 1) if measured else None,
                "frac_measured": round(measured / HBM_PEAK_GBPS, 4) if measured else None,
                "note": "achieved / frac: algorithmic bytes (96 B per pair) over the kernel's time, HIP events around its launches in this "
                        "run (kernel_ms); kernel_ms_profiled: the same kernel's average in the rocprofv3 kernel trace of the same command "
                        "(profiles/, same sources).  achieved_measured / frac_measured: the counters' bytes (`traffic`) over kernel_ms -- "
                        "about half of the HBM peak: every base row is read once per window and costs a 128-byte line.  What binds is "
                        "integer VALU issue (roofline_valu: the SIMDs are saturated, profiles/*_bench_pmc_sq.json); see DESIGN.md 4.1",
            },
            # the resource that actually binds: 32-bit integer multiply-add issue.  Per mixed addition the kernel
            # executes 8 products (2 N^2 = 162 v_mad_u64_u32 at N = 9 limbs, plus N v_mul_lo_u32) and 2 squarings (126); the
            # peak is the measured chip-wide v_mad_u64_u32 rate (MAD_PEAK_T above).
            "roofline_valu": {
                "kernel": "accumulate_kernel<Bn254G1>",
                "bound": "int32 multiply-add issue (v_mad_u64_u32)",
                "achieved": round(nwin.value * entries.value * MADS_PER_MIXED_ADD / acc_s / 1e12, 3) if acc_s > 0 and world == 1 else None,
                "peak": MAD_PEAK_T,
                "unit": "Tmad/s",
                "frac": round(nwin.value * entries.value * MADS_PER_MIXED_ADD / acc_s / 1e12 / MAD_PEAK_T, 4) if acc_s > 0 and world == 1 else None,
                "mixed_additions_per_launch": nwin.value * entries.value,
            },
            "stage_ms": {
                "digits_sort": round(float(stage[0]), 4),
                "accumulate": round(float(stage[1]), 4),
                "reduce": round(float(stage[2]), 4),
                "host_tail": round(float(stage[3]), 4),
                "total_gpu_plus_tail": round(float(stage[4]), 4),
            },
        }
        if cpu_baseline and world == 1:
            from oracle import corc  # checker / CPU baseline only
            t1 = time.perf_counter()
            cpu_res = corc.msm(cid, grp, sc_limbs, bases, threads=1)
            cpu_s = time.perf_counter() - t1
            if not (cpu_res == expected).all():
                raise SystemExit("CPU oracle disagrees with the closed-form expectation")
            line["cpu_baseline"] = {
                "value": round(n / cpu_s / 1e6, 4),
                "unit": "Mscalar/s",
                "cores": 1,
                "kind": "port",
                "sample": f"the same 2^{args.log_n}-pair MSM, ark-ec 0.4.2 signed-digit Pippenger restated in C++ (oracle/zk_oracle.cpp), "
                          f"window c={corc.ark_window(n)}, 1 thread (the default zksnake wheel runs ark's MSM single-threaded)",
                "seconds": round(cpu_s, 3),
            }
            # the restatement parallelises over windows (as ark's rayon feature does): more threads than windows stay idle
            cores = min(os.cpu_count() or 1, 254 // corc.ark_window(n) + 1)
            t1 = time.perf_counter()
            cpu_res = corc.msm(cid, grp, sc_limbs, bases, threads=cores)
            cpu_all = time.perf_counter() - t1
            if not (cpu_res == expected).all():
                raise SystemExit("CPU oracle (all cores) disagrees with the closed-form expectation")
            line["cpu_baseline_all_cores"] = {
                "value": round(n / cpu_all / 1e6, 4), "unit": "Mscalar/s", "cores": cores, "kind": "port",
                "sample": "the same MSM, one OpenMP thread per window of the restatement (rayon-style window parallelism; not what the "
                          f"default wheel does); the host has {os.cpu_count()} logical cores", "seconds": round(cpu_all, 3),
            }
        if extra and world == 1:
            # The same MSM in steady state.  After idle the GPU needs ~20 back-to-back MSMs (~30 ms of load) to reach the clock it
            # then holds (tools/ramp_probe.py, profiles/r04_ramp_probe.log: 1.70-1.79 ms for steps 2-5, 1.46-1.54 from step 21 on),
            # so the headline above -- `--warmup 5`, then 20 timed steps -- is measured on the ramp.  Reported beside it, never as
            # `value`: 100 more untimed MSMs, then 100 timed ones.
            for _ in range(100):
                step()
            sync()
            t1 = time.perf_counter()
            for _ in range(100):
                res = step()
            sync()
            sus = (time.perf_counter() - t1) / 100
            if not (res == expected).all():
                raise SystemExit("MSM result changed during the sustained loop")
            lib.zk_msm_plan_timings(handle, tm, 5)
            sustained = {"ms": round(sus * 1e3, 4), "Mscalar/s": round(n / sus / 1e6, 2), "accumulate_kernel_ms": round(tm[1], 4),
                         "after_untimed_steps": args.warmup + args.steps + 100, "timed_steps": 100,
                         "note": "the headline's MSM once the GPU holds its clock under load (the timed region of `value` starts "
                                 f"{args.warmup} MSMs after idle, on the clock ramp); reported beside `value`, not instead of it"}
            line["extra"] = extra_metrics(lib, torch, dev, args, bases, d_scalars, expected)
            line["extra"]["msm_sustained_after_clock_ramp"] = sustained
            line["extra"].update(large_msm_metric(lib, torch, args, dev, None, 0, 1))
    if extra and world > 1:
        # the whole prove split over the ranks by task x window (BASELINE metric, second half); collective on all ranks.  The
        # window-only layout of rounds 1-3 runs beside it for comparison.
        sharded = prove_metric(torch, args, dev if args.backend == "nccl" else None, world)
        sharded.update(prove_metric(torch, args, dev if args.backend == "nccl" else None, world, partition="window"))
        if args.config5_log_n:
            # BASELINE configs[4]: BLS12-381 at 2^23 constraints, G1 / G2 MSMs split over the ranks (G2 by window)
            sharded.update(prove_metric(torch, args, dev if args.backend == "nccl" else None, world, curve="BLS12_381", log_n=args.config5_log_n))
        sharded.update(large_msm_metric(lib, torch, args, dev, gather_dev, rank, world))
        if rank == 0:
            line["extra"] = sharded
    if rank == 0:
        print(json.dumps(line), flush=True)

    N.check(lib.zk_msm_plan_destroy(handle))
    if world > 1:
        dist.destroy_process_group()


def dump_outputs(path, point):
    """the MSM result a caller receives (one affine point as 64-bit limbs, x then y) as DIR/msm_result.npy: float64 of shape
    (2, 32), one row per coordinate, its little-endian bytes -- exact in float64, and a change of any bit changes a value by >= 1"""
    os.makedirs(path, exist_ok=True)
    coords = np.ascontiguousarray(point, dtype="<u8").view(np.uint8).reshape(2, -1)
    np.save(os.path.join(path, "msm_result.npy"), coords.astype(np.float64))


def extra_metrics(lib, torch, dev, args, bases, d_scalars, expected):
    """secondary numbers (not the headline), all checked for correctness before they are reported"""
    out = {}
    stream = torch.cuda.current_stream().cuda_stream
    cid, grp = N.CURVE_BN254, N.G1
    n = bases.shape[0]

    # (1) the same MSM with the fixed-base table (ZK_MSM_PRECOMPUTE): what Groth16.prove uses for proving keys
    h = N._u64(0)
    N.check(lib.zk_msm_plan_create(cid, grp, n, bases.ctypes.data, 0, N.MSM_PRECOMPUTE, args.window_bits, h))
    res = np.zeros(bases.shape[1], dtype=np.uint64)
    for _ in range(2):
        N.check(lib.zk_msm_plan_run(h, n, d_scalars.data_ptr(), 1, 0, 0, N.u64p(res), stream))
    assert (res == expected).all(), "fixed-base MSM differs from the closed form"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 10
    for _ in range(reps):
        N.check(lib.zk_msm_plan_run(h, n, d_scalars.data_ptr(), 1, 0, 0, N.u64p(res), stream))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / reps * 1e3
    tm = (N.ctypes.c_float * 5)()
    lib.zk_msm_plan_timings(h, tm, 5)
    out["msm_fixed_base_table"] = {"ms": round(ms, 4), "Mscalar/s": round(n / ms / 1e3, 2), "accumulate_kernel_ms": round(tm[1], 4),
                                   "note": "bases expanded once to 2^(c w) P_i rows (1 GiB at 2^20), one shared bucket set"}
    N.check(lib.zk_msm_plan_destroy(h))

    # (1b) throughput with two general-mode plans in flight (enqueue k+1 before finishing k): the latency-bound
    # bucket reduction and the host tail of one MSM overlap the accumulation of the next, as they do for the five
    # MSMs inside Groth16.prove.  Reported separately: the headline times strictly sequential MSMs.
    hs = [N._u64(0), N._u64(0)]
    for hh in hs:
        N.check(lib.zk_msm_plan_create(cid, grp, n, bases.ctypes.data, 0, 0, args.window_bits, hh))
    outs = [np.zeros(bases.shape[1], dtype=np.uint64) for _ in range(2)]
    N.check(lib.zk_msm_plan_enqueue(hs[0], n, d_scalars.data_ptr(), 1, 0, 0, N.STREAM_PLAN))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps2 = 20
    for k in range(reps2):
        N.check(lib.zk_msm_plan_enqueue(hs[(k + 1) & 1], n, d_scalars.data_ptr(), 1, 0, 0, N.STREAM_PLAN))
        N.check(lib.zk_msm_plan_finish(hs[k & 1], N.u64p(outs[k & 1])))
    ms = (time.perf_counter() - t0) / reps2 * 1e3
    N.check(lib.zk_msm_plan_finish(hs[reps2 & 1], N.u64p(outs[reps2 & 1])))
    assert (outs[0] == expected).all() and (outs[1] == expected).all(), "pipelined MSM differs from the closed form"
    out["msm_two_plans_in_flight"] = {"ms_per_msm": round(ms, 4), "Mscalar/s": round(n / ms / 1e3, 2)}
    for hh in hs:
        N.check(lib.zk_msm_plan_destroy(hh))

    # (1a') the reference's call shape, multiscalar_mul_g1(points, scalars) with fresh host buffers per call
    # (src/bn254/curve.rs:356-373): plan creation, upload of bases and scalars over PCIe, run, teardown -- all inside the call
    sc_host = d_scalars.cpu().numpy().view(np.uint64).copy()
    one = np.zeros(bases.shape[1], dtype=np.uint64)
    shots = []
    for _ in range(4):
        t0 = time.perf_counter()
        N.check(lib.zk_msm(cid, grp, n, n, N.u64p(sc_host), N.u64p(bases), N.u64p(one)))
        shots.append((time.perf_counter() - t0) * 1e3)
    assert (one == expected).all(), "one-shot zk_msm differs from the closed form"
    ms = float(np.median(shots[1:]))
    out["msm_one_shot_host_buffers"] = {"ms": round(ms, 4), "Mscalar/s": round(n / ms / 1e3, 2), "first_call_ms": round(shots[0], 3),
                                        "note": "zk_msm(host scalars, host points): plan creation + 96 MiB over PCIe + run + teardown per call, "
                                                "the reference's multiscalar_mul_g1 call shape; never the headline value"}

    # (1c) the other three groups at 2^20 pairs (BN254 G2 is a third of a proof; BLS12-381 is BASELINE config 5's curve)
    out.update(group_msm_metrics(lib, torch))

    # (2) BN254 Fr NTT at 2^22, resident in HBM (BASELINE config 3)
    log_n = 22
    m = 1 << log_n
    limbs = W.splitmix64(W.SEED_NTT, 4 * m).reshape(m, 4)
    limbs[:, 3] &= np.uint64((1 << 60) - 1)
    d = torch.from_numpy(limbs.view(np.int64)).to(dev)
    N.check(lib.zk_ntt_dev(0, 0, log_n, d.data_ptr(), stream))
    N.check(lib.zk_ntt_dev(0, 1, log_n, d.data_ptr(), stream))
    assert (d.cpu().numpy().view(np.uint64) == limbs).all(), "iNTT(NTT(x)) != x"
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        N.check(lib.zk_ntt_dev(0, 0, log_n, d.data_ptr(), stream))
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    out["ntt_bn254_fr_2^22"] = {"ms": round(ms, 4), "Melem/s": round(m / ms / 1e3, 2),
                                "roofline": {"kernel": "ntt_pass_kernel<BnFrParams> (3 launches per transform)", "bound": "hbm",
                                             "achieved": round(64 * m / ms / 1e6, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                             "frac": round(64 * m / ms / 1e6 / HBM_PEAK_GBPS, 5),
                                             "note": "64 B/element algorithmic (SURVEY 8d); the passes are bound by integer multiply-add issue"},
                                "roofline_valu": {"achieved": round(11 * m * 162 / ms / 1e9, 3), "peak": MAD_PEAK_T, "unit": "Tmad/s",
                                                  "frac": round(11 * m * 162 / ms / 1e9 / MAD_PEAK_T, 4),
                                                  "note": "log2(n)/2 = 11 field products of 162 v_mad_u64_u32 per element"}}
    del d

    # (3) Groth16 prove on the benchmark chain circuit (BASELINE config 4), witness as host limb arrays
    out.update(prove_metric(torch, args, None, 1, with_cpu_baseline=not args.no_cpu_baseline))
    if args.config5_log_n:
        # BASELINE configs[4] in its single-GPU form (the 8-rank form is the same call at --gpus 8)
        out.update(prove_metric(torch, args, None, 1, curve="BLS12_381", log_n=args.config5_log_n))

    # (4) PlonK prove on the same chain as gates, witness as a host limb array
    from zksnake_amd.arithmetization import Plonkish
    from zksnake_amd.plonk import Plonk
    gn = 1 << args.plonk_log_n
    r = constant.BN254_SCALAR_FIELD
    gates, perm, pub, priv = W.plonk_chain_gates(gn, r)
    plonk = Plonk(Plonkish.from_gates(gates["L"], gates["R"], gates["O"], gates["M"], gates["C"], perm, "BN254"), "BN254")
    plonk._tau = W.field_stream(W.SEED_PROVE, 1, r)[1][0]
    plonk._blinding = W.field_stream(W.SEED_PROVE, 11, r, offset=1)[1]
    plonk.setup()
    witness = N.ints_to_limbs(priv)
    times = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pproof = plonk.prove(pub, witness)
        times.append((time.perf_counter() - t0) * 1e3)
    ok = plonk.verify(pproof, pub)
    out[f"plonk_prove_bn254_2^{args.plonk_log_n}"] = {"ms": round(min(times[1:]), 3), "first_ms_incl_key_columns": round(times[0], 1), "verifies": bool(ok),
                                                     "proof_sha256": __import__("hashlib").sha256(pproof.to_bytes()).hexdigest()}
    if not ok:
        raise SystemExit("PlonK proof does not verify")
    return out


def large_msm_metric(lib, torch, args, dev, gather_dev, rank, world):
    """the same MSM at 2^--large-log-n pairs (default 2^24), window-sharded when world > 1: the size at which one MSM is long
    enough (25 ms on one GPU) for the per-rank fixed costs of the sharded form -- latency-bound bucket reduction, host tail,
    all_gather -- to stop dominating.  The expectation (sum s_i k_i) G comes from an element-wise product and a
    reduction on the GPU (zk_vec_op_dev, zk_poly_eval_dev at x = 1), not from the MSM code."""
    from zksnake_amd.frvec import DevVec, FrOps
    cid, grp, r = N.CURVE_BN254, N.G1, constant.BN254_SCALAR_FIELD
    n = 1 << args.large_log_n
    PW = N.point_limbs(cid, grp)
    sc = W.splitmix64(W.SEED_MSM_SCALARS + 1, 4 * n).reshape(n, 4)
    ks = W.splitmix64(W.SEED_MSM_BASES + 1, 4 * n).reshape(n, 4)
    sc[:, 3] &= np.uint64((1 << 60) - 1)   # < 2^252 < r
    ks[:, 3] &= np.uint64((1 << 60) - 1)
    gen = np.zeros(PW, dtype=np.uint64)
    N.check(lib.zk_point_generator(cid, grp, N.u64p(gen)))
    bases = np.zeros((n, PW), dtype=np.uint64)
    N.check(lib.zk_batch_mul(cid, grp, n, N.u64p(ks), N.u64p(gen), 1, N.u64p(bases)))
    V = FrOps(r)
    d_s, d_k, prod = V.d_from(sc), V.d_from(ks), DevVec(n, zero=False)
    V.d_mul(n, d_s.ptr(), d_k.ptr(), prod.ptr())
    dot = V.d_eval(n, prod.ptr(), 1)
    expected = np.zeros(PW, dtype=np.uint64)
    N.check(lib.zk_point_mul(cid, grp, N.u64p(gen), N.u64p(N.ints_to_limbs([dot])), N.u64p(expected)))
    del d_k, prod, ks
    handle = N._u64(0)
    N.check(lib.zk_msm_plan_create(cid, grp, n, bases.ctypes.data, 0, 0, args.window_bits, handle))
    del bases
    c_bits, nwin = N._i(0), N._i(0)
    N.check(lib.zk_msm_plan_windows(handle, c_bits, nwin))
    w_first, w_count = window_ranges(nwin.value, world)[rank]
    out = np.zeros(PW, dtype=np.uint64)

    def step():
        if w_count > 0:
            N.check(lib.zk_msm_plan_run(handle, n, d_s.ptr(), 1, w_first, w_count, N.u64p(out), None))
        else:
            out[:] = 0
        return out.copy() if world == 1 else all_gather_sum(cid, grp, out, gather_dev)

    res = step()
    if not (res == expected).all():
        raise SystemExit("large MSM does not match (sum s_i k_i) G")
    import torch.distributed as dist
    reps = 5
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        res = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = (time.perf_counter() - t0) / reps
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=gather_dev if gather_dev is not None else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if not (res == expected).all():
        raise SystemExit("large MSM result changed during the timed loop")
    N.check(lib.zk_msm_plan_destroy(handle))
    key = f"msm_bn254_g1_2^{args.large_log_n}" + (f"_window_sharded_x{world}" if world > 1 else "")
    return {key: {"ms": round(dt * 1e3, 3), "Mscalar/s": round(n / dt / 1e6, 2), "windows": nwin.value}}


def group_msm_metrics(lib, torch):
    """MSM at 2^20 pairs for BN254 G2 and both BLS12-381 groups (general path, scalars resident), checked against
    (sum s_i k_i) G with the sum computed on the GPU by the vector kernels, with both rooflines of the accumulate kernel"""
    from zksnake_amd.frvec import DevVec, FrOps
    out = {}
    n = 1 << 20
    for key, curve, grp in (("bn254_g2", "BN254", 2), ("bls12_381_g1", "BLS12_381", 1), ("bls12_381_g2", "BLS12_381", 2)):
        cid = N.curve_id(curve)
        r = W.scalar_field(curve)
        PW = N.point_limbs(cid, grp)
        sc = W.splitmix64(W.SEED_MSM_SCALARS + 16 + cid, 4 * n).reshape(n, 4)
        ks = W.splitmix64(W.SEED_MSM_BASES + 16 + cid, 4 * n).reshape(n, 4)
        sc[:, 3] &= np.uint64((1 << 60) - 1)
        ks[:, 3] &= np.uint64((1 << 60) - 1)
        gen = np.zeros(PW, dtype=np.uint64)
        N.check(lib.zk_point_generator(cid, grp, N.u64p(gen)))
        bases = np.zeros((n, PW), dtype=np.uint64)
        N.check(lib.zk_batch_mul(cid, grp, n, N.u64p(ks), N.u64p(gen), 1, N.u64p(bases)))
        V = FrOps(r)
        d_s, d_k, prod = V.d_from(sc), V.d_from(ks), DevVec(n, zero=False)
        V.d_mul(n, d_s.ptr(), d_k.ptr(), prod.ptr())
        dot = V.d_eval(n, prod.ptr(), 1)
        expected = np.zeros(PW, dtype=np.uint64)
        N.check(lib.zk_point_mul(cid, grp, N.u64p(gen), N.u64p(N.ints_to_limbs([dot])), N.u64p(expected)))
        h = N._u64(0)
        N.check(lib.zk_msm_plan_create(cid, grp, n, bases.ctypes.data, 0, 0, 0, h))
        del bases
        nw, cb = N._i(0), N._i(0)
        N.check(lib.zk_msm_plan_windows(h, cb, nw))
        ent = N._u64(0)
        N.check(lib.zk_msm_plan_entries(h, ent))
        res = np.zeros(PW, dtype=np.uint64)
        tm = (N.ctypes.c_float * 5)()
        for _ in range(2):
            N.check(lib.zk_msm_plan_run(h, n, d_s.ptr(), 1, 0, 0, N.u64p(res), None))
        if not (res == expected).all():
            raise SystemExit(f"{key}: MSM differs from (sum s_i k_i) G")
        reps, stages, walls = 7, [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            N.check(lib.zk_msm_plan_run(h, n, d_s.ptr(), 1, 0, 0, N.u64p(res), None))
            walls.append((time.perf_counter() - t0) * 1e3)
            lib.zk_msm_plan_timings(h, tm, 5)
            stages.append(list(tm))
        ms = float(np.median(walls))
        st = np.array(stages).mean(axis=0)
        acc_s = float(st[1]) * 1e-3
        mads = nw.value * ent.value * mads_per_mixed_add(cid, grp)
        out[f"msm_{key}_2^20"] = {
            "ms": round(ms, 4), "Mscalar/s": round(n / ms / 1e3, 2),
            "stage_ms": {"digits_sort": round(float(st[0]), 4), "accumulate": round(float(st[1]), 4), "reduce": round(float(st[2]), 4),
                         "host_tail": round(float(st[3]), 4)},
            "roofline": {"kernel": f"accumulate_kernel<{key}>", "bound": "hbm", "achieved": round(PAIR_BYTES[(cid, grp)] * n / acc_s / 1e9, 2),
                         "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(PAIR_BYTES[(cid, grp)] * n / acc_s / 1e9 / HBM_PEAK_GBPS, 5)},
            "roofline_valu": {"achieved": round(mads / acc_s / 1e12, 3), "peak": MAD_PEAK_T, "unit": "Tmad/s", "frac": round(mads / acc_s / 1e12 / MAD_PEAK_T, 4)}}
        N.check(lib.zk_msm_plan_destroy(h))
    return out


PAIR_BYTES = {(0, 1): 96, (0, 2): 160, (1, 1): 128, (1, 2): 224}   # scalar + affine base per pair
PROVE_BYTES_PER_CONSTRAINT = 4 * 96 + 160 + 9 * 64 + 2 * 96 + 3 * 32   # ~1.41 KB per constraint (BN254)


def mads_per_mixed_add(cid, grp):
    """v_mad_u64_u32 per XYZZ mixed addition: N 29-bit limbs (9 / 14): product 2N^2, squaring N(N+1)/2+N^2, double
    product 3N^2 (the N reduction quotients of each are v_mul_lo_u32, not counted); G1: six products, two squarings, Y3 as
    one double product; G2 (Fp2): a product is two double products, a squaring two products"""
    nl = 9 if cid == 0 else 14
    mul, sqr, mul2 = 2 * nl * nl, nl * (nl + 1) // 2 + nl * nl, 3 * nl * nl
    if grp == 1:
        return 6 * mul + 2 * sqr + mul2
    # G2 (relaxed Fp2 step): six Fp2 products of two double products, two squares of two products, and Y3 -- for nine limbs one
    # four-product reduction per component (5 N^2), for wider fields two more Fp2 products
    y3 = 2 * 5 * nl * nl if nl <= 9 else 2 * (2 * mul2)
    return 6 * (2 * mul2) + 2 * (2 * mul) + y3


def prove_cpu_baseline(g, A, B, C, w, threads):
    """the reference's prove path on the host, restated (oracle/zk_oracle.cpp): QAP quotient by radix-2 NTTs (three of size n,
    three of size 2n, as qap.py:51-67 does) + four G1 and one G2 ark-style Pippenger MSMs over the SAME proving key and
    witness as the timed GPU run, at the metric's full size.  `threads` = 1 is what the default zksnake wheel does (ark
    without its rayon feature); more threads parallelise the NTT butterflies and the MSM windows.
    Returns (seconds, proof bytes assembled from the CPU results)."""
    from oracle import corc  # checker / CPU baseline only
    from zksnake_amd.groth16 import Proof
    from zksnake_amd.ecc import EllipticCurve
    from zksnake_amd._algebra import _point_class
    pk = g.proving_key
    n = g.qap.a.n_row
    wl = N.ints_to_limbs(w)
    a = wl[np.asarray(A[1])]
    b = wl[np.asarray(B[1])]
    c = wl[np.asarray(C[1])]
    t0 = time.perf_counter()
    u, v, hq = corc.qap_h(0, a, b, c, threads=threads)
    m_u = corc.msm(0, 1, u, pk.tau_1.limbs[:n], threads=threads)
    m_v2 = corc.msm(0, 2, v, pk.tau_2.limbs[:n], threads=threads)
    m_v1 = corc.msm(0, 1, v, pk.tau_1.limbs[:n], threads=threads)
    m_h = corc.msm(0, 1, hq[:len(pk.target_1)], pk.target_1.limbs, threads=threads)
    m_k = corc.msm(0, 1, wl[2:], pk.kdelta_1.limbs, threads=threads)
    secs = time.perf_counter() - t0
    E = EllipticCurve("BN254")
    P1, P2 = _point_class(0, 1), _point_class(0, 2)
    rr, ss = g._blinding
    Apt = P1._from_limbs(m_u) + pk.alpha_1 + pk.delta_1 * rr
    B1 = P1._from_limbs(m_v1) + pk.beta_1 + pk.delta_1 * ss
    B2 = P2._from_limbs(m_v2) + pk.beta_2 + pk.delta_2 * ss
    Cpt = P1._from_limbs(m_h) + P1._from_limbs(m_k) + Apt * ss + B1 * rr + (-pk.delta_1) * (rr * ss % E.order)
    return secs, Proof(Apt, B2, Cpt).to_bytes()


def prove_metric(torch, args, shard_device, world, with_cpu_baseline=False, curve="BN254", log_n=None, partition="task"):
    """Groth16.prove on the benchmark chain circuit (benchmarks/benchmark_groth16.py:7-27 shape), pinned toxic waste and
    blinding so the proof is reproducible; timed region = prove() only, witness already on the host (benchmark_groth16.py:43-46).
    With world > 1 the proof is split over the ranks by task x window (Groth16.shard_over_ranks; partition="window": every MSM by
    window on every rank, the layout of rounds 1-3) and the time is the max over ranks.
    curve / log_n: BASELINE configs[3] by default (BN254, 2^20); configs[4] is BLS12-381 at 2^23 (reported at every N; the reference-call-shape
    and CPU legs only run for the default)."""
    import hashlib
    import statistics
    from zksnake_amd.arithmetization import R1CS
    from zksnake_amd.groth16 import Groth16
    headline_config = curve == "BN254" and log_n is None
    log_n = args.prove_log_n if log_n is None else log_n
    pn = 1 << log_n
    r = W.scalar_field(curve)
    A, B, C, w, n_col = W.chain_circuit(pn, r)
    g = Groth16(R1CS.from_triplets(A, B, C, pn, n_col, 2, curve), curve)
    g._toxic = tuple(W.field_stream(W.SEED_PROVE, 5, r)[1])
    g._blinding = tuple(W.field_stream(W.SEED_PROVE, 2, r, offset=5)[1])
    if world > 1:
        import torch.distributed as dist
        g.shard_over_ranks(shard_device, partition=partition)   # before setup(): the plans it prepares then hold this rank's share only
    t0 = time.perf_counter()
    g.setup()
    setup_s = time.perf_counter() - t0
    pub, prv = N.ints_to_limbs(w[:2]), N.ints_to_limbs(w[2:])
    # the workload itself lives in Python lists of 2^20 ints (triplets, witness): a full cyclic-GC pass over them costs
    # 10-25 ms and would land inside some proofs; freeze them out of the collector's sight (CPython gc.freeze)
    import gc
    gc.collect()
    gc.freeze()
    times, timelines = [], []
    for _ in range(8):
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        proof = g.prove(pub, prv)
        dt = (time.perf_counter() - t0) * 1e3
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=shard_device if shard_device is not None else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        times.append(dt)
        timelines.append(dict(g.last_timings))
    ok = g.verify(proof, w[:2])
    if not ok:
        raise SystemExit("Groth16 proof does not verify")
    steady = times[1:]
    med = statistics.median(steady)
    res = {"ms": round(med, 3), "ms_min": round(min(steady), 3), "ms_max": round(max(steady), 3), "proofs_timed": len(steady),
           "first_proof_ms": round(times[0], 1), "setup_s": round(setup_s, 3), "verifies": bool(ok),
           "timeline_ms": {k: round(statistics.median(t[k] for t in timelines[1:]), 3) for k in timelines[-1]},
           "proof_sha256": hashlib.sha256(proof.to_bytes()).hexdigest()}
    gpath = os.path.join(ROOT, "tests", "golden", "groth16_vectors.json")
    if os.path.exists(gpath):
        with open(gpath) as f:
            gold = json.load(f).get(curve, {}).get(str(log_n))
        if gold is not None:
            res["matches_committed_closed_form"] = bool(proof.to_bytes().hex() == gold["proof_hex"])
            if not res["matches_committed_closed_form"]:
                raise SystemExit("Groth16 proof bytes differ from the committed closed-form proof (tests/golden/groth16_vectors.json)")
    if world == 1 and headline_config:
        # (4 x 96 + 160 + 9 x 64 + 2 x 96 + 3 x 32) B per constraint over the whole prove
        gb = PROVE_BYTES_PER_CONSTRAINT * pn / 1e9
        from tools.fingerprint import load_traffic
        p_traffic, p_src = load_traffic("prove_traffic.json", "prove") if log_n == 20 else (None, None)
        res["roofline"] = {"bound": "hbm", "achieved": round(gb / (med * 1e-3), 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                           "frac": round(gb / (med * 1e-3) / HBM_PEAK_GBPS, 5), "algorithmic_GB": round(gb, 3), "traffic": p_traffic,
                           "traffic_source": p_src,
                           "note": "whole prove (host glue, witness upload over PCIe and five MSMs included), 1.41 KB per constraint "
                                   "(SURVEY 8d); the MSMs are bound by integer multiply-add issue, see roofline_valu of the MSM lines"}
        # the reference's call shape: two lists of Python ints (ints -> limbs on the host is part of the call)
        lt = []
        pub_l, prv_l = w[:2], w[2:]   # the reference benchmark hands prove() two existing lists (benchmark_groth16.py:43-46)
        for _ in range(4):
            t0 = time.perf_counter()
            proof_l = g.prove(pub_l, prv_l)
            lt.append((time.perf_counter() - t0) * 1e3)
            if proof_l.to_bytes() != proof.to_bytes():
                raise SystemExit("list[int] and limb-array witnesses give different proofs")
        res["list_int_api_ms"] = round(statistics.median(lt[1:]), 2)
        res["list_int_api_first_ms"] = round(lt[0], 2)
        # the same limb arrays in page-locked host memory (zk_host_alloc): the witness upload runs at the link rate
        from zksnake_amd.device import PinnedArray
        pin = PinnedArray(prv.shape)
        pin.array[:] = prv
        pt = []
        for _ in range(6):
            t0 = time.perf_counter()
            proof_p = g.prove(pub, pin.array)
            pt.append((time.perf_counter() - t0) * 1e3)
            if proof_p.to_bytes() != proof.to_bytes():
                raise SystemExit("pinned and pageable witnesses give different proofs")
        res["pinned_witness_ms"] = round(statistics.median(pt[1:]), 3)
        del proof_p
        pin.free()
    if with_cpu_baseline:
        # the same circuit, key, witness and blinding at the metric's full size (round-2 verdict: no extrapolated sample)
        secs, cpu_bytes = prove_cpu_baseline(g, A, B, C, w, 1)
        if cpu_bytes != proof.to_bytes():
            raise SystemExit("the CPU restatement and the GPU prover disagree on the proof bytes")
        sample = (f"the same proof at the full 2^{log_n} constraints (same key, witness and blinding): QAP quotient (radix-2 NTTs: "
                  "three of size n, three of size 2n) + four G1 and one G2 ark-style Pippenger MSMs, oracle/zk_oracle.cpp; its proof "
                  "bytes equal the GPU prover's")
        res["cpu_baseline"] = {"value": round(secs * 1e3, 1), "unit": "ms", "cores": 1, "kind": "port",
                               "sample": sample + "; 1 thread (the default zksnake wheel runs arkworks single-threaded)"}
        cores = min(os.cpu_count() or 1, 16)
        secs_all, cpu_bytes = prove_cpu_baseline(g, A, B, C, w, cores)
        if cpu_bytes != proof.to_bytes():
            raise SystemExit("the CPU restatement (all cores) and the GPU prover disagree on the proof bytes")
        res["cpu_baseline_all_cores"] = {"value": round(secs_all * 1e3, 1), "unit": "ms", "cores": cores, "kind": "port",
                                         "sample": sample + f"; {cores} threads over the NTT butterflies and the MSM windows (rayon-style; "
                                                            f"the host has {os.cpu_count()} logical cores)"}
    if world > 1:
        # what the driver's scaling curve is made of, rank by rank: the MSM windows a rank holds, the part of the QAP it evaluates
        # for them (none / u / v / the whole chain), its timeline, and the cost model's projection the partition was cut by
        tl = res["timeline_ms"]
        mine = {"rank": dist.get_rank(), "tasks": {t: list(r) for t, r in (g._my_tasks() or {}).items()},
                "qap_outputs": sorted(g._qap_needs() or []),
                "qap_ms": round(tl["qap_ms"], 3),
                "msm_ms": round(tl["msm_enqueue_ms"] + tl["msm_finish_ms"], 3),
                "exchange_assemble_ms": round(tl["exchange_assemble_ms"], 3), "collective_ms": round(tl.get("collective_ms", 0.0), 3),
                "projected_ms": (g.projected_ms[dist.get_rank()] if g.projected_ms else None)}
        table = [None] * world
        dist.all_gather_object(table, mine)
        res["partition"] = partition
        res["per_rank"] = table
        res["slowest_rank_before_collective_ms"] = round(max(t["qap_ms"] + t["msm_ms"] for t in table), 3)
        res["note"] = ("task x window partition (zksnake_amd/parallel.py): one MSM, or a window range of a long one, per rank; only the "
                       "ranks holding <target_1, h> run the whole QAP chain; one all_gather of partial points + ok flag"
                       if partition == "task" else "every MSM window-sharded on every rank, QAP replicated (the layout of rounds 1-3)")
    key = f"groth16_prove_{curve.lower()}_2^{log_n}" + (f"_{partition}_partition_x{world}" if world > 1 else "")
    del g
    gc.unfreeze()
    gc.collect()
    return {key: res}


if __name__ == "__main__":
    main()
