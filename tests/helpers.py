"""shared test helpers: seeded inputs and oracle-backed expectations (the oracle is only the checker)."""

import random

import numpy as np

from oracle import corc, pyref
from zksnake_amd import _native as N

CURVES = (("BN254", 0), ("BLS12_381", 1))


def rand_scalars(n, r, seed):
    rnd = random.Random(seed)
    vals = [rnd.randrange(r) for _ in range(n)]
    return vals, N.ints_to_limbs(vals, 4)


def rand_limbs(n, seed, top_bits=60):
    """(n,4) uint64 values below 2^(192+top_bits) -- cheap to generate at 2^20+ sizes"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    v[:, 3] &= np.uint64((1 << top_bits) - 1)
    return v


def generator_limbs(lib, cid, grp):
    out = np.zeros(N.point_limbs(cid, grp), dtype=np.uint64)
    N.check(lib.zk_point_generator(cid, grp, N.u64p(out)))
    return out


def oracle_bases(cid, grp, n, seed):
    """n points k_i * G from the C++ oracle (k_i seeded)"""
    cv = pyref.curve_by_name("BN254" if cid == 0 else "BLS12_381")
    ks, kl = rand_scalars(n, cv.r, seed)
    g = pyref.Group(cv, grp)
    pts = corc.batch_mul(cid, grp, kl, corc.points_to_limbs([g.gen], cid, grp)[0])
    return ks, pts


def window_range_scalars(cid, grp, vals, c, nwin, glv, first, count):
    """scalars e_i with sum_i e_i P_i == the partial point of a plan run over the windows [first, first + count): the signed
    digits of those windows alone, d_w = (bits [cw, cw + c) of s + bias) - 2^(c-1), put back at their places (the integer model
    of tests/msm_front_model.py); a split-scalar plan cuts the two signed halves, s = k1 + lambda k2 (mod r), and the partial
    scalar is e(k1) + lambda e(k2).  The expected point is then the CPU oracle's MSM of these scalars."""
    import msm_front_model as FM
    import reduce_model as RM
    G = RM.GROUPS[2 * cid + grp - 1]
    bias, mask, B = FM.bias_of(c, nwin), (1 << c) - 1, 1 << (c - 1)

    def part(v):
        t = v + bias
        assert t >= 0
        return sum(((((t >> (c * w)) & mask) - B) << (c * w)) for w in range(first, first + count))

    if not glv:
        return [part(s % G.r) % G.r for s in vals]
    cs = FM.glv_consts(G)
    out = []
    for s in vals:
        k1, k2 = FM.glv_halves(s % G.r, cs)
        out.append((part(k1) + cs["lam"] * part(k2)) % G.r)
    return out


# ---- stage harnesses: one tests/native source built for the device as the library itself is ------------------------------
def build_device_harness(src, d, env_var=None, timeout=1500):
    """tests/native/<name>.hip -> <d>/<name>_dev.so through the library's own pipeline (csrc/hipcc_noreassoc.sh with the
    Makefile's HIPFLAGS_NOARCH, gfx950); env_var, when set in the environment, names an already built one"""
    import os
    import subprocess
    pre = os.environ.get(env_var) if env_var else None
    if pre:
        return pre
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zksnake_amd", "csrc")
    flags = None
    with open(os.path.join(csrc, "Makefile")) as fh:
        for line in fh:
            if line.startswith("HIPFLAGS_NOARCH"):
                flags = line.split("?=", 1)[1].split()
    assert flags
    name = os.path.splitext(os.path.basename(src))[0]
    obj, so = os.path.join(str(d), name + ".o"), os.path.join(str(d), name + "_dev.so")
    env = dict(os.environ, ARCH="gfx950", TMPDIR=str(d))
    subprocess.run(["bash", os.path.join(csrc, "hipcc_noreassoc.sh"), obj, src] + flags, check=True, timeout=timeout, env=env)
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so, obj], check=True, timeout=300)
    return so


# ---- stand-alone host programs: the host side of a HIP source under the address and undefined-behaviour sanitizers ----------
def run_host_program(name, tmp_path, args=(), timeout=300):
    """tests/native/<name>.cpp -> a program of its own, built and run: a host-only hipcc compile, an EMPTY offload bundle for the
    __hip_fatbin_<hash> symbols the object refers to, link, run with every device hidden.  The sanitizer runtimes are linked into
    the program; nothing is loaded into Python.  Returns the finished process (returncode, stdout, stderr); skips without hipcc."""
    import os
    import re
    import shutil
    import subprocess
    import pytest
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    obj, stub, exe = str(tmp_path / f"{name}.o"), str(tmp_path / f"{name}_stub"), str(tmp_path / name)
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-mbmi2", "-madx",
                           "-DZK_NOINLINE_MUL", *san, "-c", os.path.join(root, "tests", "native", name + ".cpp"), "-o", obj], timeout=600)
    undefined = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout
    syms = sorted(set(re.findall(r"__hip_fatbin_[0-9a-f]+", undefined)))
    assert syms, "the host-only object names no device image"
    magic = ",".join(f"'{c}'" for c in "__CLANG_OFFLOAD_BUNDLE__")
    with open(stub + ".cpp", "w") as f:   # the magic string and a bundle count of zero: registered at load time, never looked into
        f.write("#include <stdint.h>\nstruct bundle { char magic[24]; uint64_t count; };\n")
        for sym in syms:
            f.write(f'extern "C" __attribute__((aligned(4096))) const bundle {sym} = {{{{{magic}}}, 0}};\n')
    subprocess.check_call(["g++", "-O0", "-c", stub + ".cpp", "-o", stub + ".o"], timeout=600)
    subprocess.check_call([hipcc, "--offload-host-only", *san, "-o", exe, obj, stub + ".o"], timeout=600)
    # on a machine with a GPU driver the HSA runtime starts up even with every device hidden and leaves 144 bytes of its own
    # behind at exit; the leak check stays on for everything else
    supp = tmp_path / "lsan.supp"
    supp.write_text("leak:libhsa-runtime64\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", LSAN_OPTIONS=f"suppressions={supp}:print_suppressions=0")
    return subprocess.run([exe, *map(str, args)], env=env, capture_output=True, text=True, timeout=timeout)


# ---- multi-process tests: ranks as spawned children that report through a queue ---------------------------------------
def rank_entry(worker, rank, q, args):
    """child side: run worker(rank, *args) -> result; the result or the child's traceback goes back through the queue"""
    import traceback
    try:
        q.put(("ok", rank, worker(rank, *args)))
    except BaseException:  # noqa: BLE001 - reported to the parent, which fails the test with this text
        q.put(("error", rank, traceback.format_exc()))
        raise


def run_ranks(worker, world, args=(), timeout=300, poll=0.5):
    """spawn `world` children running worker(rank, *args) and return their results ordered by rank.  The parent polls the
    queue in short intervals and fails AS SOON AS a child has reported a traceback or has exited non-zero without a result
    (round 3: a child that died early left the parent in q.get(timeout=300) until pytest-timeout killed the run)."""
    import queue as _queue
    import time
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=rank_entry, args=(worker, r, q, tuple(args))) for r in range(world)]
    for p in procs:
        p.start()
    results, deadline = {}, time.monotonic() + timeout
    try:
        while len(results) < world:
            try:
                kind, rank, payload = q.get(timeout=poll)
            except _queue.Empty:
                dead = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode not in (None, 0) and r not in results]
                if dead:
                    # give a traceback that is already on its way a moment to arrive
                    try:
                        kind, rank, payload = q.get(timeout=2.0)
                    except _queue.Empty:
                        raise AssertionError(f"rank(s) {dead} exited (rank, code) without a result") from None
                elif time.monotonic() > deadline:
                    raise AssertionError(f"ranks {sorted(set(range(world)) - set(results))} did not report within {timeout} s") from None
                else:
                    continue
            if kind == "error":
                raise AssertionError(f"rank {rank} failed:\n{payload}")
            results[rank] = payload
        for p in procs:
            p.join(60)
            assert p.exitcode == 0, f"a rank exited with code {p.exitcode}"
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join(10)
    return [results[r] for r in range(world)]
