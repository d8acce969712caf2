"""CPU: the C-ABI shared library loads, exports every symbol include/zkmi.h declares, and its host-side
functions (single-point arithmetic, codecs, scalar helpers) agree with the oracle.  No GPU compute."""

import os
import random
import re

import numpy as np
import pytest

from oracle import corc, pyref as R
from zksnake_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = (("BN254", 0), ("BLS12_381", 1))


def test_header_symbols_are_exported_and_bound(lib):
    with open(os.path.join(ROOT, "include", "zkmi.h")) as f:
        text = f.read()
    declared = set(re.findall(r"\b(zk_[a-z0-9_]+)\s*\(", text))
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in include/zkmi.h but not exported by libzkmi.so"
    assert declared == set(N.SIGNATURES), declared ^ set(N.SIGNATURES)
    assert lib.zk_version().startswith(b"zkmi")


def test_sizes(lib):
    assert [lib.zk_fq_limbs(c) for c in (0, 1, 2)] == [4, 6, -1]
    assert [lib.zk_point_limbs(0, 1), lib.zk_point_limbs(0, 2), lib.zk_point_limbs(1, 1), lib.zk_point_limbs(1, 2)] == [8, 16, 12, 24]
    assert [lib.zk_point_bytes(0, 1), lib.zk_point_bytes(0, 2), lib.zk_point_bytes(1, 1), lib.zk_point_bytes(1, 2)] == [32, 64, 48, 96]


def test_no_gpu_fails_loudly(lib):
    """without a GPU the compute entry points must report ZK_ERR_HIP, never fall back to the CPU"""
    if lib.zk_device_count() > 0:
        pytest.skip("a GPU is visible")
    assert lib.zk_init(0) == N.ZK_ERR_HIP
    assert b"no CPU fallback" in lib.zk_last_error()
    a = np.zeros((4, 4), dtype=np.uint64)
    out = np.zeros((4, 4), dtype=np.uint64)
    assert lib.zk_ntt(0, 0, 0, 4, N.u64p(a), 4, N.u64p(out)) == N.ZK_ERR_HIP
    bases = np.zeros((4, 8), dtype=np.uint64)
    res = np.zeros(8, dtype=np.uint64)
    assert lib.zk_msm(0, 1, 4, 4, N.u64p(a), N.u64p(bases), N.u64p(res)) == N.ZK_ERR_HIP
    with pytest.raises(N.ZkError):
        N.ensure_gpu()


def _queue_probe(code, env_extra):
    """run `code` in a fresh interpreter (the decision is taken once per process) and return its stdout lines"""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "ZKMI_TEST_RUNTIME_STARTED", "ZKMI_HW_QUEUES_SET_BY_LIBRARY")}
    env.update(env_extra)
    env["PYTHONPATH"] = ROOT
    res = subprocess.run([sys.executable, "-W", "always", "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    return res.stdout.split(), res.stderr


_QUEUE_CODE = """
import ctypes
{first}
from zksnake_amd import _native as N
lib = N.load()
{second}
q = ctypes.c_int(-1)
st = lib.zk_hw_queues_prepare(ctypes.byref(q))
libc = ctypes.CDLL(None); libc.getenv.restype = ctypes.c_char_p
st2, q2 = ctypes.c_int(-1), ctypes.c_int(-1)
rc = lib.zk_init_ex(0, ctypes.byref(st2), ctypes.byref(q2))
print(st, q.value, (libc.getenv(b"GPU_MAX_HW_QUEUES") or b"-").decode(), N.queue_status, st2.value, q2.value)
"""


@pytest.mark.parametrize("order", ["torch_first", "lib_first"])
def test_hw_queues_are_set_by_the_library_in_either_import_order(order):
    """GPU_MAX_HW_QUEUES is put in place by the C library (zk_hw_queues_prepare / zk_init), not by a Python import side
    effect: unset -> the library sets 12 before its first HIP call, whichever of torch and the library is imported first
    (importing torch does not start the HIP runtime); the status is the same from every entry point"""
    first, second = ("import torch", "") if order == "torch_first" else ("", "import torch")
    out, _ = _queue_probe(_QUEUE_CODE.format(first=first, second=second), {})
    assert out == [str(N.QUEUES_SET_BY_LIBRARY), "12", "12", str(N.QUEUES_SET_BY_LIBRARY), str(N.QUEUES_SET_BY_LIBRARY), "12"]


def test_hw_queues_caller_setting_wins_and_late_start_is_reported():
    out, _ = _queue_probe(_QUEUE_CODE.format(first="", second=""), {"GPU_MAX_HW_QUEUES": "4"})
    assert out == [str(N.QUEUES_CALLER), "4", "4", str(N.QUEUES_CALLER), str(N.QUEUES_CALLER), "4"]
    # the runtime already running (a C-ABI consumer whose host initialised HIP first): reported, warned about, nothing set
    out, err = _queue_probe(_QUEUE_CODE.format(first="", second=""), {"ZKMI_TEST_RUNTIME_STARTED": "1"})
    assert out == [str(N.QUEUES_TOO_LATE), "0", "-", str(N.QUEUES_TOO_LATE), str(N.QUEUES_TOO_LATE), "0"]
    assert "GPU_MAX_HW_QUEUES" in err and "RuntimeWarning" in err


@pytest.mark.parametrize("name,cid", CURVES)
@pytest.mark.parametrize("grp", [1, 2])
def test_point_arithmetic_and_codec(lib, name, cid, grp):
    cv = R.curve_by_name(name)
    g = R.Group(cv, grp)
    rnd = random.Random(5)
    W = N.point_limbs(cid, grp)
    gen = np.zeros(W, dtype=np.uint64)
    N.check(lib.zk_point_generator(cid, grp, N.u64p(gen)))
    assert corc.limbs_to_points(gen, cid, grp)[0] == g.gen and lib.zk_point_on_curve(cid, grp, N.u64p(gen)) == 1
    pts = []
    for k in [0, 1, 2, cv.r - 1, cv.r, cv.r + 5] + [rnd.randrange(cv.r) for _ in range(4)]:
        out = np.zeros(W, dtype=np.uint64)
        N.check(lib.zk_point_mul(cid, grp, N.u64p(gen), N.u64p(N.ints_to_limbs([k])), N.u64p(out)))
        P = corc.limbs_to_points(out, cid, grp)[0]
        assert P == g.mul(g.gen, k)
        pts.append((out, P))
    nb = lib.zk_point_bytes(cid, grp)
    for a, Pa in pts:
        for b, Pb in pts[:5]:
            out = np.zeros(W, dtype=np.uint64)
            N.check(lib.zk_point_add(cid, grp, N.u64p(a), N.u64p(b), N.u64p(out)))
            assert corc.limbs_to_points(out, cid, grp)[0] == g.add(Pa, Pb)
        buf = np.zeros(nb, dtype=np.uint8)
        N.check(lib.zk_point_compress(cid, grp, N.u64p(a), N.u8p(buf)))
        assert bytes(buf) == R.compress(cv, grp, Pa)
        back = np.zeros(W, dtype=np.uint64)
        N.check(lib.zk_point_decompress(cid, grp, N.u8p(buf), N.u64p(back)))
        assert (back == a).all()
        neg = np.zeros(W, dtype=np.uint64)
        N.check(lib.zk_point_neg(cid, grp, N.u64p(a), N.u64p(neg)))
        assert corc.limbs_to_points(neg, cid, grp)[0] == g.neg(Pa)
    # rejected encodings: bad flags, x off the curve
    back = np.zeros(W, dtype=np.uint64)
    bad = np.frombuffer(bytes([0xFF] * nb), dtype=np.uint8).copy()
    assert lib.zk_point_decompress(cid, grp, N.u8p(bad), N.u64p(back)) == N.ZK_ERR_POINT
    off = np.zeros(W, dtype=np.uint64)
    off[0] = 5
    assert lib.zk_point_on_curve(cid, grp, N.u64p(off)) == 0


@pytest.mark.parametrize("name,cid", CURVES)
@pytest.mark.parametrize("grp", [1, 2])
def test_point_codec_against_the_integer_model(lib, name, cid, grp):
    """every case of codec_model.cases (each decode branch and validation edge) through the per-point host codec, which runs the
    routines of the batched kernels: the model's status message and, when accepted, the model's point limb for limb; a refused
    call leaves the caller's buffer alone; an accepted point compresses back to the bytes it came from"""
    import codec_model as M
    cv = R.curve_by_name(name)
    W, nb = N.point_limbs(cid, grp), lib.zk_point_bytes(cid, grp)
    sentinel = np.uint64(0xA5A5A5A5A5A5A5A5)
    for label, data, status, pt in M.cases(cv, grp, 1):
        out = np.full(W, sentinel, dtype=np.uint64)
        rc = lib.zk_point_decompress(cid, grp, N.u8p(np.frombuffer(data, dtype=np.uint8).copy()), N.u64p(out))
        if status != "CODEC_OK":
            assert rc == N.ZK_ERR_POINT and lib.zk_last_error() == M.MESSAGE[status], (label, data.hex(), rc, lib.zk_last_error())
            assert (out == sentinel).all(), (label, data.hex())
            continue
        assert rc == 0, (label, data.hex(), lib.zk_last_error())
        assert (out == corc.points_to_limbs([pt], cid, grp)[0]).all(), (label, data.hex())
        buf = np.full(nb, 0xA5, dtype=np.uint8)
        N.check(lib.zk_point_compress(cid, grp, N.u64p(out), N.u8p(buf)))
        assert bytes(buf) == data == M.encode_point(cv, grp, pt), label
    # compression takes reduced coordinates: x + p, y + p (one component at a time) and p itself are refused; so is an off-curve
    # point; a refused call leaves the caller's bytes alone
    g = R.Group(cv, grp)
    P = g.mul(g.gen, 5)
    flat = [P[0], P[1]] if grp == 1 else [*P[0], *P[1]]
    for k in range(len(flat)):
        for v in (flat[k] + cv.p, cv.p):
            row = np.array(N.ints_to_limbs(flat[:k] + [v] + flat[k + 1:], W // len(flat)), dtype=np.uint64).reshape(-1)
            buf = np.full(nb, 0xA5, dtype=np.uint8)
            assert lib.zk_point_compress(cid, grp, N.u64p(row), N.u8p(buf)) == N.ZK_ERR_POINT
            assert lib.zk_last_error() == M.MESSAGE["CODEC_COORD_RANGE"] and (buf == 0xA5).all()
    row = corc.points_to_limbs([P], cid, grp)[0].copy()
    row[0] ^= 1
    buf = np.full(nb, 0xA5, dtype=np.uint8)
    assert lib.zk_point_compress(cid, grp, N.u64p(row), N.u8p(buf)) == N.ZK_ERR_POINT
    assert lib.zk_last_error() == M.MESSAGE["CODEC_NOT_ON_CURVE"] and (buf == 0xA5).all()


def test_golden_encodings(lib):
    import json
    with open(os.path.join(ROOT, "tests", "golden", "oracle_vectors.json")) as f:
        gold = json.load(f)
    for name, cid in CURVES:
        for grp in (1, 2):
            og = gold[name][f"g{grp}"]
            W = N.point_limbs(cid, grp)
            nb = lib.zk_point_bytes(cid, grp)
            gen = np.zeros(W, dtype=np.uint64)
            N.check(lib.zk_point_generator(cid, grp, N.u64p(gen)))
            buf = np.zeros(nb, dtype=np.uint8)
            N.check(lib.zk_point_compress(cid, grp, N.u64p(gen), N.u8p(buf)))
            assert bytes(buf).hex() == og["generator_compressed"]
            N.check(lib.zk_point_compress(cid, grp, N.u64p(np.zeros(W, dtype=np.uint64)), N.u8p(buf)))
            assert bytes(buf).hex() == og["infinity_compressed"]
            # dlog * G compresses to the recorded MSM result
            out = np.zeros(W, dtype=np.uint64)
            N.check(lib.zk_point_mul(cid, grp, N.u64p(gen), N.u64p(N.ints_to_limbs([int(og["msm_dlog"])])), N.u64p(out)))
            N.check(lib.zk_point_compress(cid, grp, N.u64p(out), N.u8p(buf)))
            assert bytes(buf).hex() == og["msm_compressed"]


@pytest.mark.parametrize("name,cid", CURVES)
def test_scalar_field_helpers(lib, name, cid):
    cv = R.curve_by_name(name)
    rnd = random.Random(6)
    for n in (1, 2, 8, 64, 1 << 20):
        out = np.zeros(4, dtype=np.uint64)
        N.check(lib.zk_fr_root_of_unity(cid, n, N.u64p(out)))
        assert N.limbs_to_ints(out.reshape(1, 4))[0] == cv.root_of_unity(n)
    for n in (1, 2, 8, 64):
        for tau in (rnd.randrange(cv.r), cv.root_of_unity(n) if n > 1 else 1, 1, cv.r + 3):
            o = np.zeros((n, 4), dtype=np.uint64)
            N.check(lib.zk_fr_lagrange_coeffs(cid, n, N.u64p(N.ints_to_limbs([tau])), N.u64p(o)))
            assert N.limbs_to_ints(o) == R.lagrange_at(n, tau % cv.r, cv)
    out = np.zeros(4, dtype=np.uint64)
    assert lib.zk_fr_root_of_unity(cid, 1 << 40, N.u64p(out)) == N.ZK_ERR_DOMAIN


def test_relaxed_g2_step_host_build_and_integer_models(tmp_path):
    """the relaxed-range G2 mixed addition of the accumulate kernel: (1) a host build of the library's own field / curve code
    runs it against the plain formulas on chains of additions with the special cases (tests/native/relaxed_g2_check.cpp);
    (2) the integer models replay its limb operations, and those of the lazy NTT butterfly, with every limb, column-sum
    and value bound asserted on inputs pushed to the ends of their ranges (tools/model_relaxed_g2.py, tools/model_lazy_ntt.py)"""
    import subprocess
    import sys
    exe = str(tmp_path / "relaxed_g2_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "relaxed_g2_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.count(": ok") == 2, res.stdout + res.stderr
    for model in ("model_relaxed_g2.py", "model_lazy_ntt.py"):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", model)], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and "ok" in res.stdout, res.stdout + res.stderr


def test_dev_buf_gives_every_block_back_exactly_once(tmp_path):
    """DevBuf (csrc/dev_buf.h), the owner of every cached device block, against counting stand-ins for the allocator
    (tests/native/dev_buf_check.cpp): scope end, alloc on a holder, a failing alloc, moves, a double reset, shared ownership
    and an early return past three buffers each end with the blocks handed out equal to the blocks returned, none of them
    twice.  A host program under the address and undefined-behaviour sanitizers; no GPU and no device code.  The sanitizer
    runtimes are linked into the program, so it runs as it is whatever else the environment loads into a process."""
    import subprocess
    exe = str(tmp_path / "dev_buf_check")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "native", "dev_buf_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.count(": ok") == 7 and "all ok" in res.stdout, res.stdout + res.stderr


def test_ntt_pass_plan_equals_its_integer_model(tmp_path):
    """ntt_plan (csrc/ntt_plan.h), which ntt_dev_impl loops over, printed for log_n = 0 .. 30 by tests/native/ntt_plan_check.cpp
    and compared line by line with qap_model.plan, the copy the GPU chain tests derive their sizes from.  A host program under
    the address and undefined-behaviour sanitizers, their runtimes linked in; no GPU and no device code."""
    import subprocess
    import qap_model
    exe = str(tmp_path / "ntt_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "native", "ntt_plan_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == 31
    for log_n, line in enumerate(lines):
        assert line == f"{log_n}:" + "".join(f" {m},{q}" for m, q in qap_model.plan(log_n)), line


def test_msm_reduce_plan_equals_its_integer_model(tmp_path):
    """reduce_shape / reduce_plan (csrc/msm_reduce_plan.h), which MsmPlan sizes its buffers and launches its strided sums from,
    printed by tests/native/reduce_plan_check.cpp and compared word for word with reduce_model.one_step_jobs / two_step_jobs, the
    copies the GPU stage tests build their arrays from, plus the selection rule and the shape written out here: c = 2 .. 20 (17
    and 20 wide), 1 .. 16 bucket sets (which crosses 2^18 buckets both ways at c = 16), both settings of sum_one_step, three of
    lanes_per_output.  A host program under the address and undefined-behaviour sanitizers, their runtimes linked in; no GPU."""
    import subprocess
    import reduce_model as M
    exe = str(tmp_path / "reduce_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "native", "reduce_plan_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    cases = [(c, groups, one_step, lpo) for c in (2, 3, 4, 9, 15, 16, 17, 20) for groups in (1, 2, 8, 16) for one_step in (0, 1) for lpo in (0, 2, 64)]
    assert len(lines) == len(cases)
    step_counts = set()
    for (c, groups, one_step, lpo_opt), line in zip(cases, lines):
        wide = c > 16
        B = 1 << (c - 1)
        R = 1 << min(-(-(c - 1) // 2), 20 if wide else 8)   # 2^ceil((c - 1) / 2), at most 2^8 unless wide
        C = B // R
        K = 16 if R >= 64 and C >= 64 else 0
        two = not one_step and groups * B >= 1 << 18 and K >= 2 and C % K == 0 and R % K == 0 and C // K >= 2 and R // K >= 2
        if two:
            (prow, pcol), (frow, fcol), lpo2 = M.two_step_jobs(groups, R, C, K)
            steps = [(prow, pcol, 2), (frow, fcol, lpo2)]
        else:
            rows, cols = M.one_step_jobs(groups, R, C)
            steps = [(rows, cols, lpo_opt or (32 if groups * (R + C) >= 4096 else 64))]
        want = f"{c} {int(wide)} {groups} {one_step} {lpo_opt}: {B} {R} {C} {-(-R // 128)} {-(-C // 128)} {K} | {len(steps)}"
        for j0, j1, lpo in steps:
            want += " | " + " ".join(str(int(w)) for w in list(j0.words()) + list(j1.words()) + [lpo])
        assert line == want, (line, want)
        step_counts.add((c, groups, len(steps)))
    # the threshold is crossed both ways at c = 16, and a wide set takes two steps on its own
    assert {(16, 2, 1), (16, 8, 2), (20, 1, 2), (15, 16, 2), (15, 8, 1)} <= step_counts


def _tail_shape(c, wide):
    """R, C, weighted-sum blocks per row array and per column array, log2 C: the reduction shape of c-bit windows"""
    R = 1 << min(-(-(c - 1) // 2), 20 if wide else 8)
    C = (1 << (c - 1)) // R
    return R, C, -(-R // 128), -(-C // 128), C.bit_length() - 1


def _tail_scalar(s, c, shape_c, wide, groups, q_first, pre):
    """the multiple of the generator msm_host_tail must return when block i of h_final is s[i] G, from the formula in its comment:
    per bucket set W = 2^(lc+7) X_R + 2^lc sum S_k + 2^7 X_C + (sum S'_k + sum T_k), X = sum_k k T_k, over the row blocks (S_k, T_k)
    and the column blocks (S'_k, T'_k); total = sum_g 2^(c (q_first + g)) W_g, or W_0 alone in fixed-base mode"""
    _, _, bpr, bpc, lc = _tail_shape(shape_c, wide)
    assert len(s) == 2 * groups * (bpr + bpc)
    total = 0
    for g in range(groups):
        rows = [(s[(g * bpr + k) * 2], s[(g * bpr + k) * 2 + 1]) for k in range(bpr)]
        cols = [(s[(groups * bpr + g * bpc + k) * 2], s[(groups * bpr + g * bpc + k) * 2 + 1]) for k in range(bpc)]
        x_r, x_c = sum(k * t for k, (_, t) in enumerate(rows)), sum(k * t for k, (_, t) in enumerate(cols))
        w = (x_r << (lc + 7)) + (sum(sk for sk, _ in rows) << lc) + (x_c << 7) + sum(sk for sk, _ in cols) + sum(t for _, t in rows)
        total += w if pre else w << (c * (q_first + g))
    return total


def test_msm_host_tail_against_integers(tmp_path):
    """msm_host_tail (csrc/msm_host_tail.h), the stage between the last kernel of an MSM and its result, for all four groups on
    blocks that are known multiples s_i G (tests/native/host_tail_check.cpp builds them with the library's own host arithmetic):
    the affine point it returns must be (the integer formula of _tail_scalar) G by pyref, exactly.  Shapes: c = 4 (one block per
    array), c = 16 (two row blocks), c = 20 fixed-base (eight row blocks, four column blocks); general mode with 1 and 3 bucket sets
    and q_first 0 and 2.  Inputs: random multiples with a quarter of the blocks at infinity; one block solved for so that the total
    is infinity; every block the same point (the additions double); blocks alternating between a point and its negative (they
    cancel); every block at infinity.  The refusal "reduction layout does not fit the window" is asked for once; no shape of
    reduce_shape reaches it (lc + 7 <= c for every c with more than one row block), so the case pairs the blocks of c = 16 with
    13-bit windows.  A host program under the address and undefined-behaviour sanitizers, their runtimes linked in; no GPU."""
    import subprocess
    import reduce_model as M
    exe = str(tmp_path / "host_tail_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "native", "host_tail_check.cpp")], timeout=600)
    rnd = random.Random(8)
    configs = [(c, 0, groups, q_first, 0) for c in (4, 16) for groups in (1, 3) for q_first in (0, 2)] + [(20, 1, 1, 0, 1)]
    cases = []
    for G in M.GROUPS:
        for c, wide, groups, q_first, pre in configs:
            kinds = ["mixed", "total_inf"] + (["equal", "opposite", "all_inf"] if groups == 1 and q_first == 0 else [])
            for kind in kinds:
                _, _, bpr, bpc, _ = _tail_shape(c, wide)
                n = 2 * groups * (bpr + bpc)
                a = rnd.randrange(1, 1 << 64)
                if kind == "mixed":
                    s = [0 if rnd.random() < 0.25 else rnd.randrange(1, 1 << 64) for _ in range(n)]
                elif kind == "total_inf":
                    # the first column block's S of set 0 enters the total with the factor 2^(c q_first) (1 in fixed-base mode)
                    s = [rnd.randrange(1, 1 << 64) for _ in range(n)]
                    fix = 2 * groups * bpr
                    s[fix] = 0
                    rest = _tail_scalar(s, c, c, wide, groups, q_first, pre)
                    s[fix] = -rest * pow(1 if pre else 1 << (c * q_first), -1, G.r) % G.r
                elif kind == "equal":
                    s = [a] * n
                elif kind == "opposite":
                    s = [a if i % 2 == 0 else G.r - a for i in range(n)]
                else:
                    s = [0] * n
                cases.append((G, kind, (c, c, wide, groups, q_first, pre), s))
    G0 = M.GROUPS[0]
    refusal = (G0, "refusal", (13, 16, 0, 2, 0, 0), [rnd.randrange(1, 1 << 64) for _ in range(2 * 2 * 3)])
    text = "".join(f"{G.gid} {' '.join(map(str, cfg))} {len(s)}\n" + "".join(f"{v:x}\n" for v in s) for G, _, cfg, s in cases + [refusal])
    res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == len(cases) + 1
    infinities = 0
    for (G, kind, cfg, s), line in zip(cases, lines):
        want = G.mul_gen(_tail_scalar(s, *cfg))
        flat = [0] * (2 * G.d) if want is None else [v for coord in want for v in G.comp(coord)]
        assert [int(x, 16) for x in line.split()] == flat, (G, kind, cfg, line)
        infinities += want is None
        assert (want is None) == (kind in ("total_inf", "all_inf")) or kind == "opposite", (G, kind, cfg)
    assert infinities >= 4 * (len(configs) + 3)
    assert lines[-1] == "refused: internal: reduction layout does not fit the window", lines[-1]


def test_protocol_host_sides_refuse_bad_arguments_under_sanitizers(tmp_path):
    """the host side of csrc/ipa.hip and csrc/rangeproof.hip (argument rules, overlap checks, the conversion of the challenges,
    the shared pieces of fr_sum.hip.h and ipa_chain.hip.h) as two stand-alone programs under the address and undefined-behaviour
    sanitizers (tests/native/ipa_args_check.cpp, rangeproof_args_check.cpp, built by the recipe in their headers, which
    helpers.run_host_program carries out): a host-only compile, an EMPTY offload bundle for the __hip_fatbin_<hash> symbol the
    object refers to, link, run.  The sanitizer runtimes are linked into the programs.  A program sees no device on any machine, so the calls that pass the checks fail in the
    launch with ZK_ERR_HIP, which is what it expects."""
    from helpers import run_host_program
    for name in ("ipa_args_check", "rangeproof_args_check"):
        res = run_host_program(name, tmp_path)
        assert res.returncode == 0 and f"{name}: all ok" in res.stdout, res.stdout + res.stderr


def test_build_script_falls_back_to_plain_hipcc_when_the_pass_pipeline_cannot_be_reproduced(tmp_path):
    """csrc/hipcc_noreassoc.sh drives clang / opt / llc by hand to leave LLVM's `reassociate` pass out of the device pipeline; on a
    toolchain whose O3 pipeline text has no such pass it must not fail the build (round-3 advisor finding) but compile the unit
    with the stock driver, LLCFLAGS travelling as -mllvm options.  Fake tools stand in for the toolchain."""
    import stat
    import subprocess
    script = os.path.join(ROOT, "zksnake_amd", "csrc", "hipcc_noreassoc.sh")
    llvm = tmp_path / "llvm"
    llvm.mkdir()

    def tool(path, body):
        path.write_text("#!/bin/bash\n" + body)
        path.chmod(path.stat().st_mode | stat.S_IXUSR)

    tool(llvm / "clang++", 'while [ $# -gt 0 ]; do if [ "$1" = "-o" ]; then : > "$2"; fi; shift; done\n')
    tool(llvm / "opt", 'echo "module(function(instcombine,simplifycfg)),BitcodeWriterPass"; exit 1\n')   # no reassociate in this pipeline
    hipcc = tmp_path / "hipcc"
    tool(hipcc, f'echo "$@" > {tmp_path}/hipcc_args; while [ $# -gt 0 ]; do if [ "$1" = "-o" ]; then echo obj > "$2"; fi; shift; done\n')
    src = tmp_path / "unit.hip"
    src.write_text("// nothing\n")
    out = tmp_path / "unit.o"
    env = dict(os.environ, LLVM_BIN=str(llvm), HIPCC=str(hipcc), ARCH="gfx950", LLCFLAGS="-amdgpu-sched-strategy=max-ilp", TMPDIR=str(tmp_path))
    res = subprocess.run(["bash", script, str(out), str(src), "-O3", "-DZK_GROUP=Bn254G1"], env=env, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    assert "plain hipcc" in res.stderr
    args = (tmp_path / "hipcc_args").read_text()
    assert "--offload-arch=gfx950" in args and "-mllvm -amdgpu-sched-strategy=max-ilp" in args and "-DZK_GROUP=Bn254G1" in args
    assert out.read_text() == "obj\n"
