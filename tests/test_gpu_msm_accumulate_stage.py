"""The accumulate kernels on hand-built layouts: tests/native/accumulate_stage.hip launches the PRODUCTION accumulate_kernel,
accumulate_split_kernel and bases_to_mont_kernel (csrc/msm_accumulate.hip.h) through that header's launch_accumulate and
launch_bases_to_mont, the calls MsmPlan makes, on entry lists, bucket offsets and run offsets built here from (bucket sizes, seg_len), so that the alignments a scalar vector only meets by
luck are all there: buckets that end exactly on a segment boundary, buckets of seg_len, seg_len +- 1, 2 seg_len, 2 seg_len + 1
entries at offsets 0, 1 and seg_len - 1 inside a segment, more than 1500 empty keys before / between / after the non-empty ones,
one key, totals of 1, seg_len - 1, seg_len and k seg_len + 1 entries, one entry per bucket.  Every run's slot (the run_slot rule as
restated in msm_front_model.runs_of) is compared with the sum of its entries' known multiples of the generator, exactly, and with
the range promise of msm_front_model.check_row; rows no run owns must keep the sentinel they were filled with.  The harness checks
on the host that every index the kernel will form is inside its arrays and refuses (code 4) instead of launching; the refusals
have a test of their own, which needs the GPU machine too because the harness is a device build."""

import ctypes
import os
import random

import numpy as np
import pytest

import msm_front_model as FM
from reduce_model import GROUPS, Pool
from test_field_edges import ROOT

SRC = os.path.join(ROOT, "tests", "native", "accumulate_stage.hip")
pytestmark = pytest.mark.gpu
gid = lambda G: G.name  # noqa: E731
SENTINEL = 0xA5A5A5A5
BASE_KINDS = ("random", "all_equal", "alternating", "mostly_inf")


class Harness:
    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        lib.as_accumulate.restype = ci
        lib.as_accumulate.argtypes = [ci, ci, vp, u64, vp, u64, vp, vp, u32, u32, u32, vp, u64, vp]
        lib.as_bases_to_mont.restype = ci
        lib.as_bases_to_mont.argtypes = [ci, vp, u64, ci, vp]
        lib.as_constants.restype = None
        lib.as_constants.argtypes = [vp]
        c = np.zeros(2, dtype=np.uint32)
        lib.as_constants(c.ctypes.data)
        assert list(c) == [FM.COMBINE_SMALL_MAX, FM.COMBINE_WAVE_MAX]

    def accumulate(self, G, split, bases, sorted_words, bstart, sstart, seg_len, prio, n_partials, expect_rc=0):
        bases = np.ascontiguousarray(bases, dtype=np.uint32)
        sw = np.ascontiguousarray(sorted_words, dtype=np.uint32)
        bs, ss = np.ascontiguousarray(bstart, dtype=np.uint32), np.ascontiguousarray(sstart, dtype=np.uint32)
        n_keys = len(bs) - 1
        partials = np.full((n_partials, G.XW), SENTINEL, dtype=np.uint32)
        buckets = np.full((n_keys, G.XW), SENTINEL, dtype=np.uint32)
        rc = self.lib.as_accumulate(G.gid, int(split), bases.ctypes.data, bases.shape[0], sw.ctypes.data, len(sw), bs.ctypes.data, ss.ctypes.data,
                                    n_keys, seg_len, prio, partials.ctypes.data, n_partials, buckets.ctypes.data)
        assert rc == expect_rc, f"as_accumulate({G}) returned {rc}, expected {expect_rc}"
        return partials, buckets

    def bases_to_mont(self, G, canon, glv):
        canon = np.ascontiguousarray(canon, dtype=np.uint32)
        out = np.full(((2 if glv else 1) * canon.shape[0] + 1, canon.shape[1]), SENTINEL, dtype=np.uint32)
        rc = self.lib.as_bases_to_mont(G.gid, canon.ctypes.data, canon.shape[0], int(glv), out.ctypes.data)
        assert rc == 0, rc
        return out


def build_harness(d):
    """through the library's own pipeline, as build_stages of test_gpu_msm_reduce_stages.py; ZKMI_ACC_STAGE_LIB names an already
    built one"""
    from helpers import build_device_harness
    return build_device_harness(SRC, d, "ZKMI_ACC_STAGE_LIB")


@pytest.fixture(scope="module")
def harness(tmp_path_factory, gpu):
    return Harness(build_harness(tmp_path_factory.mktemp("as_dev")))


# ---- layouts --------------------------------------------------------------------------------------------------------------------------
def affine_rows(G, pool):
    """the pool's points as affine Montgomery rows (memory form); infinity as the all-zero row the bucket step skips"""
    rows = []
    for aff in pool.affine:
        if aff is None:
            rows.append([0] * (2 * G.LIMBS))
            continue
        words = []
        for coord in aff:
            for comp in G.to_mont(coord):
                words += [(comp >> (32 * i)) & 0xFFFFFFFF for i in range(G.f.W)]
        rows.append(words)
    return np.array(rows, dtype=np.uint32)


def aligned_sizes(S):
    """buckets of S - 1, S, S + 1, 2 S, 2 S + 1 entries starting at offsets 0, 1 and S - 1 inside a segment (a filler bucket before
    each moves the position there), so that buckets end exactly on, one before and one after a segment boundary"""
    sizes, pos = [], 0
    for off in (0, 1, S - 1):
        for size in (S - 1, S, S + 1, 2 * S, 2 * S + 1):
            fill = (off - pos) % S
            if fill:
                sizes.append(fill)
                pos += fill
            sizes.append(size)
            pos += size
    return sizes


def partition(total, parts, rnd):
    cuts = sorted(rnd.randrange(total + 1) for _ in range(parts - 1))
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


def layouts(S, rnd):
    k = 257 if S <= 64 else 5
    out = [("aligned", aligned_sizes(S)),
           ("empties", [0] * 1500 + [3] + [0] * 1600 + [S + 2] + [0] * 1500 + [1] + [0] * 1700),
           ("one_key", [5 * S + 3]),
           ("one_entry_per_bucket", [1] * (3 * 256 + 5))]
    for total in (1, S - 1, S, k * S + 1):
        out.append((f"total_{total}", partition(total, 7, rnd)))
    out.append((f"total_{k * S + 1}_one_bucket", [0, k * S + 1, 0]))
    return out


def run_layout(harness, G, pool, rows, sizes, S, signs, seed, split=False, prio=0):
    bstart = np.zeros(len(sizes) + 1, dtype=np.int64)
    bstart[1:] = np.cumsum(sizes)
    total = int(bstart[-1])
    sstart = FM.run_start(bstart, S)
    idx = pool.draw(total, seed)
    sign = {"none": np.zeros(total, dtype=np.int64), "all": np.ones(total, dtype=np.int64), "alternate": np.arange(total, dtype=np.int64) % 2}[signs]
    words = idx | (sign << 31)
    n_partials = int(sstart[-1]) + 3
    partials, buckets = harness.accumulate(G, split, rows, words, bstart, sstart, S, prio, n_partials)
    return bstart, sstart, idx, sign, partials, buckets


def check_layout(G, pool, S, bstart, sstart, idx, sign, partials, buckets, label):
    sc = np.array(pool.scalar, dtype=object)
    runs = FM.runs_of(bstart, sstart, S)
    logs = [int(sum(int(sc[i]) * (1 - 2 * int(s)) for i, s in zip(idx[a:b], sign[a:b]))) for _, _, _, a, b in runs]
    want = FM.oracle_multiples(G, logs)
    owned_p, owned_b = set(), set()
    for (key, kind, slot, a, b), aff in zip(runs, want):
        row = partials[slot] if kind == "partial" else buckets[slot]
        (owned_p if kind == "partial" else owned_b).add(slot)
        FM.check_row(G, row, aff, f"{label}: run of key {key} -> {kind}[{slot}], entries {a}..{b}")
    for slot in range(partials.shape[0]):
        if slot not in owned_p:
            # the slots of single-run buckets inside `partials` stay unused: run_start counts them, the run itself goes to `buckets`
            assert (partials[slot] == SENTINEL).all(), f"{G} {label}: partials[{slot}] belongs to no multi-run bucket and was written"
    for key in range(buckets.shape[0]):
        if key not in owned_b:
            assert (buckets[key] == SENTINEL).all(), f"{G} {label}: buckets[{key}] has no single run and was written"
    return len(runs)


@pytest.mark.parametrize("kind", BASE_KINDS)
@pytest.mark.parametrize("G", GROUPS, ids=gid)
def test_accumulate_layouts(harness, G, kind):
    """every layout at seg_len 8, 13, 64 and 1024 with the sign bit on no / every / every other entry; P = Q, P = -Q and infinity
    occur inside the segment walks through the base kinds; prio_steps 0 and 1 give the same words; the Fp2 groups run through both
    kernels with word-identical outputs"""
    pool = Pool(G, kind, 900 + 10 * G.gid + BASE_KINDS.index(kind))
    rows = affine_rows(G, pool)
    rnd = random.Random(901 + G.gid)
    checked = 0
    for S in (8, 13, 64, 1024):
        for li, (name, sizes) in enumerate(layouts(S, rnd)):
            signs = ("none", "all", "alternate")[(li + S) % 3]
            label = f"{kind} seg_len {S} layout {name} signs {signs}"
            res = run_layout(harness, G, pool, rows, sizes, S, signs, 7 * li + S)
            checked += check_layout(G, pool, S, *res, label)
            for split, prio in [(False, 1)] + ([(True, 0), (True, 1)] if G.d == 2 else []):
                other = run_layout(harness, G, pool, rows, sizes, S, signs, 7 * li + S, split=split, prio=prio)
                assert (other[4] == res[4]).all() and (other[5] == res[5]).all(), f"{G} {label}: split {split} prio_steps {prio} differs from the one-lane kernel without priority steps"
    assert checked > 1000


@pytest.mark.parametrize("G", GROUPS, ids=gid)
def test_harness_refuses_layouts_that_leave_the_arrays(harness, G):
    """the host-side walk: a reference past the base table, run offsets that are not the layout's run counts (a slot outside
    partials), non-monotone bucket offsets and a total that is not bucket_start[n_keys] are refused with code 4, nothing launched"""
    pool = Pool(G, "random", 950 + G.gid, size=8)
    rows = affine_rows(G, pool)
    S = 8
    bstart = np.array([0, 3, 3, 20, 21], dtype=np.int64)
    sstart = FM.run_start(bstart, S)
    words = np.arange(21, dtype=np.int64) % 8
    n_part = int(sstart[-1])
    harness.accumulate(G, False, rows, words, bstart, sstart, S, 0, n_part)
    bad_ref = words.copy()
    bad_ref[20] = 8 | (1 << 31)
    harness.accumulate(G, False, rows, bad_ref, bstart, sstart, S, 0, n_part, expect_rc=4)
    short = sstart.copy()
    short[-1] -= 1
    harness.accumulate(G, False, rows, words, bstart, short, S, 0, n_part, expect_rc=4)
    harness.accumulate(G, False, rows, words, bstart, sstart, S, 0, n_part - 1, expect_rc=4)
    harness.accumulate(G, False, rows, words, np.array([0, 3, 2, 20, 21]), sstart, S, 0, n_part, expect_rc=4)
    harness.accumulate(G, False, rows, words[:20], bstart, sstart, S, 0, n_part, expect_rc=4)
    harness.accumulate(G, G.d == 1, rows, words, bstart, sstart, S, 0, n_part, expect_rc=1 if G.d == 1 else 0)


@pytest.mark.parametrize("G", GROUPS, ids=gid)
def test_bases_to_mont(harness, G):
    """canonical affine rows -> Montgomery rows, plain and interleaved with phi(P) (G2: the NEG_Y convention), against pyref; sizes
    around the 128-lane workgroup; the row after the last one keeps its sentinel"""
    pool = Pool(G, "random", 960 + G.gid, size=130)
    rinv = pow(G.f.R, -1, G.p)
    W32 = G.f.W

    def canon(aff):
        out = []
        for coord in aff:
            for comp in G.comp(coord):
                out += [(comp >> (32 * i)) & 0xFFFFFFFF for i in range(W32)]
        return out

    def decode(ws):
        comps = [sum(int(ws[j * W32 + t]) << (32 * t) for t in range(W32)) for j in range(2 * G.d)]
        assert all(x < 2 * G.p for x in comps)     # the range the bucket step takes its base in
        plain = [x * rinv % G.p for x in comps]
        return (plain[0], plain[1]) if G.d == 1 else ((plain[0], plain[1]), (plain[2], plain[3]))

    for n in (1, 127, 128, 129, 130):
        pts = pool.affine[:n]
        arr = np.array([canon(a) for a in pts], dtype=np.uint32)
        for glv in (0, 1):
            out = harness.bases_to_mont(G, arr, glv)
            assert (out[-1] == SENTINEL).all()
            for i, P in enumerate(pts):
                if glv:
                    assert decode(out[2 * i]) == P and decode(out[2 * i + 1]) == FM.phi(G, P), (n, i)
                else:
                    assert decode(out[i]) == P, (n, i)
