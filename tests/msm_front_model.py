"""Integer model of the front half of the MSM pipeline (digits -> sort -> run offsets -> accumulate), for
tests/test_gpu_msm_front_stages.py and tests/test_gpu_msm_accumulate_stage.py.  numpy + Python integers, no GPU.

Definitions (B = 2^(c-1), r the scalar field's modulus, windows w = 0 .. nwin - 1):

  digits    bias = sum_w 2^(cw + c - 1);  u_w = ((s mod r) + bias) >> cw & (2^c - 1) is what the digit rows store, d_w = u_w - B the
            signed digit, sum_w d_w 2^(cw) = s mod r.  A split-scalar plan stores the digits of the two signed halves (k1, k2),
            s = k1 + lambda k2 (mod r), interleaved: entry 2i carries k1 of scalar i, entry 2i + 1 carries k2.
  entries   one per non-zero digit: key = set * B + |d| - 1, word = (d < 0) << 31 | ref.  `ref` is the row of the base table the
            accumulate kernel reads:
              general plan        ref = i            set = w - w_first          rows P_i
              split-scalar plan   ref = 2i, 2i + 1   set = w - w_first          rows P_i, phi(P_i)
              fixed-base plan     ref = (w - pw_first) n + i    set = 0 (ONE bucket set for all windows)    rows 2^(cw) P_i
            (scatter_kernel / scatter_range_kernel write `i` or `ref_base + i`; the two-level sort carries the same reference
            through level A and sort_lo_kernel strips the fine bucket bits off it again.)
  offsets   bucket_start = exclusive prefix of the key counts (n_keys + 1 words); the sorted list is cut into segments of seg_len
            entries, a run is the part of one bucket inside one segment: runs(key) = 1 + (s1 - 1) // seg_len - s0 // seg_len for a
            non-empty bucket [s0, s1); run_start = exclusive prefix of the run counts (n_keys + 1 words); buckets of more than
            COMBINE_SMALL_MAX runs are listed from the front of big_list, of more than COMBINE_WAVE_MAX from its back (any order).
  run slot  a bucket with ONE run is written to buckets[key]; otherwise the run of segment t goes to
            partials[run_start[key] + t - bucket_start[key] // seg_len].
  rows      what accumulate hands to combine_kernel / strided_sum_kernel (the input contract tabulated at the top of
            test_gpu_msm_reduce_stages.py): X < 4p, Y / ZZ / ZZZ < 2p per component, ZZ = 0 for infinity; the Fp2 groups bring X
            below 2p before the row leaves the registers (xyzz_relaxed_finish).

The checkers at the bottom raise AssertionError; test_gpu_msm_front_stages.py runs them on the buffers of a real run and the CPU
tests there run them on buffers built from this model with one thing broken at a time."""

import os
import re

import numpy as np

import reduce_model as RM
from oracle import pyref
from reduce_model import COMBINE_SMALL_MAX, COMBINE_WAVE_MAX, GROUPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROUTES = {0: "none", 1: "ranged", 2: "one-level", 3: "two-level-derive", 4: "two-level-scan", 5: "two-level-partial"}
VIEW_SLOTS = 29
VIEW_FIELDS = ("d_dig", "d_bases", "sorted", "bstart", "sstart", "big_list", "big_count", "partials", "buckets",
               "n", "n_api", "c", "nwin", "B", "glv", "pre", "wide", "pw_first", "pw_count", "w_first", "w_count", "groups", "seg_len",
               "m", "dstride", "route", "fine_log", "split_fine", "split_acc")
GLV_BITS = 128
SEG_TARGET_LANES = 256 * 1024


class View:
    """the slots of zk_msm_plan_debug_view (include/zkmi.h) by name"""

    def __init__(self, slots):
        assert len(slots) == VIEW_SLOTS == len(VIEW_FIELDS)
        for k, v in zip(VIEW_FIELDS, slots):
            setattr(self, k, int(v))
        self.n_keys = self.groups * self.B
        self.route_name = ROUTES[self.route]


# ---- windows ------------------------------------------------------------------------------------------------------------------
def window_count(bits, c):
    """windows of c bits that hold every value of `bits` bits plus the bias (two-bit windows need one more: msm_plan.h)"""
    return (bits + c - 1) // c + (1 if c == 2 else 0)


def glv_window_count(c):
    return window_count(GLV_BITS, c)


def bias_of(c, nwin):
    return sum(1 << (c * w + c - 1) for w in range(nwin))


def digits(scalars, r, c, nwin):
    """biased digits u_w of every scalar: list (per scalar) of nwin values in [0, 2^c)"""
    bias, mask = bias_of(c, nwin), (1 << c) - 1
    return [[((s % r + bias) >> (c * w)) & mask for w in range(nwin)] for s in scalars]


def signed_digits(scalars, r, c, nwin):
    B = 1 << (c - 1)
    return [[u - B for u in row] for row in digits(scalars, r, c, nwin)]


def biased_digit_rows(values, c, nwin, windows):
    """the same for many values at once: rows (len(windows), len(values)) of u_w for signed or unsigned `values` with
    |value| <= bias; bits [cw, cw + c) of value + bias, cut out of the little-endian bytes with numpy"""
    bias = bias_of(c, nwin)
    nbytes = (nwin * c + 7) // 8 + 9
    buf = b"".join((v + bias).to_bytes(nbytes, "little") for v in values)
    raw = np.frombuffer(buf, dtype=np.uint8).reshape(len(values), nbytes)
    out = np.zeros((len(windows), len(values)), dtype=np.int64)
    for k, w in enumerate(windows):
        byte, off = (c * w) // 8, (c * w) % 8
        word = np.zeros(len(values), dtype=np.uint64)
        for j in range(4):   # c + off <= 27 bits
            word |= raw[:, byte + j].astype(np.uint64) << np.uint64(8 * j)
        out[k] = ((word >> np.uint64(off)) & np.uint64((1 << c) - 1)).astype(np.int64)
    return out


# ---- the scalar split ------------------------------------------------------------------------------------------------------------
def _glv_table():
    """constants of csrc/glv_params.h (generated by tools/gen_glv_params.py), parsed: per group name lambda, beta, NEG_Y, the
    lattice vectors as signed integers and the two rounding multipliers"""
    with open(os.path.join(ROOT, "zksnake_amd", "csrc", "glv_params.h")) as fh:
        text = fh.read()
    out = {}
    for name, body in re.findall(r"struct (\w+)Glv \{(.*?)\n\};", text, re.S):
        lam = int(re.search(r"lambda = (0x[0-9a-f]+)", body).group(1), 16)
        neg_y = re.search(r"NEG_Y = (\w+);", body).group(1) == "true"
        lists = [[int(x.rstrip("u"), 16) for x in grp.split(",")] for grp in re.findall(r"\{((?:\s*0x[0-9a-f]+u,?)+)\}", body)]
        val = lambda ws: sum(w << (32 * i) for i, w in enumerate(ws))  # noqa: E731
        beta, g1, g2, a1, b1, a2, b2 = lists
        out[name] = dict(lam=lam, neg_y=neg_y, beta=val(beta), g1=val(g1), g2=val(g2))
        out[name]["a1"], out[name]["b1"] = _lattice_vector(val(a1), val(b1), lam, name)
        out[name]["a2"], out[name]["b2"] = _lattice_vector(val(a2), val(b2), lam, name)
    return out


_R_OF = {"Bn254": pyref.BN254.r, "Bn254G2": pyref.BN254.r, "Bls381": pyref.BLS12_381.r, "Bls381G2": pyref.BLS12_381.r}


def _lattice_vector(a, b, lam, name):
    """the header stores the vectors mod 2^128 (a component may need all 128 bits: BLS12-381's lambda is one): the signed reading
    is the one that lies in the lattice, a + b lambda = 0 (mod r)"""
    fits = [(x, y) for x in (a, a - (1 << 128)) for y in (b, b - (1 << 128)) if (x + y * lam) % _R_OF[name] == 0]
    assert len(fits) == 1, (name, fits)
    return fits[0]


_GLV_NAMES = {"BN254_G1": "Bn254", "BN254_G2": "Bn254G2", "BLS12_381_G1": "Bls381", "BLS12_381_G2": "Bls381G2"}
_GLV = None


def glv_consts(G):
    global _GLV
    if _GLV is None:
        _GLV = _glv_table()
    return _GLV[_GLV_NAMES[G.name]]


def glv_halves(s, cs):
    """(k1, k2), signed: (s, 0) minus the lattice point c1 v1 + c2 v2 nearest to it, c_i = (s g_i + 2^319) >> 320 (the rounded
    quotients of tools/gen_glv_params.py); s = k1 + lambda k2 (mod r) for ANY integers c1, c2, the rounding makes the halves short"""
    c1 = (s * cs["g1"] + (1 << 319)) >> 320
    c2 = (s * cs["g2"] + (1 << 319)) >> 320
    return s - c1 * cs["a1"] - c2 * cs["a2"], -c1 * cs["b1"] - c2 * cs["b2"]


def phi(G, P):
    """the endomorphism of the group on an affine pyref point: (beta x, y) on G1, (c x, -y) on G2"""
    if P is None:
        return None
    cs = glv_consts(G)
    F = G.g.F
    x = F.small(cs["beta"], P[0])
    return (x, F.neg(P[1]) if cs["neg_y"] else P[1])


# ---- a run of a plan ---------------------------------------------------------------------------------------------------------
def pick_seg_len(entries, B, pre, target=SEG_TARGET_LANES):
    """MsmPlan::pick_seg_len restated: ceil(entries / target lanes) held to [8, 64]; a fixed-base plan keeps a bucket within about
    12 runs (entries / B entries per bucket), up to 1024"""
    sl = min(64, max(8, -(-entries // target)))
    if pre:
        sl = min(1024, max(sl, (entries // B + 11) // 12))
    return sl


class Run:
    """the expected buffers of one run: scalars (ints, already mod-reduced or not) against a plan described by `v` (a View or any
    object with its scalar fields)"""

    def __init__(self, G, v, scalars):
        self.G, self.v = G, v
        c, B, r = v.c, v.B, G.r
        m_api = len(scalars)
        windows = list(range(v.w_first, v.w_first + v.w_count))
        red = [s % r for s in scalars]
        if v.glv:
            cs = glv_consts(G)
            halves = []
            for s in red:
                halves.extend(glv_halves(s, cs))
            self.u = biased_digit_rows(halves, c, v.nwin, windows)
        else:
            self.u = biased_digit_rows(red, c, v.nwin, windows)
        m = self.u.shape[1]
        assert m == (2 * m_api if v.glv else m_api)
        keys, words = [], []
        idx = np.arange(m, dtype=np.int64)
        for k, w in enumerate(windows):
            d = self.u[k] - B
            nz = d != 0
            key = (0 if v.pre else k) * B + np.abs(d[nz]) - 1
            ref = idx[nz] + ((w - v.pw_first) * v.n if v.pre else 0)
            assert ref.size == 0 or int(ref.max()) < 1 << 31
            keys.append(key)
            words.append(ref | ((d[nz] < 0).astype(np.int64) << 31))
        self.keys = np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64)
        self.words = np.concatenate(words) if words else np.zeros(0, dtype=np.int64)
        self.n_keys = (1 if v.pre else v.w_count) * B
        self.bstart = bucket_start(self.keys, self.n_keys)
        self.total = int(self.bstart[-1])

    def digit_rows(self):
        """the rows of d_dig the run wrote: (w_count, m), row k = window w_first + k (stored at row w_first - pw_first + k)"""
        return self.u

    def packed(self):
        """(keys << 32 | word) sorted: the multiset of entries per key"""
        return np.sort((self.keys.astype(np.uint64) << np.uint64(32)) | self.words.astype(np.uint64))


def bucket_start(keys, n_keys):
    out = np.zeros(n_keys + 1, dtype=np.int64)
    out[1:] = np.cumsum(np.bincount(keys, minlength=n_keys))
    return out


def run_counts(bstart, seg_len):
    bstart = np.asarray(bstart, dtype=np.int64)
    s0, s1 = bstart[:-1], bstart[1:]
    return np.where(s1 > s0, 1 + (s1 - 1) // seg_len - s0 // seg_len, 0)


def run_start(bstart, seg_len):
    out = np.zeros(len(bstart), dtype=np.int64)
    out[1:] = np.cumsum(run_counts(bstart, seg_len))
    return out


def tiers(runs):
    """(wave-tier keys, workgroup-tier keys) as sorted arrays, by reduce_model.tier_of's rule"""
    runs = np.asarray(runs)
    wave = np.nonzero((runs > COMBINE_SMALL_MAX) & (runs <= COMBINE_WAVE_MAX))[0]
    big = np.nonzero(runs > COMBINE_WAVE_MAX)[0]
    assert all(RM.tier_of(int(runs[k])) == "wave" for k in wave[:4]) and all(RM.tier_of(int(runs[k])) == "big" for k in big[:4])
    return wave, big


def runs_of(bstart, sstart, seg_len, keys=None):
    """(key, slot kind, slot index, first entry, end entry) of every run of `keys` (default: all non-empty keys): kind "bucket" for
    the single run of a bucket (slot = key), "partial" otherwise"""
    out = []
    bstart = np.asarray(bstart, dtype=np.int64)
    sstart = np.asarray(sstart, dtype=np.int64)
    if keys is None:
        keys = np.nonzero(bstart[1:] > bstart[:-1])[0]
    for key in keys:
        key = int(key)
        s0, s1 = int(bstart[key]), int(bstart[key + 1])
        if s1 == s0:
            continue
        t0, t1 = s0 // seg_len, (s1 - 1) // seg_len
        if t1 == t0:
            out.append((key, "bucket", key, s0, s1))
            continue
        for t in range(t0, t1 + 1):
            out.append((key, "partial", int(sstart[key]) + t - t0, max(s0, t * seg_len), min(s1, (t + 1) * seg_len)))
    return out


# ---- logarithms -----------------------------------------------------------------------------------------------------------------
class Logs:
    """bases k_i G with small known k_i (below 2^31, so that int64 sums over a bucket cannot overflow): the logarithm of a table
    row is k_i times a weight that depends only on the row's class -- 1, lambda (odd rows of a split-scalar plan) or 2^(c w)
    (window w of a fixed-base table) -- so the logarithm of any signed sum of rows is sum_class weight * (int64 sum of +-k)"""

    def __init__(self, G, v, ks):
        self.G, self.v = G, v
        self.ks = np.asarray(ks, dtype=np.int64)
        assert self.ks.size == v.n_api and int(self.ks.max()) < 1 << 31
        if v.glv:
            self.weights = [1, glv_consts(G)["lam"]]
        elif v.pre:
            self.weights = [pow(2, v.c * (v.pw_first + k), G.r) for k in range(v.pw_count)]
        else:
            self.weights = [1]

    def row_log(self, ref):
        v = self.v
        if v.glv:
            return int(self.ks[ref // 2]) * self.weights[ref % 2] % self.G.r
        if v.pre:
            return int(self.ks[ref % v.n]) * self.weights[ref // v.n] % self.G.r
        return int(self.ks[ref])

    def sum_log(self, words):
        """logarithm of sum +-row(ref) over the entry words"""
        v = self.v
        words = np.asarray(words, dtype=np.int64)
        ref = words & 0x7FFFFFFF
        sign = 1 - 2 * (words >> 31)
        if v.glv:
            cls, k = ref & 1, self.ks[ref >> 1]
        elif v.pre:
            cls, k = ref // v.n, self.ks[ref % v.n]
        else:
            cls, k = np.zeros_like(ref), self.ks[ref]
        sums = np.zeros(len(self.weights), dtype=np.int64)
        np.add.at(sums, cls, sign * k)
        return sum(int(s) * w for s, w in zip(sums, self.weights)) % self.G.r


def oracle_multiples(G, logs, threads=8):
    """[log] G as pyref affine points (None = infinity) from the CPU oracle's threaded batch multiplication"""
    from oracle import corc
    cid = 0 if G.name.startswith("BN254") else 1
    if not logs:
        return []
    gen = corc.points_to_limbs([G.g.gen], cid, G.which)[0]
    out = corc.batch_mul(cid, G.which, corc.ints_to_limbs([x % G.r for x in logs], 4), gen, threads=threads)
    return corc.limbs_to_points(out, cid, G.which)


# ---- checkers ---------------------------------------------------------------------------------------------------------------------
def check_digits(got_rows, run):
    want = run.digit_rows()
    got = np.asarray(got_rows).astype(np.int64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} digits differ, first at (window row, entry) {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def check_bstart(got, run):
    got = np.asarray(got).astype(np.int64)
    assert got.shape == run.bstart.shape
    assert int(got[-1]) == run.total == len(run.keys), f"bstart[n_keys] = {int(got[-1])}, non-zero digits: {run.total}"
    bad = np.nonzero(got != run.bstart)[0]
    assert bad.size == 0, f"bstart differs at {len(bad)} keys, first key {int(bad[0])}: got {int(got[bad[0]])}, want {int(run.bstart[bad[0]])}"


def check_sorted(got_sorted, got_bstart, run):
    """per key the multiset of entry words, through one sort of (key, word) on each side; keys of the GPU side from ITS offsets"""
    got_bstart = np.asarray(got_bstart).astype(np.int64)
    got_sorted = np.asarray(got_sorted).astype(np.uint64)
    counts = np.diff(got_bstart)
    assert (counts >= 0).all() and int(got_bstart[0]) == 0 and int(got_bstart[-1]) == got_sorted.size == run.total
    keys = np.repeat(np.arange(len(counts), dtype=np.uint64), counts)
    packed = np.sort((keys << np.uint64(32)) | got_sorted)
    want = run.packed()
    bad = np.nonzero(packed != want)[0]
    assert bad.size == 0, (f"{len(bad)} sorted entries differ, first: got key {int(packed[bad[0]]) >> 32} word {int(packed[bad[0]]) & 0xFFFFFFFF:#x}, "
                           f"want key {int(want[bad[0]]) >> 32} word {int(want[bad[0]]) & 0xFFFFFFFF:#x}")


def check_sstart(got, bstart, seg_len):
    got = np.asarray(got).astype(np.int64)
    want = run_start(bstart, seg_len)
    assert got.shape == want.shape
    assert int(got[-1]) == int(want[-1]), f"sstart[n_keys] = {int(got[-1])}, runs: {int(want[-1])}"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"sstart differs at {len(bad)} keys, first key {int(bad[0])}: got {int(got[bad[0]])}, want {int(want[bad[0]])}"


def check_big(big_list, big_count, bstart, seg_len):
    n_keys = len(bstart) - 1
    wave, big = tiers(run_counts(bstart, seg_len))
    bc = [int(x) for x in np.asarray(big_count)[:2]]
    assert bc == [len(wave), len(big)], f"big_count {bc}, model {[len(wave), len(big)]}"
    bl = np.asarray(big_list).astype(np.int64)
    assert sorted(bl[:bc[0]]) == list(wave), "front of big_list (17 .. 2048 runs) is not the model's set"
    assert sorted(bl[n_keys - bc[1]:n_keys]) == list(big), "back of big_list (more than 2048 runs) is not the model's set"
    return wave, big


def check_row(G, words, want, what="", finished=True):
    """a row accumulate or combine left behind: the range promise to the reduction stages, ZZ = 0 <=> ZZZ = 0, infinity as ZZ = 0,
    and the affine point.  finished: the row was written by an accumulate kernel, which for the Fp2 groups brings X below 2p
    (xyzz_relaxed_finish); a bucket combine_kernel wrote keeps pair_add's X < 4p"""
    pt = G.unrow(words)
    try:
        G.check_row_range(pt)
        if G.d == 2 and finished:
            assert all(x < 2 * G.p for x in pt[0]), "Fp2 groups finish X below 2p"
        assert G.is_zero(pt[2]) == G.is_zero(pt[3]), "ZZ = 0 <=> ZZZ = 0"
        if G.is_inf(pt):
            assert all(x == 0 for x in pt[2]), "infinity is stored as ZZ = 0 (not p)"
        got = G.to_affine(pt)
        assert got == want, f"point differs: got {got}, want {want}"
    except AssertionError as e:
        raise AssertionError(f"{G} {what}: {e}") from None


def check_empty_bucket(G, words, what=""):
    assert not np.asarray(words).any(), f"{G} {what}: an empty bucket must be all-zero words after combine"
