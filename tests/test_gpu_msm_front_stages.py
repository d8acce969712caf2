"""The front half of the MSM pipeline stage by stage: digits -> sort (+ offset scans) -> accumulate (-> combine), every buffer a
real zk_msm_plan_run leaves behind (zk_msm_plan_debug_view + zk_dev_download) against the integer model of tests/msm_front_model.py.
No tolerance anywhere: digits, offsets and entry words are compared as integers, rows as affine points plus their range promise.

  buffer        producer                                   contract checked here
  d_dig         digits_kernel / glv_digits_kernel          u_w = ((s mod r) + bias) >> cw & (2^c - 1); split scalars interleaved
  d_bases       bases_to_mont_kernel, precompute_table     P_i / (P_i, phi P_i) / 2^(cw) P_i in Montgomery form, < 2p
  bstart        the sort route of the case                 exclusive prefix of the key counts, bstart[n_keys] = non-zero digits
  sorted        the sort route of the case                 per key the multiset of sign << 31 | ref
  sstart        runs_offsets_kernel / runs_scan_block+scan  exclusive prefix of the run counts INCLUDING sstart[n_keys]
  big_list/count  the same kernels                         the two tiers as sets
  partials      accumulate_kernel / accumulate_split       every run of a multi-run bucket = sum of its entries' rows, in range
  buckets       accumulate (one run), combine (the rest)   bucket sum, in range; empty bucket = zero words

Below 2^14 entries every row is checked; above, a sample whose classes (tier buckets, first and last key of every set, buckets
on the first 4096 segment boundaries, 2048 drawn buckets) are counted one by one and whose run rows are counted against the model's
run counts.  Inputs: the bases k_i G come from the CPU oracle up to 2^13 points and from the library's zk_batch_mul above (64 rows
held against the oracle) -- the one place where library GPU code feeds the model side; every expected value comes from the oracle.
The module ends with an assertion over the sort routes the passing cases reported, for 16- and 32-bit digits.  The CPU tests (no gpu
marker) hold the model against its definitions and show that every checker raises on a single corrupted word."""

import random

import numpy as np
import pytest

import msm_front_model as FM
import reduce_model as RM
from msm_front_model import Logs, Run, View
from oracle import corc, pyref
from reduce_model import GROUPS
from zksnake_amd import _native as N
from zksnake_amd import workloads as W

gid = lambda G: G.name  # noqa: E731
BN_G1 = GROUPS[0]
FULL_CHECK_BELOW = 1 << 14
SAMPLE_DRAWN = 2048
SAMPLE_SEGMENTS = 4096
RUNS_PER_BUCKET_MAX = 4096


def ids_of(G):
    return (0 if G.name.startswith("BN254") else 1), G.which


# ---- CPU: the model against its definitions ----------------------------------------------------------------------------------------
def _edge_scalars(r, c, nwin):
    vals = [0, 1, r - 1, r, (1 << 256) - 1, (1 << 255) - 1, r + 1, 2 * r - 1]
    for w in range(nwin):
        for s in ((1 << (c * w)) - 1, 1 << (c * w), (1 << (c * w)) + 1, 1 << (c * w + c - 1), (1 << (c * w + c - 1)) - 1, (1 << (c * w + c - 1)) + 1):
            if s < 1 << 256:
                vals.append(s)
    return vals


@pytest.mark.parametrize("curve", [pyref.BN254, pyref.BLS12_381], ids=lambda cv: cv.name)
def test_model_digits_recompose(curve):
    """sum_w (u_w - 2^(c-1)) 2^(cw) == s mod r for every c in 2 .. 20 on edge scalars, every digit in range, the byte-slicing form
    of the model equal to the shift-and-mask definition; and the scalars 2^(cw + c - 1) put -2^(c-1) into window w (the last key)"""
    r = curve.r
    for c in range(2, 21):
        nwin = FM.window_count(r.bit_length() + 1, c)
        vals = _edge_scalars(r, c, nwin)
        sd = FM.signed_digits(vals, r, c, nwin)
        B = 1 << (c - 1)
        for s, row in zip(vals, sd):
            assert sum(d << (c * w) if d >= 0 else -((-d) << (c * w)) for w, d in enumerate(row)) == s % r, (c, hex(s))
            assert all(-B <= d < B for d in row)
        fast = FM.biased_digit_rows([s % r for s in vals], c, nwin, list(range(nwin)))
        assert (fast.T == np.array(FM.digits(vals, r, c, nwin), dtype=np.int64)).all(), c
        for w in range(nwin - 1):
            s = 1 << (c * w + c - 1)
            if s < r:
                assert FM.signed_digits([s], r, c, nwin)[0][w] == -B


@pytest.mark.parametrize("G", GROUPS, ids=gid)
def test_model_split_halves(G):
    """k1 + lambda k2 = s (mod r) on the corner scalars of test_split_scalar_plan_on_the_decomposition_corner_cases, both halves
    inside what the window count assumes: |k| <= bias (digits never underflow) and k + bias < 2^(nwin c) for every c in 2 .. 16;
    lambda acts as phi on the generator"""
    cs = FM.glv_consts(G)
    r, lam = G.r, cs["lam"]
    assert FM.phi(G, G.g.gen) == G.g.mul(G.g.gen, lam)
    vals = [0, 1, 2, r - 1, r - 2, r // 2, r // 2 + 1, lam, lam + 1, lam - 1, r - lam, r - lam + 1, (r - 1) // 3, 2 * (r - 1) // 3,
            lam * lam % r, (lam * lam + 1) % r, cs["a1"] % r, (-cs["b1"]) % r, cs["a2"] % r, cs["b2"] % r]
    vals += [(1 << b) % r for b in range(0, 256, 7)] + [(r - (1 << b)) % r for b in range(0, 254, 9)]
    rnd = random.Random(3 + G.gid)
    vals += [rnd.randrange(r) for _ in range(300)]
    for s in vals:
        k1, k2 = FM.glv_halves(s, cs)
        assert (k1 + lam * k2 - s) % r == 0
        for k in (k1, k2):
            assert abs(k) < 1 << 127
            for c in range(2, 17):
                nwin = FM.glv_window_count(c)
                bias = FM.bias_of(c, nwin)
                assert 0 <= k + bias < 1 << (nwin * c), (c, hex(s))


class _Plan:
    """the scalar fields of a view for a model-only run"""

    def __init__(self, G, n_api, c, glv=False, pre=False, pw_first=0, pw_count=0, w_first=None, w_count=None):
        self.c, self.B, self.glv, self.pre, self.n_api = c, 1 << (c - 1), int(glv), int(pre), n_api
        self.n = 2 * n_api if glv else n_api
        self.nwin = FM.glv_window_count(c) if glv else FM.window_count(G.r.bit_length() + 1, c)
        self.pw_first, self.pw_count = pw_first, pw_count or self.nwin
        self.w_first = self.pw_first if w_first is None else w_first
        self.w_count = self.pw_count if w_count is None else w_count
        self.groups = 1 if pre else self.w_count
        self.n_keys = self.groups * self.B


@pytest.mark.parametrize("mode", ("general", "split", "fixed"))
@pytest.mark.parametrize("G", GROUPS, ids=gid)
def test_model_entries_sum_to_the_msm(G, mode):
    """the entry list of the model, summed with pyref (buckets by point additions, sum_b (b + 1) bucket_b, 2^(c w) per bucket set),
    equals the pyref MSM: the key / reference / sign rules of the three plan kinds, including phi rows and table rows"""
    n, c = 10, 5
    rnd = random.Random(11 + G.gid)
    g = G.g
    pts = [aff for aff, _ in RM.real_points(G, n, 21 + G.gid)]
    scalars = [rnd.randrange(G.r) for _ in range(n - 3)] + [0, G.r - 1, 1 << (c * 3 + c - 1)]
    v = _Plan(G, n, c, glv=mode == "split", pre=mode == "fixed")
    run = Run(G, v, scalars)
    if mode == "split":
        rows = [q for P in pts for q in (P, FM.phi(G, P))]
    elif mode == "fixed":
        rows, cur = [], pts
        for _ in range(v.nwin):
            rows += cur
            cur = [g.mul(P, 1 << c) for P in cur]
    else:
        rows = pts
    buckets = [None] * run.n_keys
    for key, word in zip(run.keys, run.words):
        P = rows[int(word) & 0x7FFFFFFF]
        buckets[int(key)] = g.add(buckets[int(key)], g.neg(P) if int(word) >> 31 else P)
    total = None
    for s in range(run.n_keys // v.B):
        acc = None
        for b in range(v.B):
            acc = g.add(acc, g.mul(buckets[s * v.B + b], b + 1) if buckets[s * v.B + b] is not None else None)
        total = g.add(total, acc if mode == "fixed" else (g.mul(acc, pow(2, c * s, G.r)) if acc is not None else None))
    assert total == g.msm(pts, scalars)
    assert int(run.bstart[-1]) == sum(1 for row in run.u for u in row if u != v.B)


def test_model_run_offsets_and_seg_len():
    bstart = np.array([0, 0, 5, 8, 8, 16, 17, 40, 40])
    assert list(FM.run_counts(bstart, 8)) == [0, 1, 1, 0, 1, 1, 3, 0]
    assert list(FM.run_start(bstart, 8)) == [0, 0, 1, 2, 2, 3, 4, 7, 7]
    runs = FM.runs_of(bstart, FM.run_start(bstart, 8), 8)
    assert runs == [(1, "bucket", 1, 0, 5), (2, "bucket", 2, 5, 8), (4, "bucket", 4, 8, 16), (5, "bucket", 5, 16, 17),
                    (6, "partial", 4, 17, 24), (6, "partial", 5, 24, 32), (6, "partial", 6, 32, 40)]
    assert FM.pick_seg_len(1000 * 16, 1 << 15, False) == 8 and FM.pick_seg_len(1 << 24, 1 << 15, False) == 64
    assert FM.pick_seg_len((1 << 20) + 1, 1 << 15, False, target=64) == 64 and FM.pick_seg_len(3 * 262144 + 1, 1 << 15, False) == 8
    assert FM.pick_seg_len(10 * 262144 + 1, 1 << 15, False) == 11
    assert FM.pick_seg_len(13 << 20, 1 << 19, True) == 52 and FM.pick_seg_len(26 * 4096, 512, True) == 18


# ---- one set of buffers, every check ---------------------------------------------------------------------------------------------------
def check_front_buffers(G, v, run, logs, buf, full_below=FULL_CHECK_BELOW, seed=1):
    """items 1-4 and 6 of the stage checks on host copies of the buffers: buf = dict(dig, bstart, sorted, sstart, big_list, big_count,
    partials, buckets).  Returns the number of run rows and bucket rows checked."""
    seg_len = v.seg_len
    FM.check_digits(buf["dig"], run)
    FM.check_bstart(buf["bstart"], run)
    FM.check_sorted(buf["sorted"], buf["bstart"], run)
    FM.check_sstart(buf["sstart"], run.bstart, seg_len)
    wave, big = FM.check_big(buf["big_list"], buf["big_count"], run.bstart, seg_len)
    bstart, sstart = run.bstart, FM.run_start(run.bstart, seg_len)
    nonempty = np.nonzero(bstart[1:] > bstart[:-1])[0]
    counts = FM.run_counts(bstart, seg_len)
    if run.total < full_below:
        keys = nonempty
        runs = FM.runs_of(bstart, sstart, seg_len, keys)
        assert len(runs) == int(counts.sum()), "below the threshold every run is checked"
    else:
        # the classes of the sample, each counted against a figure that does not come from the sets themselves
        tier = set(int(k) for k in wave) | set(int(k) for k in big)
        assert len(tier) == int((counts > FM.COMBINE_SMALL_MAX).sum())
        ends, sets_with_entries = set(), 0
        for s in range(run.n_keys // v.B):
            ks = nonempty[(nonempty >= s * v.B) & (nonempty < (s + 1) * v.B)]
            if ks.size:
                sets_with_entries += 1
                ends.update((int(ks[0]), int(ks[-1])))
        assert sets_with_entries == int((np.diff(bstart[::v.B]) > 0).sum()) and sets_with_entries <= len(ends) <= 2 * sets_with_entries
        # every run that starts or ends on a segment boundary among the first SAMPLE_SEGMENTS segments: the buckets of the entries
        # on either side of the boundaries
        n_edges = min(SAMPLE_SEGMENTS, (run.total - 1) // seg_len)
        edges = np.arange(1, n_edges + 1, dtype=np.int64) * seg_len
        boundary = set()
        for pos in (edges - 1, edges):
            boundary.update(int(k) for k in np.searchsorted(bstart, pos, side="right") - 1)
        assert n_edges == 0 or len(boundary) >= 1
        for e in (edges[:1], edges[-1:]):     # both neighbours of the first and of the last boundary are inside sampled buckets
            for pos in (e - 1, e):
                assert all(any(bstart[k] <= q < bstart[k + 1] for k in boundary) for q in pos)
        n_drawn = min(SAMPLE_DRAWN, nonempty.size)
        drawn = set(int(k) for k in np.random.default_rng(seed).choice(nonempty, size=n_drawn, replace=False))
        assert len(drawn) == n_drawn
        keys = np.array(sorted(tier | ends | boundary | drawn), dtype=np.int64)
        assert max(len(tier), len(ends), len(boundary), n_drawn) <= len(keys) <= len(tier) + len(ends) + len(boundary) + n_drawn
        # a bucket of more than RUNS_PER_BUCKET_MAX runs (all scalars equal on 2^20 entries) is sampled itself: its first and last 64
        # runs and 512 drawn; the number of run rows checked is held against the model's run counts of the sampled buckets
        rnd = random.Random(seed)
        runs = []
        for key in keys:
            lst = FM.runs_of(bstart, sstart, seg_len, [key])
            runs += lst if len(lst) <= RUNS_PER_BUCKET_MAX else lst[:64] + lst[-64:] + rnd.sample(lst[64:-64], 512)
        want_rows = int(np.minimum(counts[keys], np.where(counts[keys] > RUNS_PER_BUCKET_MAX, 640, RUNS_PER_BUCKET_MAX)).sum())
        assert len(runs) == want_rows >= n_drawn, (len(runs), want_rows, n_drawn)
    sorted_gpu = np.asarray(buf["sorted"]).astype(np.int64)
    want_runs = FM.oracle_multiples(G, [logs.sum_log(sorted_gpu[a:b]) for _, _, _, a, b in runs])
    for (key, kind, slot, a, b), want in zip(runs, want_runs):
        if kind == "partial":
            FM.check_row(G, buf["partials"][slot], want, f"run of key {key} in partials[{slot}] (entries {a}..{b}, seg_len {seg_len})")
    want_buckets = FM.oracle_multiples(G, [logs.sum_log(sorted_gpu[int(bstart[k]):int(bstart[k + 1])]) for k in keys])
    for key, want in zip(keys, want_buckets):
        single = int(sstart[key + 1] - sstart[key]) == 1     # accumulate wrote the row itself; otherwise combine_kernel did
        FM.check_row(G, buf["buckets"][int(key)], want, f"bucket {int(key)} ({int(bstart[key + 1] - bstart[key])} entries, seg_len {seg_len})", finished=single)
    empties = np.nonzero(bstart[1:] == bstart[:-1])[0]
    if run.total < full_below:
        bad = [int(k) for k in empties if np.asarray(buf["buckets"][int(k)]).any()]
        assert not bad, f"{G}: empty buckets with non-zero words after combine: {bad[:8]}"
    else:
        for k in list(empties[:64]) + list(empties[-64:]):
            FM.check_empty_bucket(G, buf["buckets"][int(k)], f"bucket {int(k)}")
    return len(runs), len(keys)


def model_buffers(G, v, run, logs, rnd):
    """a consistent set of buffers from the model alone (what a correct run would leave behind, in one of its valid orders)"""
    order = np.lexsort((run.words, run.keys))
    sorted_words = run.words[order]
    sstart = FM.run_start(run.bstart, v.seg_len)
    wave, big = FM.tiers(FM.run_counts(run.bstart, v.seg_len))
    big_list = np.zeros(run.n_keys, dtype=np.int64)
    big_list[:len(wave)] = wave[::-1]
    big_list[run.n_keys - len(big):] = big
    runs = FM.runs_of(run.bstart, sstart, v.seg_len)
    partials = np.zeros((int(sstart[-1]), G.XW), dtype=np.uint32)
    buckets = np.zeros((run.n_keys, G.XW), dtype=np.uint32)

    def row(aff):
        pt = G.xyzz(aff, rnd)
        if G.d == 2:
            pt = (tuple(x % (2 * G.p) for x in pt[0]),) + pt[1:]
        return G.row(pt)

    pts = FM.oracle_multiples(G, [logs.sum_log(sorted_words[a:b]) for _, _, _, a, b in runs])
    for (key, kind, slot, a, b), aff in zip(runs, pts):
        if kind == "partial":
            partials[slot] = row(aff)
    keys = np.nonzero(run.bstart[1:] > run.bstart[:-1])[0]
    for key, aff in zip(keys, FM.oracle_multiples(G, [logs.sum_log(sorted_words[int(run.bstart[k]):int(run.bstart[k + 1])]) for k in keys])):
        buckets[int(key)] = row(aff)
    return dict(dig=run.digit_rows().copy(), bstart=run.bstart.copy(), sorted=sorted_words.copy(), sstart=sstart, big_list=big_list,
                big_count=np.array([len(wave), len(big)]), partials=partials, buckets=buckets)


@pytest.mark.parametrize("G", [GROUPS[0], GROUPS[3]], ids=gid)
def test_checkers_bite(G):
    """a consistent set of buffers built from the model passes; with ONE thing broken every time a check raises: sstart[n_keys] off
    by one, an entry moved to the neighbouring key, a flipped sign bit, a key missing from the front of big_list, a run's row out of
    range (X + 2p) and negated, bstart flat where the model has entries, a wrong digit, a non-zero word in an empty bucket"""
    n, c = 300, 4
    rnd = random.Random(77 + G.gid)
    v = _Plan(G, n, c)
    v.seg_len = 8
    scalars = [rnd.randrange(G.r) for _ in range(n)]
    scalars[:200] = [scalars[0]] * 200     # buckets of more than 16 runs: the front of big_list is not empty
    ks = [rnd.randrange(1, 1 << 31) for _ in range(n)]
    run, logs = Run(G, v, scalars), Logs(G, v, ks)
    good = model_buffers(G, v, run, logs, rnd)
    n_runs, n_buckets = check_front_buffers(G, v, run, logs, good)
    assert n_runs > 100 and n_buckets > 100
    for full_below in (0, 1 << 30):     # the sampling path and the every-row path on the same buffers
        assert check_front_buffers(G, v, run, logs, good, full_below=full_below)[0] >= 100
    wave, _ = FM.tiers(FM.run_counts(run.bstart, 8))
    assert len(wave) >= 1, "the case must list a bucket"
    p = G.p

    def broken(name):
        b = {k: np.array(x, copy=True) for k, x in good.items()}
        multi = next(r for r in FM.runs_of(run.bstart, good["sstart"], 8) if r[1] == "partial")
        cnt = np.diff(run.bstart)
        key_full = next(k for k in range(run.n_keys - 1) if cnt[k] >= 2 and cnt[k + 1] >= 1 and k % v.B != v.B - 1)
        if name == "sstart_last":
            b["sstart"][-1] += 1
        elif name == "entry_moved":
            e = int(run.bstart[key_full + 1])    # the last entry of the key and the first of its neighbour change places
            assert b["sorted"][e - 1] != b["sorted"][e]
            b["sorted"][e - 1], b["sorted"][e] = b["sorted"][e], b["sorted"][e - 1]
        elif name == "sign_flipped":
            b["sorted"][int(run.bstart[key_full])] ^= 1 << 31
        elif name == "big_list_front":
            b["big_list"][0] = b["big_list"][1] if len(wave) > 1 else (int(wave[0]) + 1) % run.n_keys
        elif name in ("row_out_of_range", "row_negated"):
            pt = G.unrow(b["partials"][multi[2]])
            if name == "row_negated":
                pt = G.neg_pt(pt)
            else:
                lift = 2 * p if G.d == 2 else 4 * p
                pt = (tuple(x % p + lift for x in pt[0]),) + pt[1:]
                assert G.to_affine(pt) == G.to_affine(G.unrow(b["partials"][multi[2]]))
            b["partials"][multi[2]] = G.row(pt)
        elif name == "bstart_flat":
            b["bstart"][key_full + 1:] = b["bstart"][key_full]
        elif name == "digit":
            b["dig"][1, 5] ^= 1
        elif name == "empty_bucket":
            empty = int(np.nonzero(np.diff(run.bstart) == 0)[0][0]) if (np.diff(run.bstart) == 0).any() else None
            assert empty is not None
            b["buckets"][empty][3] = 1
        return b

    # what the intended checker says for each corruption
    expect = {"sstart_last": r"sstart\[n_keys\]", "entry_moved": "sorted entries differ", "sign_flipped": "sorted entries differ",
              "big_list_front": "front of big_list", "row_out_of_range": r"partials\[\d+\]", "row_negated": "point differs",
              "bstart_flat": r"bstart\[n_keys\]", "digit": "digits differ", "empty_bucket": "empty bucket"}
    for name, message in expect.items():
        bad = broken(name)     # built outside the block: a failing set-up assertion must not count as a catch
        for full_below in (0, 1 << 30):
            with pytest.raises(AssertionError, match=message):
                check_front_buffers(G, v, run, logs, bad, full_below=full_below)


# ---- GPU: a real run, buffer by buffer ------------------------------------------------------------------------------------------------------
SEEN_ROUTES = set()   # (route name, wide) of every case that passed


def _download(gpu, ptr, count, dtype):
    out = np.zeros(count, dtype=dtype)
    if count:
        N.check(gpu.zk_dev_download(out.ctypes.data, ptr, out.nbytes))
    return out


def _view(gpu, h):
    slots = np.zeros(FM.VIEW_SLOTS, dtype=np.uint64)
    N.check(gpu.zk_msm_plan_debug_view(h, N.u64p(slots), FM.VIEW_SLOTS))
    return View(slots)


def small_logs(n, seed):
    return (W.splitmix64(seed, n) % np.uint64((1 << 31) - 1) + np.uint64(1)).astype(np.int64)


def make_bases(gpu, G, ks):
    """k_i G: from the CPU oracle up to 2^13 points; above, from the library's batch multiplication with 64 rows held against the
    oracle (a wrong base would also make every run row that contains it differ from its oracle value)"""
    cid, grp = ids_of(G)
    n = len(ks)
    kl = np.zeros((n, 4), dtype=np.uint64)
    kl[:, 0] = ks.astype(np.uint64)
    gen = corc.points_to_limbs([G.g.gen], cid, grp)[0]
    if n <= 1 << 13:
        return corc.batch_mul(cid, grp, kl, gen)
    bases = np.zeros((n, N.point_limbs(cid, grp)), dtype=np.uint64)
    N.check(gpu.zk_batch_mul(cid, grp, n, N.u64p(kl), N.u64p(gen), 1, N.u64p(bases)))
    pick = np.random.default_rng(n).choice(n, size=64, replace=False)
    assert (bases[pick] == corc.batch_mul(cid, grp, kl[pick], gen)).all()
    return bases


def mixed_scalars(G, v_like, n, seed, top_bits=125):
    """mostly uniform; every 16th zero, every 16th (offset 1) a 40-bit value, and from index 2 on the scalars 2^(cw + c - 1) whose
    digit in window w is -2^(c-1): the LAST key of that window's bucket set (and +1, the first key, in the window above)"""
    _, ints = W.field_stream(seed, n, G.r)
    for i in range(0, n, 16):
        ints[i] = 0
    for i in range(1, n, 16):
        ints[i] &= (1 << 40) - 1
    c, nwin = v_like
    # below 2^125 such a scalar is its own first half under the split (second half zero)
    tops = [1 << (c * w + c - 1) for w in range(nwin) if (1 << (c * w + c - 1)) < min(G.r, 1 << top_bits)]
    for j, s in enumerate(tops):
        if 2 + 16 * j < n:
            ints[2 + 16 * j] = s
    return ints


def skewed_scalars(G, n, seed):
    """half of the scalars equal (per window one bucket with half of all entries: the workgroup tier, more than 2048 runs), 2000
    more equal to a second value (17 .. 2048 runs: the wave tier), the rest uniform"""
    _, ints = W.field_stream(seed, n, G.r)
    ints[:n // 2] = [(G.r - 1) // 3] * (n // 2)
    ints[n // 2:n // 2 + 2000] = [(G.r - 1) // 5] * 2000
    return ints


def model_tiers(G, v, scalars):
    """(wave-tier keys, workgroup-tier keys, last key of the last set populated) of the run `v` describes, from the model alone"""
    run = Run(G, v, scalars)
    wave, big = FM.tiers(FM.run_counts(run.bstart, v.seg_len))
    return wave, big, bool(run.bstart[run.n_keys] > run.bstart[run.n_keys - 1])


def skew_on_route(gpu, G, h, n, ks, route, first, count, seed, wide=False):
    """the skewed and the all-equal scalar sets on a window-range run that takes `route`: both ends of big_list are populated (the
    model says so), so the tier lists of the route's run-offset kernel are compared on non-empty sets"""
    sk = skewed_scalars(G, n, seed)
    v = run_and_check(gpu, G, h, sk, ks, first=first, count=count, expect_route=route, expect_wide=wide, seg_variants=False)[0]
    wave, big, _ = model_tiers(G, v, sk)
    assert len(wave) >= 1 and len(big) >= 1, (len(wave), len(big))
    eq = [(G.r - 1) // 3] * n
    v = run_and_check(gpu, G, h, eq, ks, first=first, count=count, expect_route=route, expect_wide=wide, seg_variants=False)[0]
    wave, big, _ = model_tiers(G, v, eq)
    assert len(big) >= 1


def run_and_check(gpu, G, h, scalars, ks, first=0, count=0, expect_route=None, expect_wide=None, seg_variants=True, table_check=False):
    cid, grp = ids_of(G)
    sc = N.ints_to_limbs([s % (1 << 256) for s in scalars], 4)
    out = np.zeros(N.point_limbs(cid, grp), dtype=np.uint64)
    views = []
    variants = [None] + ([64, "creation"] if seg_variants else [])
    for lanes in variants:
        if lanes is not None:
            N.check(gpu.zk_msm_plan_set_option(h, b"segment_lanes", 64 if lanes == 64 else FM.SEG_TARGET_LANES))
        N.check(gpu.zk_msm_plan_run(h, len(scalars), sc.ctypes.data, 0, first, count, N.u64p(out), None))
        v = _view(gpu, h)
        views.append(v)
        target = 64 if lanes == 64 else FM.SEG_TARGET_LANES
        assert v.seg_len == FM.pick_seg_len(v.w_count * v.m, v.B, bool(v.pre), target), (v.seg_len, v.w_count * v.m, target)
        assert v.m == (2 if v.glv else 1) * len(scalars) and v.dstride == (v.m + 7) // 8 * 8 and v.groups == (1 if v.pre else v.w_count)
        if count:
            assert (v.w_first, v.w_count) == (first, count)
        if expect_route is not None:
            assert v.route_name == expect_route, f"the case is named after route {expect_route}, the run took {v.route_name}"
        if expect_wide is not None:
            assert bool(v.wide) == expect_wide
        run, logs = Run(G, v, scalars), Logs(G, v, ks)
        esz = 4 if v.wide else 2
        dig = _download(gpu, v.d_dig + (v.w_first - v.pw_first) * v.dstride * esz, v.w_count * v.dstride, np.uint32 if v.wide else np.uint16)
        buf = dict(dig=dig.reshape(v.w_count, v.dstride)[:, :v.m])
        buf["bstart"] = _download(gpu, v.bstart, v.n_keys + 1, np.uint32)
        FM.check_bstart(buf["bstart"], run)           # before anything is sized by it
        buf["sorted"] = _download(gpu, v.sorted, run.total, np.uint32)
        buf["sstart"] = _download(gpu, v.sstart, v.n_keys + 1, np.uint32)
        FM.check_sstart(buf["sstart"], run.bstart, v.seg_len)
        buf["big_list"] = _download(gpu, v.big_list, v.n_keys, np.uint32)
        buf["big_count"] = _download(gpu, v.big_count, 2, np.uint32)
        buf["partials"] = _download(gpu, v.partials, int(buf["sstart"][-1]) * G.XW, np.uint32).reshape(-1, G.XW)
        buf["buckets"] = _download(gpu, v.buckets, v.n_keys * G.XW, np.uint32).reshape(-1, G.XW)
        n_runs, n_buckets = check_front_buffers(G, v, run, logs, buf)
        print(f"[front] {G} n_api {v.n_api} c {v.c} glv {v.glv} pre {v.pre} wide {v.wide} windows {v.w_first}+{v.w_count} m {v.m} route {v.route_name} "
              f"fine_log {v.fine_log} split_fine {v.split_fine} seg_len {v.seg_len} entries {run.total} runs {int(buf['sstart'][-1])} "
              f"checked {n_runs} run rows, {n_buckets} bucket rows")
        if not count:   # the whole pipeline's point, from the logarithms
            want = FM.oracle_multiples(G, [sum(int(s % G.r) * int(k) for s, k in zip(scalars, ks)) % G.r])[0]
            assert corc.limbs_to_points(out.reshape(1, -1), cid, grp)[0] == want
        SEEN_ROUTES.add((v.route_name, bool(v.wide), bool(v.split_fine)))
    if table_check:
        check_base_table(gpu, G, views[0], ks)
    return views


def check_base_table(gpu, G, v, ks, max_rows=1 << 12):
    """item 5: d_bases rows out of Montgomery form against the oracle's multiples of the generator"""
    LW = G.LIMBS
    rows_total = (v.pw_count if v.pre else 1) * v.n
    idx = np.arange(rows_total) if rows_total <= max_rows else np.unique(np.concatenate([np.arange(64), np.arange(rows_total - 64, rows_total),
                                                                                    np.random.default_rng(5).choice(rows_total, size=max_rows, replace=False)]))
    raw = _download(gpu, v.d_bases, rows_total * 2 * LW, np.uint32).reshape(rows_total, 2 * LW)
    logs = Logs(G, v, ks)
    want = FM.oracle_multiples(G, [logs.row_log(int(i)) for i in idx])
    rinv = pow(G.f.R, -1, G.p)
    W32 = G.f.W
    for i, aff in zip(idx, want):
        ws = [int(x) for x in raw[i]]
        comps = [sum(ws[j * W32 + t] << (32 * t) for t in range(W32)) for j in range(2 * G.d)]
        assert all(x < 2 * G.p for x in comps), f"{G} base row {i}: a coordinate outside [0, 2p), the range the bucket step takes its base in"
        plain = [x * rinv % G.p for x in comps]
        got = (plain[0], plain[1]) if G.d == 1 else ((plain[0], plain[1]), (plain[2], plain[3]))
        assert got == aff, f"{G} base row {i} (n {v.n}, glv {v.glv}, pre {v.pre}): {got} != {aff}"


def with_plan(gpu, G, n, flags, c, ks, fn, win=None, options=()):
    cid, grp = ids_of(G)
    bases = make_bases(gpu, G, ks)
    h = N._u64(0)
    if win:
        N.check(gpu.zk_msm_plan_create_range(cid, grp, n, bases.ctypes.data, 0, flags, c, win[0], win[1], h))
    else:
        N.check(gpu.zk_msm_plan_create(cid, grp, n, bases.ctypes.data, 0, flags, c, h))
    try:
        for name, value in options:
            N.check(gpu.zk_msm_plan_set_option(h, name, value))
        wb, nw = N._i(0), N._i(0)
        N.check(gpu.zk_msm_plan_windows(h, wb, nw))
        return fn(h, wb.value, nw.value)
    finally:
        N.check(gpu.zk_msm_plan_destroy(h))


@pytest.mark.gpu
@pytest.mark.parametrize("flags", (0, N.MSM_NO_GLV), ids=("split", "no_glv"))
def test_ranged_small(gpu, flags):
    """bucket-range partition at n = 1000: every row checked; mixed scalars (zeros, 40-bit values, last-key scalars), all scalars
    equal, only 40-bit scalars, a short scalar vector, one scalar, a window range with first > 0, the view refused in flight"""
    G, n = BN_G1, 1000
    ks = small_logs(n, 0xF00 + flags)

    def body(h, c, nwin):
        mixed = mixed_scalars(G, (c, nwin), n, 0xF10, 125 if flags == 0 else 256)
        v = run_and_check(gpu, G, h, mixed, ks, expect_route="ranged", expect_wide=False, table_check=True)[0]
        assert bool(v.glv) == (flags == 0) and v.n == (2 * n if flags == 0 else n)
        run = Run(G, v, mixed)
        if not v.glv:   # the last key of every set but the top one is populated (the top window's digit is never negative)
            for s in range(v.w_count - 1):
                if (1 << (c * s + c - 1)) < G.r and 2 + 16 * s < n:
                    assert run.bstart[(s + 1) * v.B] > run.bstart[(s + 1) * v.B - 1], s
            assert run.bstart[v.w_count * v.B] == run.bstart[v.w_count * v.B - 1]
        assert run.bstart[1] > 0 and run.bstart[v.B] > run.bstart[v.B - 1], "first and last key of the first set"
        run_and_check(gpu, G, h, [(G.r - 1) // 3] * n, ks, expect_route="ranged", seg_variants=False)
        run_and_check(gpu, G, h, [s & ((1 << 40) - 1) for s in mixed], ks, expect_route="ranged", seg_variants=False)
        run_and_check(gpu, G, h, mixed[:333], ks, expect_route="ranged", seg_variants=False)
        run_and_check(gpu, G, h, [mixed[5]], ks, expect_route="ranged", seg_variants=False)
        # windows [1, 3): digits stored relative to the plan's first window; the top set of the run now has its last key
        vr = run_and_check(gpu, G, h, mixed, ks, first=1, count=2, expect_route="ranged", seg_variants=False)[0]
        rr = Run(G, vr, mixed)
        if not vr.glv:
            assert rr.bstart[2 * vr.B] > rr.bstart[2 * vr.B - 1], "sstart[n_keys] / the last key of the last set is populated here"
        # in flight: refused
        sc = N.ints_to_limbs(mixed, 4)
        N.check(gpu.zk_msm_plan_enqueue(h, n, sc.ctypes.data, 0, 0, 0, N.STREAM_PLAN))
        slots = np.zeros(FM.VIEW_SLOTS, dtype=np.uint64)
        assert gpu.zk_msm_plan_debug_view(h, N.u64p(slots), FM.VIEW_SLOTS) == N.ZK_ERR_ARG
        out = np.zeros(N.point_limbs(0, 1), dtype=np.uint64)
        N.check(gpu.zk_msm_plan_finish(h, N.u64p(out)))
        assert gpu.zk_msm_plan_debug_view(h, N.u64p(slots), FM.VIEW_SLOTS - 1) == N.ZK_ERR_ARG

    with_plan(gpu, G, n, flags, 0, ks, body)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", (0, N.MSM_NO_GLV), ids=("split", "no_glv"))
def test_ranged_2_16(gpu, flags):
    """the largest sizes the bucket-range partition sorts: the library's default plan (split scalars, m = 2^17 + 6) and the plain one"""
    G, n = BN_G1, (1 << 16) + 3
    ks = small_logs(n, 0xF20 + flags)
    with_plan(gpu, G, n, flags, 0, ks, lambda h, c, nwin: run_and_check(gpu, G, h, mixed_scalars(G, (c, nwin), n, 0xF21), ks, expect_route="ranged"))


@pytest.mark.gpu
def test_all_equal_scalars_fill_the_workgroup_tier(gpu):
    """one bucket per window holds every entry: thousands of runs (the back of big_list) at the plan's segment length"""
    G, n = BN_G1, 20000
    ks = small_logs(n, 0xF30)

    def body(h, c, nwin):
        v = run_and_check(gpu, G, h, [(G.r - 1) // 3] * n, ks, expect_route="ranged", seg_variants=False)[0]
        _, big = FM.tiers(FM.run_counts(Run(G, v, [(G.r - 1) // 3] * n).bstart, v.seg_len))
        assert len(big) >= 1

    with_plan(gpu, G, n, N.MSM_NO_GLV, 0, ks, body)


@pytest.mark.gpu
def test_two_level_derive_and_one_level_2_19(gpu):
    """general n = 2^19 + 5 (split scalars, m = 2^20 + 10): two-level sort with level-A offsets derived in the scatter kernel; with
    two_level_sort = 0 the chunked one-level sort; a one-window run of the same plan has a count matrix too large to derive from
    (one-workgroup scan); window ranges with first > 0 whose last set has its last key populated; skewed and all-equal scalars on
    the derive, scan and one-level routes (both ends of big_list populated)"""
    G, n = BN_G1, (1 << 19) + 5
    ks = small_logs(n, 0xF40)

    def body(h, c, nwin):
        mixed = mixed_scalars(G, (c, nwin), n, 0xF41)
        run_and_check(gpu, G, h, mixed, ks, expect_route="two-level-derive", expect_wide=False)
        # window ranges below the top window: the scalar 2^(cw + c - 1) of mixed_scalars puts an entry into the LAST key of the
        # last set, the bucket behind sstart[n_keys] -- on the scan, the ranged and the derive route of this plan
        for first, count, scalars, route in ((2, 1, mixed, "two-level-scan"), (1, 3, mixed[:70001], "ranged"), (2, 4, mixed, "two-level-derive")):
            v = run_and_check(gpu, G, h, scalars, ks, first=first, count=count, expect_route=route, seg_variants=False)[0]
            assert model_tiers(G, v, scalars)[2], f"{route}: the last key of the last set is populated"
        skew_on_route(gpu, G, h, n, ks, "two-level-derive", 2, 4, 0xF42)
        skew_on_route(gpu, G, h, n, ks, "two-level-scan", 5, 1, 0xF43)
        N.check(gpu.zk_msm_plan_set_option(h, b"two_level_sort", 0))
        run_and_check(gpu, G, h, mixed, ks, expect_route="one-level", seg_variants=False)
        skew_on_route(gpu, G, h, n, ks, "one-level", 3, 2, 0xF44)

    with_plan(gpu, G, n, 0, 0, ks, body)


@pytest.mark.gpu
def test_two_level_partial_16_bit(gpu, monkeypatch):
    """six fine bits (ZKMI_FINE_LOG, read when the plan is created): 8 x 512 (set, bin) pairs x 32 sub-histograms = 2^17 counts go
    through the sliced partial sums; rerun at segment_lanes 64 and at the creation value; a window range whose last key is populated; skewed
    and all-equal scalars (both ends of big_list populated)"""
    monkeypatch.setenv("ZKMI_FINE_LOG", "6")
    G, n = BN_G1, (1 << 19) + 5
    ks = small_logs(n, 0xF50)

    def body(h, c, nwin):
        mixed = mixed_scalars(G, (c, nwin), n, 0xF51)
        v = run_and_check(gpu, G, h, mixed, ks, expect_route="two-level-partial", expect_wide=False)[0]     # and at both segment lengths
        assert v.fine_log == 6
        # four windows x 512 bins x 64 sub-histograms is still 2^17 counts
        v = run_and_check(gpu, G, h, mixed, ks, first=1, count=4, expect_route="two-level-partial", seg_variants=False)[0]
        assert model_tiers(G, v, mixed)[2], "the last key of the last set is populated"
        skew_on_route(gpu, G, h, n, ks, "two-level-partial", 1, 4, 0xF52)

    with_plan(gpu, G, n, 0, 0, ks, body)


@pytest.mark.gpu
def test_fixed_base_2_12(gpu):
    """MSM_PRECOMPUTE at n = 2^12: ONE bucket set fed by every window (two-level, one-workgroup scan), the one-level sort with
    two_level_sort = 0, the table rows 2^(cw) P_i"""
    G, n = BN_G1, 1 << 12
    ks = small_logs(n, 0xF60)

    def body(h, c, nwin):
        mixed = mixed_scalars(G, (c, nwin), n, 0xF61)
        v = run_and_check(gpu, G, h, mixed, ks, expect_route="two-level-scan", expect_wide=False, table_check=True)[0]
        assert v.pre and v.groups == 1
        run = Run(G, v, mixed)
        assert run.bstart[v.B] > run.bstart[v.B - 1] and run.bstart[1] > 0, "first and last key of the shared set are populated"
        N.check(gpu.zk_msm_plan_set_option(h, b"two_level_sort", 0))
        run_and_check(gpu, G, h, mixed, ks, expect_route="one-level")

    with_plan(gpu, G, n, N.MSM_PRECOMPUTE, 0, ks, body)


@pytest.mark.gpu
def test_wide_scan_17_bit(gpu):
    """explicit 17-bit windows (32-bit digits) on a fixed-base plan of 2^14 points: all windows -> sliced partial sums, one window ->
    one-workgroup scan"""
    G, n = BN_G1, 1 << 14
    ks = small_logs(n, 0xF70)

    def body(h, c, nwin):
        assert c == 17
        mixed = mixed_scalars(G, (c, nwin), n, 0xF71)
        run_and_check(gpu, G, h, mixed, ks, expect_route="two-level-partial", expect_wide=True, seg_variants=False)
        v = run_and_check(gpu, G, h, mixed, ks, first=3, count=1, expect_route="two-level-scan", expect_wide=True)[0]
        assert model_tiers(G, v, mixed)[2], "the last key of the shared set is populated"
        # 2^14 equal scalars: one bucket of 2^14 entries per window, 2048 runs of eight -- the front of big_list on both wide routes
        eq = [(G.r - 1) // 3] * n
        for first, count, route in ((0, 0, "two-level-partial"), (3, 1, "two-level-scan")):
            v = run_and_check(gpu, G, h, eq, ks, first=first, count=count, expect_route=route, expect_wide=True, seg_variants=False)[0]
            assert len(model_tiers(G, v, eq)[0]) >= 1

    with_plan(gpu, G, n, N.MSM_PRECOMPUTE, 17, ks, body)


@pytest.mark.gpu
@pytest.mark.parametrize("n,split_fine", [(1 << 20, False), ((1 << 20) + 77, False), ((1 << 20) + (1 << 18) + 77, True)],
                         ids=("2_20", "2_20_plus_77", "1_25x2_20_plus_77_split_fine"))
def test_wide_fixed_base_2_20(gpu, n, split_fine):
    """the default fixed-base plan from 2^20 points on: 13 windows of 20 bits, 32-bit digits, 4096 coarse bins, the sliced partial
    sums; an odd size; and from 13 n > 2^24 table rows on (n = 1.25 * 2^20 + 77) a reference needs more than the 24 bits the 7 fine bits
    leave in a level-A entry, so the fine bits travel in a byte array beside the entries"""
    G = BN_G1
    ks = small_logs(n, 0xF80)

    def body(h, c, nwin):
        assert (c, nwin) == (20, 13)
        v = run_and_check(gpu, G, h, mixed_scalars(G, (c, nwin), n, 0xF81), ks, expect_route="two-level-partial", expect_wide=True, seg_variants=False)[0]
        assert bool(v.split_fine) == split_fine

    with_plan(gpu, G, n, N.MSM_PRECOMPUTE, 0, ks, body)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("general", "no_glv", "fixed"))
@pytest.mark.parametrize("G", GROUPS, ids=gid)
def test_all_groups(gpu, G, mode):
    """n = 2^12 + 1 in every group and plan kind, the Fp2 groups through both accumulate kernels: base table and run rows"""
    n = (1 << 12) + 1
    ks = small_logs(n, 0xF90 + G.gid)
    flags = {"general": 0, "no_glv": N.MSM_NO_GLV, "fixed": N.MSM_PRECOMPUTE}[mode]

    def body(h, c, nwin):
        mixed = mixed_scalars(G, (c, nwin), n, 0xF91 + G.gid)
        for split in ((0, 1) if G.d == 2 else (None,)):
            if split is not None:
                N.check(gpu.zk_msm_plan_set_option(h, b"split_pairs", split))
            v = run_and_check(gpu, G, h, mixed, ks, seg_variants=False, table_check=split in (None, 0))[0]
            assert split is None or v.split_acc == split
            assert bool(v.glv) == (mode == "general") and bool(v.pre) == (mode == "fixed")

    with_plan(gpu, G, n, flags, 0, ks, body)


@pytest.mark.gpu
@pytest.mark.parametrize("c", (2, 3, 8, 13, 16))
def test_explicit_window_bits(gpu, c):
    """two-key bucket sets (c = 2, B = 2), B = 4, and the 128 KiB LDS histogram of c = 16; no split, n = 3000"""
    G, n = BN_G1, 3000
    ks = small_logs(n, 0xFA0 + c)
    with_plan(gpu, G, n, N.MSM_NO_GLV, c, ks,
              lambda h, cc, nwin: run_and_check(gpu, G, h, mixed_scalars(G, (cc, nwin), n, 0xFA1 + c), ks, expect_route="ranged", seg_variants=c in (2, 16)))


@pytest.mark.gpu
def test_every_route_was_seen():
    """runs last in this module: every route of stage_sort was reported by a passing case, for 16- and 32-bit digits"""
    routes16 = {r for r, wide, _ in SEEN_ROUTES if not wide}
    routes32 = {r for r, wide, _ in SEEN_ROUTES if wide}
    assert routes16 >= {"ranged", "one-level", "two-level-derive", "two-level-scan", "two-level-partial"}, routes16
    assert routes32 >= {"two-level-scan", "two-level-partial"}, routes32      # wide windows exist in fixed-base plans only: no derive
    assert any(sf for _, _, sf in SEEN_ROUTES), "no case kept the fine bits beside the entries"
