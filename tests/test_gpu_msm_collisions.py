"""End-to-end MSMs on COLLIDING points through the C ABI.  Every other MSM test uses bases k_i G with random k_i: bucket sums are
then distinct random points and no addition after the accumulate kernel ever meets P = Q, P = -Q or an infinity in the middle of
a chain.  Here the bases come from the palette {+-G, +-2G, +-3G, infinity} or are all one point, so the combine tiers, the row /
column sums, the suffix scan and the host tail add equal, opposite and infinite points at every level.  The expected value is
the closed form (sum s_i k_i mod r) G in Python integers, the point from zk_point_mul (as test_msm_skewed_scalars_full_size) and,
up to 2^14 points, also from the CPU oracle's MSM.  Every input runs in general mode, without the scalar split (MSM_NO_GLV) and
in fixed-base mode (MSM_PRECOMPUTE); on each live plan the reduction runs with sum_one_step 0 / 1 and lanes_per_output
0 / 2 / 16 / 64, the G2 groups with split_pairs 0 and 1, and once as three window ranges summed on the host."""

import numpy as np
import pytest

from helpers import generator_limbs
from oracle import corc, pyref
from zksnake_amd import _native as N
from zksnake_amd import workloads as W

pytestmark = pytest.mark.gpu

GROUPS = [(0, 1), (0, 2), (1, 1), (1, 2)]
IDS = ["BN254_G1", "BN254_G2", "BLS12_381_G1", "BLS12_381_G2"]
MODES = (0, N.MSM_NO_GLV, N.MSM_PRECOMPUTE)
PALETTE = (1, -1, 2, -2, 3, -3, 0)     # multiples of G; 0 = the point at infinity
BASE_K = 7                             # "one point" of the all-equal inputs: 7 G


def _curve(cid):
    return pyref.BN254 if cid == 0 else pyref.BLS12_381


def _palette_rows(cid, grp, ks):
    g = pyref.Group(_curve(cid), grp)
    return corc.points_to_limbs([None if k == 0 else g.mul(g.gen, k) for k in ks], cid, grp)


def _expect(gpu, cid, grp, dot):
    out = np.zeros(N.point_limbs(cid, grp), dtype=np.uint64)
    N.check(gpu.zk_point_mul(cid, grp, N.u64p(generator_limbs(gpu, cid, grp)), N.u64p(N.ints_to_limbs([dot % _curve(cid).r])), N.u64p(out)))
    return out


def _run_modes(gpu, cid, grp, bases, sc, dot, c=0, modes=MODES, sweep=True):
    """the MSM of (sc, bases) on a plan of every mode, under every reduction / accumulate option, and as three window ranges"""
    from zksnake_amd.parallel import sum_points, window_ranges
    n = bases.shape[0]
    PW = N.point_limbs(cid, grp)
    exp = _expect(gpu, cid, grp, dot)
    if n <= 1 << 14:
        assert (corc.msm(cid, grp, sc, bases, threads=8) == exp).all(), "the closed form and the CPU oracle disagree"
    options = [()]
    if sweep:
        options += [((b"sum_one_step", 1), (b"lanes_per_output", lpo)) for lpo in (0, 2, 16, 64)] + [((b"sum_one_step", 0), (b"lanes_per_output", 0))]
    splits = (0, 1) if grp == 2 else (None,)
    for flags in modes:
        h = N._u64(0)
        N.check(gpu.zk_msm_plan_create(cid, grp, n, bases.ctypes.data, 0, flags, c, h))
        try:
            for split in splits:
                if split is not None:
                    N.check(gpu.zk_msm_plan_set_option(h, b"split_pairs", split))
                for opts in options:
                    for name, value in opts:
                        N.check(gpu.zk_msm_plan_set_option(h, name, value))
                    out = np.zeros(PW, dtype=np.uint64)
                    N.check(gpu.zk_msm_plan_run(h, n, sc.ctypes.data, 0, 0, 0, N.u64p(out), None))
                    assert (out == exp).all(), f"flags {flags} split_pairs {split} options {opts}"
            cb, nw = N._i(0), N._i(0)
            N.check(gpu.zk_msm_plan_windows(h, cb, nw))
            parts = []
            for first, count in window_ranges(nw.value, 3):
                part = np.zeros(PW, dtype=np.uint64)
                if count:
                    N.check(gpu.zk_msm_plan_run(h, n, sc.ctypes.data, 0, first, count, N.u64p(part), None))
                parts.append(part)
            assert (sum_points(cid, grp, parts) == exp).all(), f"flags {flags}: window ranges"
        finally:
            N.check(gpu.zk_msm_plan_destroy(h))


def _only_one_base(bases, sc_ints, ks, keep):
    """every base replaced by infinity except one"""
    b = np.zeros_like(bases)
    b[keep] = bases[keep]
    return b, sc_ints[keep] * ks[keep]


def _palette_input(cid, grp, n, seed, scalar_set=None):
    r = _curve(cid).r
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(PALETTE), size=n)
    ks = [PALETTE[i] for i in idx]
    bases = _palette_rows(cid, grp, PALETTE)[idx]
    if scalar_set is None:
        sc, ints = W.field_stream(0xC011 + seed, n, r)
    else:
        pick = rng.integers(0, len(scalar_set), size=n)
        ints = [scalar_set[i] for i in pick]
        sc = N.ints_to_limbs(scalar_set, 4)[pick]
    return np.ascontiguousarray(bases), np.ascontiguousarray(sc), ints, ks


@pytest.mark.parametrize("cid,grp", GROUPS, ids=IDS)
def test_palette_bases_random_scalars(gpu, cid, grp):
    """bases drawn from {+-G, +-2G, +-3G, infinity}: seven distinct rows, so every bucket sum is a small multiple of G and equal,
    opposite and infinite bucket sums meet all through the reduction; 2^20 points (n_keys >= 2^18: the two-step row / column sums)
    for BN254 G1"""
    sizes = [1 << 10, (1 << 16) + 3] + ([1 << 20] if (cid, grp) == (0, 1) else [])
    for n in sizes:
        bases, sc, ints, ks = _palette_input(cid, grp, n, 17 + n % 1000)
        _run_modes(gpu, cid, grp, bases, sc, sum(a * b for a, b in zip(ints, ks)))
        if n == 1 << 10:
            keep = n // 3 if ks[n // 3] else ks.index(1)
            b1, dot = _only_one_base(bases, ints, ks, keep)
            _run_modes(gpu, cid, grp, b1, sc, dot, sweep=False)


@pytest.mark.parametrize("cid,grp", GROUPS, ids=IDS)
def test_all_bases_equal_all_scalars_equal(gpu, cid, grp):
    """one bucket per window: every segment's second step is a doubling, every run of the bucket is the same point, and the wave /
    workgroup tiers of combine add equal partials at every tree level"""
    r = _curve(cid).r
    s = 0xDEADBEEFCAFEBABE1234567890ABCDEF0123456789ABCDEF % r
    row = _palette_rows(cid, grp, [BASE_K])
    for n in [1 << 12] + ([1 << 20] if (cid, grp) == (0, 1) else [1 << 16]):
        bases = np.ascontiguousarray(np.tile(row, (n, 1)))
        sc = np.ascontiguousarray(np.tile(N.ints_to_limbs([s]), (n, 1)))
        _run_modes(gpu, cid, grp, bases, sc, n * s * BASE_K)
        if n == 1 << 12:
            b1, dot = _only_one_base(bases, [s] * n, [BASE_K] * n, n // 3)
            _run_modes(gpu, cid, grp, b1, sc, dot, sweep=False)


@pytest.mark.parametrize("cid,grp", GROUPS, ids=IDS)
def test_alternating_bases_all_scalars_equal(gpu, cid, grp):
    """P, -P, P, ..: accumulators alternate between a point and infinity, runs of even length are infinity and so is the result;
    with one unpaired base at the end the result is s P"""
    r = _curve(cid).r
    s = 0x1234567890ABCDEFFEDCBA0987654321DEADBEEF % r
    rows = _palette_rows(cid, grp, [BASE_K, -BASE_K])
    n = 1 << 12
    for extra in (0, 1):
        m = n + extra
        ks = [BASE_K if i % 2 == 0 else -BASE_K for i in range(m)]
        bases = np.ascontiguousarray(rows[np.arange(m) % 2])
        sc = np.ascontiguousarray(np.tile(N.ints_to_limbs([s]), (m, 1)))
        _run_modes(gpu, cid, grp, bases, sc, extra * s * BASE_K)
        if extra == 0:
            out = np.zeros(N.point_limbs(cid, grp), dtype=np.uint64)
            N.check(gpu.zk_msm(cid, grp, m, m, N.u64p(sc), N.u64p(bases), N.u64p(out)))
            assert not out.any(), "everything cancels: the point at infinity"
            b1, dot = _only_one_base(bases, [s] * m, ks, m // 3)
            _run_modes(gpu, cid, grp, b1, sc, dot, sweep=False)


@pytest.mark.parametrize("c", [11, 13])
@pytest.mark.parametrize("cid,grp", GROUPS, ids=IDS)
def test_all_bases_equal_scalars_one_to_n(gpu, cid, grp, c):
    """scalars 1 .. n with n below half the bucket count of a window (2^(c-1) buckets of signed digits), no scalar split: every
    occupied bucket of the lowest window holds the same single point, so the row / column sums and the suffix scan add equal
    points only"""
    n = (1 << (c - 2)) - 1
    ints = list(range(1, n + 1))
    bases = np.ascontiguousarray(np.tile(_palette_rows(cid, grp, [BASE_K]), (n, 1)))
    sc = N.ints_to_limbs(ints, 4)
    _run_modes(gpu, cid, grp, bases, sc, BASE_K * n * (n + 1) // 2, c=c, modes=(N.MSM_NO_GLV, N.MSM_PRECOMPUTE))
    b1, dot = _only_one_base(bases, ints, [BASE_K] * n, n // 3)
    _run_modes(gpu, cid, grp, b1, sc, dot, c=c, modes=(N.MSM_NO_GLV,), sweep=False)


@pytest.mark.parametrize("cid,grp", GROUPS, ids=IDS)
def test_palette_bases_few_scalars(gpu, cid, grp):
    """scalars from {0, 1, 2, r - 1, r - 2}: few buckets, large equal and opposite sums"""
    r = _curve(cid).r
    n = 1 << 12
    bases, sc, ints, ks = _palette_input(cid, grp, n, 29, scalar_set=[0, 1, 2, r - 1, r - 2])
    _run_modes(gpu, cid, grp, bases, sc, sum(a * b for a, b in zip(ints, ks)))
    keep = next(i for i in range(n) if ks[i] and ints[i])
    b1, dot = _only_one_base(bases, ints, ks, keep)
    _run_modes(gpu, cid, grp, b1, sc, dot, sweep=False)
