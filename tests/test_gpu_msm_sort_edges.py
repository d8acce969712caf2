"""GPU: the split-scalar two-level sort at its edges -- sizes that do not divide the level-A chunks, one bucket holding every
entry (the big_list tiers of the combine stage), digits that are zero in most windows, the 2^22 split-scalar limit and
window-range runs whose count matrix is too large for the level-A workgroups to derive their own offsets.  Every result is
checked against the closed form (sum s_i k_i mod r) G with bases k_i G, with both settings of the two-level sort."""

import numpy as np
import pytest

from helpers import generator_limbs
from oracle import pyref
from zksnake_amd import _native as N
from zksnake_amd import workloads as W

pytestmark = pytest.mark.gpu

CID, GRP = 0, 1
R = pyref.BN254.r


def _bases(gpu, n, seed):
    ks = W.splitmix64(seed, 4 * n).reshape(n, 4)
    ks[:, 3] &= np.uint64((1 << 60) - 1)
    gen = generator_limbs(gpu, CID, GRP)
    bases = np.zeros((n, N.point_limbs(CID, GRP)), dtype=np.uint64)
    N.check(gpu.zk_batch_mul(CID, GRP, n, N.u64p(ks), N.u64p(gen), 1, N.u64p(bases)))
    k_ints = [int.from_bytes(row.tobytes(), "little") for row in ks]
    return bases, k_ints


def _expected(gpu, sc_ints, k_ints):
    dot = sum(a * b for a, b in zip(sc_ints, k_ints)) % R
    exp = np.zeros(N.point_limbs(CID, GRP), dtype=np.uint64)
    N.check(gpu.zk_point_mul(CID, GRP, N.u64p(generator_limbs(gpu, CID, GRP)), N.u64p(N.ints_to_limbs([dot])), N.u64p(exp)))
    return exp


def _ints(limbs):
    return [int.from_bytes(row.tobytes(), "little") for row in limbs]


def _run_both_sorts(gpu, bases, sc, windows=None, routes=None):
    """the plan's result with the two-level sort and without; `windows`: run as these (first, count) ranges and add up;
    `routes`: a list that receives (two_level option, sort route of the run) from the plan's debug view"""
    from zksnake_amd.parallel import sum_points
    n = bases.shape[0]
    h = N._u64(0)
    N.check(gpu.zk_msm_plan_create(CID, GRP, n, bases.ctypes.data, 0, 0, 0, h))
    outs = []
    try:
        for two_level in (1, 0, 1):
            N.check(gpu.zk_msm_plan_set_option(h, b"two_level_sort", two_level))
            parts = []
            for first, count in windows or [(0, 0)]:
                out = np.zeros(N.point_limbs(CID, GRP), dtype=np.uint64)
                N.check(gpu.zk_msm_plan_run(h, sc.shape[0], sc.ctypes.data, 0, first, count, N.u64p(out), None))
                parts.append(out)
                if routes is not None:
                    view = np.zeros(N.MSM_VIEW_SLOTS, dtype=np.uint64)
                    N.check(gpu.zk_msm_plan_debug_view(h, N.u64p(view), N.MSM_VIEW_SLOTS))
                    routes.append((two_level, int(view[N.MSM_VIEW_ROUTE])))
            outs.append(parts[0] if len(parts) == 1 else sum_points(CID, GRP, parts))
    finally:
        N.check(gpu.zk_msm_plan_destroy(h))
    return outs


@pytest.mark.parametrize("n", [(1 << 18) + 1, (1 << 20) - 3])
def test_sizes_off_the_chunk_length(gpu, n):
    bases, k_ints = _bases(gpu, n, 0x51E5 + n)
    sc, sc_ints = W.field_stream(0xD161 + n, n, R)
    exp = _expected(gpu, sc_ints, k_ints)
    for out in _run_both_sorts(gpu, bases, sc):
        assert (out == exp).all()


def test_one_bucket_holds_every_entry(gpu):
    """all scalars equal: every window puts all 2^21 entries into one bucket (far above the LDS stage of level B), which the
    combine stage reduces through its workgroup tier"""
    n = 1 << 20
    bases, k_ints = _bases(gpu, n, 0xB16)
    s = (R - 1) // 3
    sc = np.tile(N.ints_to_limbs([s], 4), (n, 1))
    exp = _expected(gpu, [s] * n, k_ints)
    for out in _run_both_sorts(gpu, bases, sc):
        assert (out == exp).all()


def test_digits_zero_in_most_windows(gpu):
    """40-bit scalars: the second half of the split is zero and only the low windows of the first half carry entries, so
    whole windows are empty and the offsets of the windows after them must not move"""
    n = (1 << 19) + 7
    bases, k_ints = _bases(gpu, n, 0x2E60)
    sc = W.splitmix64(0x2E61, 4 * n).reshape(n, 4)
    sc[:, 1:] = 0
    sc[:, 0] &= np.uint64((1 << 40) - 1)
    sc[::5, 0] = 0  # and some scalars are zero altogether
    exp = _expected(gpu, _ints(sc), k_ints)
    for out in _run_both_sorts(gpu, bases, sc):
        assert (out == exp).all()


def test_mixed_skew_at_the_split_scalar_limit(gpu):
    """2^22 points, the largest split-scalar plan: coarse bins above the register and LDS stages of level B, a quarter of
    the scalars equal"""
    n = 1 << 22
    bases, k_ints = _bases(gpu, n, 0x4A22)
    sc, sc_ints = W.field_stream(0x4A23, n, R)
    sc[::4] = N.ints_to_limbs([12345], 4)[0]
    sc_ints = [12345 if i % 4 == 0 else v for i, v in enumerate(sc_ints)]
    exp = _expected(gpu, sc_ints, k_ints)
    for out in _run_both_sorts(gpu, bases, sc):
        assert (out == exp).all()


@pytest.mark.parametrize("n,world", [((1 << 18) + 1, 2), ((1 << 20) - 3, 3), ((1 << 20) - 3, 8)])
def test_window_range_runs(gpu, n, world):
    """window-range runs of one plan (what a sharded rank does): fewer windows, more chunks per window, so the count matrix
    goes through the scan launch unless it is small; the partial points add up to the full MSM"""
    from zksnake_amd.parallel import window_ranges
    bases, k_ints = _bases(gpu, n, 0x3A4E)
    sc, sc_ints = W.field_stream(0x3A4F, n, R)
    exp = _expected(gpu, sc_ints, k_ints)
    h = N._u64(0)
    N.check(gpu.zk_msm_plan_create(CID, GRP, n, bases.ctypes.data, 0, 0, 0, h))
    nw = N._i(0)
    try:
        N.check(gpu.zk_msm_plan_windows(h, N._i(0), nw))
    finally:
        N.check(gpu.zk_msm_plan_destroy(h))
    ranges = [rc for rc in window_ranges(nw.value, world) if rc[1] > 0]
    routes = []
    for out in _run_both_sorts(gpu, bases, sc, ranges, routes):
        assert (out == exp).all()
    # 2^18 + 1 points in two halves: 64 chunks x 128 bins, small enough for the level-A workgroups to derive their offsets; the
    # other two shapes have more chunks per window and go through the scan launch
    want = N.MSM_ROUTE_TWO_LEVEL_DERIVE if (n, world) == ((1 << 18) + 1, 2) else N.MSM_ROUTE_TWO_LEVEL_SCAN
    assert {r for on, r in routes if on} == {want} and {r for on, r in routes if not on} == {N.MSM_ROUTE_ONE_LEVEL}, routes
