"""GPU: two live plans of different groups and scalar fields share one body of front code and nothing else.

The digits-and-sort front of an MSM plan (MsmFront, csrc/msm_front.hip) is compiled once for all four groups: a BN254 G1 plan and
a BLS12-381 G2 plan run the same kernels, launched by the same host code, with the large-LDS attributes set on one set of kernel
symbols.  Everything a sort owns must therefore hang off the plan's own front, never off the code they share.  Here plan B runs
a whole MSM between the two halves of plan A's run (enqueue_sort ... enqueue_rest), on another curve, with another scalar field,
window width, digit stride and bucket count; a front that kept anything per process (a buffer, the layout, the route it last took)
would hand A's accumulate kernel B's sort, or report B's sort in A's debug view.

  plan A  BN254 G1, 300 points        plan B  BLS12-381 G2, 77 points, MSM_NO_GLV
  1. A.enqueue_sort   2. B.run   3. A.enqueue_rest   4. A.finish
  - both points == pyref's MSM (the plain double-and-add definition over Python integers), bit for bit;
  - afterwards each debug view describes the plan's OWN sort: n, n_api, c, route, dstride, m;
  - the device pointers of slots 0 and 2..6 (digits, sorted, bstart, sstart, big_list, big_count) of A and B are pairwise different.

Pairs (each with A created first and with B created first -- the second plan's creation sets the function attributes again):
  general     default flags: split scalars for A (600 entries, dstride 600), plain for B (77 entries, dstride 80); both take the
              bucket-range sort (general mode, m < 2^19): ZK_MSM_ROUTE_RANGED.
  precompute  both MSM_PRECOMPUTE at window_bits = 16.  With the default options such a plan sorts in two levels (5 fine bits:
              1024 coarse bins of the one shared bucket set x 16 sub-histograms, fewer than 2^17 counters, so one workgroup
              scans them): ZK_MSM_ROUTE_TWO_LEVEL_SCAN.
  one_level   the same two plans with "two_level_sort" switched off: ZK_MSM_ROUTE_ONE_LEVEL, the chunked sort whose histogram
              takes 2^15 x 4 B = 128 KiB of LDS per workgroup, in both scalar fields.
These are the smallest shapes at which ownership can go wrong; the pyref points are computed once and shared by all cases."""

import numpy as np
import pytest

from helpers import oracle_bases, rand_scalars
from oracle import corc, pyref
from test_gpu_msm_plan_reuse import Plan
from zksnake_amd import _native as N

pytestmark = pytest.mark.gpu

V_DIG, V_SORTED, V_BSTART, V_SSTART, V_BIG_LIST, V_BIG_COUNT = 0, 2, 3, 4, 5, 6
V_N, V_N_API, V_C, V_PRE, V_M, V_DSTRIDE = 9, 10, 11, 15, 23, 24
OWNED = (V_DIG, V_SORTED, V_BSTART, V_SSTART, V_BIG_LIST, V_BIG_COUNT)


class Side:
    """one plan's inputs and its expected point: made once, shared by every case, never modified"""

    def __init__(self, cid, grp, n, seed):
        self.cid, self.grp, self.n = cid, grp, n
        cv = pyref.BN254 if cid == 0 else pyref.BLS12_381
        self.words = N.point_limbs(cid, grp)
        _, self.bases = oracle_bases(cid, grp, n, seed)
        vals, _ = rand_scalars(n, cv.r, seed + 1)
        vals[0], vals[1], vals[n - 1] = 0, 1, cv.r - 1
        self.scalars = N.ints_to_limbs(vals, 4)
        g = pyref.Group(cv, grp)
        self.expect = corc.points_to_limbs([g.msm(corc.limbs_to_points(self.bases, cid, grp), vals)], cid, grp)[0]
        for a in (self.bases, self.scalars, self.expect):
            a.setflags(write=False)


_SIDES = {}


def sides():
    if not _SIDES:
        _SIDES["A"] = Side(0, 1, 300, 5100)
        _SIDES["B"] = Side(1, 2, 77, 5200)
    return _SIDES["A"], _SIDES["B"]


class PlanAt(Plan):
    """Plan with the window width given at creation"""

    def __init__(self, lib, cs, flags, window_bits):
        self.lib, self.cs, self.flags = lib, cs, flags
        h = N._u64(0)
        N.check(lib.zk_msm_plan_create(cs.cid, cs.grp, cs.n, cs.bases.ctypes.data, 0, flags, window_bits, h))
        self.h = h.value
        c, nw, ent = N._i(0), N._i(0), N._u64(0)
        N.check(lib.zk_msm_plan_windows(self.h, c, nw))
        N.check(lib.zk_msm_plan_entries(self.h, ent))
        self.c, self.nwin, self.entries = c.value, nw.value, ent.value

    def view(self):
        v = np.zeros(N.MSM_VIEW_SLOTS, dtype=np.uint64)
        N.check(self.lib.zk_msm_plan_debug_view(self.h, N.u64p(v), N.MSM_VIEW_SLOTS))
        return [int(x) for x in v]


# flags of A, flags of B, window_bits, "two_level_sort" (None: as created), entries per point of A, c of A and of B, route
PAIRS = {
    # c = log2(entries) - 2, at least 4 (pick_window_bits): 600 entries -> 7, 77 -> 4
    "general": (0, N.MSM_NO_GLV, 0, None, 2, (7, 4), N.MSM_ROUTE_RANGED),
    "precompute": (N.MSM_PRECOMPUTE, N.MSM_PRECOMPUTE, 16, None, 1, (16, 16), N.MSM_ROUTE_TWO_LEVEL_SCAN),
    "one_level": (N.MSM_PRECOMPUTE, N.MSM_PRECOMPUTE, 16, 0, 1, (16, 16), N.MSM_ROUTE_ONE_LEVEL),
}


@pytest.mark.parametrize("first", ["A_first", "B_first"])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_two_plans_of_other_curves_interleaved(gpu, pair, first):
    flags_a, flags_b, wbits, two_level, per_point, cs, route = PAIRS[pair]
    sa, sb = sides()
    plans = {}
    try:
        for k in ("A", "B") if first == "A_first" else ("B", "A"):
            plans[k] = PlanAt(gpu, sa if k == "A" else sb, flags_a if k == "A" else flags_b, wbits)
            if two_level is not None:
                N.check(plans[k].option(b"two_level_sort", two_level))
        a, b = plans["A"], plans["B"]
        N.check(a.enqueue_sort(sa.scalars))
        got_b = b.run(sb.scalars)
        N.check(a.enqueue_rest())
        got_a = a.finish()
        assert (got_b == sb.expect).all(), "plan B (BLS12-381 G2) differs from pyref's MSM"
        assert (got_a == sa.expect).all(), "plan A (BN254 G1) differs from pyref's MSM"
        va, vb = a.view(), b.view()
        for name, p, v, s, c, m in (("A", a, va, sa, cs[0], per_point * sa.n), ("B", b, vb, sb, cs[1], sb.n)):
            want = {V_N: m, V_N_API: s.n, V_C: c, V_PRE: 1 if p.flags & N.MSM_PRECOMPUTE else 0, N.MSM_VIEW_ROUTE: route, V_DSTRIDE: (m + 7) & ~7, V_M: m}
            assert {k: v[k] for k in want} == want, f"plan {name}'s view does not describe its own sort"
        ptrs = [va[k] for k in OWNED] + [vb[k] for k in OWNED]
        assert all(ptrs) and len(set(ptrs)) == len(ptrs), "the two plans' fronts share a buffer"
    finally:
        for p in plans.values():
            p.destroy()
