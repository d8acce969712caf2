"""GPU: an MSM plan carries nothing from one run into the next.

A prover keeps a handful of plans alive for the life of a key and pushes run after run through them: other scalars, other
lengths, other window ranges, through every entry point (enqueue, enqueue_sort + enqueue_rest, enqueue_shared, cancel,
wait_event).  Here ONE plan sees a fixed sequence of unlike runs, and every run is compared (==) with the CPU oracle: corc.msm
over bases made by the oracle; a window range is the oracle's MSM of the scalars cut down to the signed digits of those windows
(helpers.window_range_scalars).  No expectation comes from another run of the library.

What each step would expose if the member named were cleaned at plan creation only, or not awaited:

1. test_one_plan_a_sequence_of_unlike_runs (all four groups at n = 1500, BN254 also at 2^13 + 3; split scalars, NO_GLV, PRECOMPUTE)
   a  random scalars                      the fresh plan (baseline of everything below)
   b  all zero                            buckets, partials, rows, fin, h_final: no entry lands anywhere (bstart[n_keys] = 0, the
                                          accumulate kernel leaves at once), combine_kernel must set EVERY bucket to infinity
   c  all r - 1, then all one value       big_list / big_count: one bucket per window holds every entry, more runs than
                                          COMBINE_SMALL_MAX -- the wave tier of combine_kernel; twice, so the list is reused
   d  random again                        big_count (zeroed by the digits kernel of each run), stale big_list entries, sstart
   e  n - 1, 1, 0, n scalars              d_dig (rows are dstride = m rounded up to 8 apart: the stride moves), d_scalars' tail,
                                          hist / total of the chunks that a short run does not reach; q_m == 0 launches nothing,
                                          finish gives infinity, and the next run must not inherit ws.* or q_m from it
   f  windows [1, 2), all, last, all      ws.groups, ws.w_first, ws.w_count, n_keys and the dig_base offset; bstart / sstart /
                                          buckets beyond a one-window run keep the previous run's content
   g  device scalars, host, device        d_scalars (the plan's staging copy) against the caller's buffer, both ways
   h  caller's stream, then STREAM_PLAN   q_stream; ev_start / ev_end / ev_acc* recorded on another stream than the last time
   i  two_level_sort, sum_one_step,       tmp_ref / bin_start / bin_runs / slice_sums of the two-level sort against hist / total
      segment_lanes, lanes_per_output     of the one-level one (fixed-base plans change route, asserted), seg_len and with it
      flipped, then (a) and (c) again     sstart / partials / big_list, parts / rows of the strided sums
2. cancel
   idle                                   nothing: ZK_OK
   after enqueue                          q_pending (finish refused), then a run of other scalars: every buffer of the abandoned
                                          run, h_final included
   between enqueue_sort and enqueue_rest  q_sorted (enqueue_rest and finish refused), ws.seg_len of the abandoned sort
   the lender, borrower in flight         the borrower reads sorted / bstart / sstart / big_list / big_count of a plan that is idle
                                          again; the lender's next run must wait for ev_release (ws.lent) before its digits kernel
                                          zeroes big_count and its sort overwrites the lists
   the borrower                           the lender's ws.lent with ev_release recorded by a run nobody collected; sharing again
3. borrowing from a lender that has only sorted
                                          sorted_ready = ws.ev_acc0 and ws.seg_len must come from phase 1 (enqueue_sort);
                                          a refused borrower (other size) leaves ws.lent set with ev_release never recorded:
                                          the lender's next run waits for it and must not stall
4. zk_msm_plan_wait_event                 the plan's stream must wait for the event before the digits kernel reads the caller's
                                          device scalars: they arrive behind a spin on another (non-blocking) stream; without
                                          the wait the run multiplies the buffer's earlier content (a valid, different point)
5. through PointArray                     one plan() handle over three multiexp calls of other lengths; release() with a run (and
                                          with a sort only) left enqueued: _drop's cancel, then a new plan on the same slot

Sizes: n = 1500 and 2^13 + 3, as the issue sets them.  At these sizes a general plan always takes the bucket-range sort (m < 2^19)
and the strided sums are one step (fewer than 2^18 buckets) whatever the knobs say; a fixed-base plan switches between the
two-level and the chunked one-level sort with "two_level_sort"."""

import ctypes

import numpy as np
import pytest

import stream_state_child as S
from helpers import oracle_bases, rand_scalars, window_range_scalars
from oracle import corc, pyref
from zksnake_amd import _native as N
from zksnake_amd.device import DeviceBuffer

pytestmark = pytest.mark.gpu

N_SMALL, N_ODD = 1500, (1 << 13) + 3
MODES = [0, N.MSM_NO_GLV, N.MSM_PRECOMPUTE]
MODE_IDS = ["split", "no_glv", "precompute"]
GROUPS_AT_SIZES = [(0, 1, N_SMALL), (0, 2, N_SMALL), (1, 1, N_SMALL), (1, 2, N_SMALL), (0, 1, N_ODD), (0, 2, N_ODD)]
SHARED = [(N.MSM_PRECOMPUTE, N_SMALL), (N.MSM_NO_GLV, N_SMALL), (N.MSM_PRECOMPUTE, N_ODD), (N.MSM_NO_GLV, N_ODD)]
SHARED_IDS = ["precompute-1500", "no_glv-1500", "precompute-8195", "no_glv-8195"]


# ---- inputs and oracle expectations: computed once per (curve, group, n), shared, never modified ----------------------------------
class Case:
    def __init__(self, cid, grp, n):
        self.cid, self.grp, self.n = cid, grp, n
        self.r = (pyref.BN254 if cid == 0 else pyref.BLS12_381).r
        self.words = N.point_limbs(cid, grp)
        _, self.bases = oracle_bases(cid, grp, n, 7000 + 100 * cid + 10 * grp + (n & 7))
        self._sc, self._exp = {}, {}

    def ints(self, tag):
        return self._scalars(tag)[0]

    def limbs(self, tag):
        return self._scalars(tag)[1]

    def _scalars(self, tag):
        """tag: "zero", "rm1" (all r - 1), "same" (all one random value) or a letter (random; 0, 1 and r - 1 among them).
        Tags mean the same scalars in every group of a curve: a G2 plan borrows the sort of a G1 plan's run over them."""
        if tag not in self._sc:
            n, r = self.n, self.r
            if tag == "zero":
                vals = [0] * n
            elif tag == "rm1":
                vals = [r - 1] * n
            elif tag == "same":
                vals = [rand_scalars(1, r, 4242 + self.cid)[0][0]] * n
            else:
                vals, _ = rand_scalars(n, r, 9000 + 31 * ord(tag) + self.cid)
                vals[3], vals[n // 2], vals[n - 1] = 0, 1, r - 1
            limbs = N.ints_to_limbs(vals, 4)
            limbs.setflags(write=False)
            self._sc[tag] = (vals, limbs)
        return self._sc[tag]

    def expect(self, tag, m=None, windows=None):
        """the oracle's point for the first m scalars of `tag`; windows = (c, nwin, glv, first, count) of a window-range run"""
        m = self.n if m is None else m
        key = (tag, m, windows)
        if key not in self._exp:
            if windows is None:
                sc = self.limbs(tag)[:m]
            else:
                sc = N.ints_to_limbs(window_range_scalars(self.cid, self.grp, self.ints(tag)[:m], *windows), 4)
            e = corc.msm(self.cid, self.grp, sc, self.bases[:m], threads=8)
            e.setflags(write=False)
            self._exp[key] = e
        return self._exp[key]


_CASES = {}


def case(cid, grp, n):
    if (cid, grp, n) not in _CASES:
        _CASES[(cid, grp, n)] = Case(cid, grp, n)
    return _CASES[(cid, grp, n)]


# ---- one live plan ---------------------------------------------------------------------------------------------------------------------
class Plan:
    def __init__(self, lib, cs, flags, n=None):
        self.lib, self.cs, self.flags = lib, cs, flags
        h = N._u64(0)
        n = cs.n if n is None else n
        N.check(lib.zk_msm_plan_create(cs.cid, cs.grp, n, cs.bases.ctypes.data, 0, flags, 0, h))
        self.h = h.value
        c, nw, ent = N._i(0), N._i(0), N._u64(0)
        N.check(lib.zk_msm_plan_windows(self.h, c, nw))
        N.check(lib.zk_msm_plan_entries(self.h, ent))
        self.c, self.nwin, self.glv = c.value, nw.value, ent.value == 2 * n
        assert ent.value in (n, 2 * n)

    # the three enqueue forms return the status; the scalars are a host limb array or a device pointer (dev=True)
    def _args(self, sc, m, first, count, dev):
        if dev:
            return (self.h, self.cs.n if m is None else m, sc, 1, first, count)
        return (self.h, sc.shape[0] if m is None else m, sc.ctypes.data, 0, first, count)

    def enqueue(self, sc, m=None, first=0, count=0, dev=False, stream=N.STREAM_PLAN):
        return self.lib.zk_msm_plan_enqueue(*self._args(sc, m, first, count, dev), stream)

    def enqueue_sort(self, sc, m=None, first=0, count=0, dev=False, stream=N.STREAM_PLAN):
        return self.lib.zk_msm_plan_enqueue_sort(*self._args(sc, m, first, count, dev), stream)

    def enqueue_rest(self, after=0):
        return self.lib.zk_msm_plan_enqueue_rest(self.h, after)

    def enqueue_shared(self, lender, stream=N.STREAM_PLAN):
        return self.lib.zk_msm_plan_enqueue_shared(self.h, lender.h, stream)

    def cancel(self):
        return self.lib.zk_msm_plan_cancel(self.h)

    def finish_status(self):
        return self.lib.zk_msm_plan_finish(self.h, N.u64p(np.zeros(self.cs.words, dtype=np.uint64)))

    def finish(self):
        out = np.full(self.cs.words, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)   # infinity must be WRITTEN, not found there
        N.check(self.lib.zk_msm_plan_finish(self.h, N.u64p(out)))
        return out

    def run(self, sc, **kw):
        N.check(self.enqueue(sc, **kw))
        return self.finish()

    def two_step(self, sc, **kw):
        N.check(self.enqueue_sort(sc, **kw))
        N.check(self.enqueue_rest())
        return self.finish()

    def option(self, name, value):
        return self.lib.zk_msm_plan_set_option(self.h, name, value)

    def route(self):
        view = np.zeros(N.MSM_VIEW_SLOTS, dtype=np.uint64)
        N.check(self.lib.zk_msm_plan_debug_view(self.h, N.u64p(view), N.MSM_VIEW_SLOTS))
        return int(view[N.MSM_VIEW_ROUTE])

    def destroy(self):
        if self.h is not None:
            N.check(self.lib.zk_msm_plan_destroy(self.h))
            self.h = None


class Steps:
    """compares step after step and keeps going after a wrong point, so that one run of the sequence names every step that fails
    (a wrong point is not a fault; a status other than ZK_OK raises at once)"""

    def __init__(self):
        self.bad, self.done = [], 0

    def check(self, label, got, want):
        self.done += 1
        if not (got == want).all():
            self.bad.append(label)

    def settle(self):
        assert not self.bad, f"{len(self.bad)} of {self.done} runs differ from the CPU oracle, in this order: {self.bad}"


# ---- 1. one plan, a sequence of unlike runs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("cid,grp,n", GROUPS_AT_SIZES)
def test_one_plan_a_sequence_of_unlike_runs(gpu, cid, grp, n, flags):
    cs = case(cid, grp, n)
    pre = flags == N.MSM_PRECOMPUTE
    p = Plan(gpu, cs, flags)
    st = S.new_stream(gpu)
    dbuf = None
    s = Steps()
    try:
        # the window-range model against itself: every window together is the scalar again
        assert window_range_scalars(cid, grp, cs.ints("A")[:40], p.c, p.nwin, p.glv, 0, p.nwin) == [v % cs.r for v in cs.ints("A")[:40]]

        def go(label, tag, m=None, **kw):
            s.check(label, p.run(cs.limbs(tag), m=m, **kw), cs.expect(tag, m))

        # a. the fresh plan
        go("a random", "A")
        # b. nothing lands in a bucket: buckets / partials / rows / fin / h_final of (a) would show
        go("b zero", "zero")
        # c. one bucket per window holds everything: big_list / big_count (wave tier of the combine), twice
        go("c r-1", "rm1")
        go("c same", "same")
        # d. random again must not see the big-bucket list of (c): big_count, big_list, sstart
        go("d random", "B")
        # e. lengths: the digit rows' stride and the chunks move; the zero-length run launches nothing (q_m == 0) and the
        #    run after it starts from whatever ws.* the run BEFORE it left
        go("e n-1", "B", n - 1)
        go("e 1", "C", 1)
        go("e 0", "C", 0)
        go("e n", "C", n)
        # f. window ranges: ws.groups / ws.w_first / ws.w_count / n_keys and the dig_base offset move
        if not pre:
            for label, first, count in (("f [1,2)", 1, 1), ("f all", 0, p.nwin), ("f last", p.nwin - 1, 1), ("f plan's range", 0, 0)):
                want = cs.expect("A") if count in (0, p.nwin) else cs.expect("A", None, (p.c, p.nwin, p.glv, first, count))
                s.check(label, p.run(cs.limbs("A"), first=first, count=count), want)
        # g. the caller's device buffer, then the host (through the plan's d_scalars), then the device buffer again
        dbuf = DeviceBuffer.from_numpy(cs.limbs("D"))
        s.check("g device", p.run(dbuf.ptr, dev=True), cs.expect("D"))
        go("g host", "E")
        s.check("g device again", p.run(dbuf.ptr, dev=True), cs.expect("D"))
        s.check("g device, shorter", p.run(dbuf.ptr, m=n - 7, dev=True), cs.expect("D", n - 7))
        # h. a caller's stream, then the plan's own: q_stream and the streams the plan's events were recorded on
        go("h caller's stream", "A", stream=st)
        go("h plan's stream", "B")
        # i. the knobs of the live plan between runs, then (a) and (c) again
        N.check(p.option(b"two_level_sort", 0))
        N.check(p.option(b"sum_one_step", 1))
        go("i one-level random", "A")
        assert p.route() == (N.MSM_ROUTE_ONE_LEVEL if pre else N.MSM_ROUTE_RANGED)
        go("i one-level r-1", "rm1")
        go("i one-level same", "same")
        two_level = p.option(b"two_level_sort", 1)     # refused (ZK_ERR_ARG) by a plan created without that sort's buffers
        assert two_level == N.ZK_OK if pre else two_level in (N.ZK_OK, N.ZK_ERR_ARG)
        N.check(p.option(b"sum_one_step", 0))
        N.check(p.option(b"segment_lanes", 64))        # the longest segments: fewer runs per bucket, other sstart / partials
        N.check(p.option(b"lanes_per_output", 16))
        go("i long segments random", "A")
        assert p.route() in (N.MSM_ROUTES_TWO_LEVEL if pre else (N.MSM_ROUTE_RANGED,))
        go("i long segments r-1", "rm1")
        go("i long segments same", "same")
        N.check(p.option(b"segment_lanes", 256 * 1024))
        N.check(p.option(b"lanes_per_output", 0))
        go("i defaults again, random", "B")
        go("i defaults again, zero", "zero")
        s.settle()
    finally:
        p.destroy()
        N.check(gpu.zk_stream_destroy(st))
        if dbuf is not None:
            dbuf.free()


# ---- 2. cancel ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("cid,grp", [(0, 1), (1, 2)])
def test_cancel_returns_the_plan_to_idle(gpu, cid, grp, flags):
    cs = case(cid, grp, N_SMALL)
    p = Plan(gpu, cs, flags)
    s = Steps()
    try:
        assert p.cancel() == N.ZK_OK                                   # idle
        # a complete run in flight
        N.check(p.enqueue(cs.limbs("A")))
        assert p.cancel() == N.ZK_OK
        assert p.finish_status() == N.ZK_ERR_ARG                       # nothing pending any more
        assert p.cancel() == N.ZK_OK                                   # idle again
        s.check("run after cancel", p.run(cs.limbs("B")), cs.expect("B"))
        # sorted only
        N.check(p.enqueue_sort(cs.limbs("rm1")))
        assert p.cancel() == N.ZK_OK
        assert p.enqueue_rest() == N.ZK_ERR_ARG
        assert p.finish_status() == N.ZK_ERR_ARG
        s.check("two-step run after cancel", p.two_step(cs.limbs("C")), cs.expect("C"))
        # a cancelled zero-length run, and a cancelled short one before a full one
        N.check(p.enqueue(cs.limbs("A"), m=0))
        assert p.cancel() == N.ZK_OK
        N.check(p.enqueue(cs.limbs("A"), m=5))
        assert p.cancel() == N.ZK_OK
        s.check("run after cancelled short runs", p.run(cs.limbs("D")), cs.expect("D"))
        s.settle()
    finally:
        h = p.h
        p.destroy()
    assert gpu.zk_msm_plan_cancel(h) == N.ZK_ERR_ARG                   # unknown handle (handle values are never reused)
    assert b"unknown MSM plan handle" in gpu.zk_last_error()


@pytest.mark.parametrize("flags,n", SHARED, ids=SHARED_IDS)
def test_cancel_with_a_shared_sort_in_flight(gpu, flags, n):
    g1, g2 = case(0, 1, n), case(0, 2, n)
    lender, borrower = Plan(gpu, g1, flags), Plan(gpu, g2, flags)
    s = Steps()
    try:
        # cancel the lender under the borrower, and start the lender's next run at once: it overwrites what the borrower reads
        # unless it waits for ev_release
        N.check(lender.enqueue(g1.limbs("A")))
        N.check(borrower.enqueue_shared(lender))
        assert lender.cancel() == N.ZK_OK
        assert lender.finish_status() == N.ZK_ERR_ARG
        N.check(lender.enqueue(g1.limbs("rm1")))
        s.check("borrower of a cancelled lender", borrower.finish(), g2.expect("A"))
        s.check("lender at once after its cancel", lender.finish(), g1.expect("rm1"))
        # cancel the borrower; the lender finishes, runs again, and shares again
        N.check(lender.enqueue(g1.limbs("C")))
        N.check(borrower.enqueue_shared(lender))
        assert borrower.cancel() == N.ZK_OK
        assert borrower.finish_status() == N.ZK_ERR_ARG
        s.check("lender of a cancelled borrower", lender.finish(), g1.expect("C"))
        s.check("lender again", lender.run(g1.limbs("D")), g1.expect("D"))
        N.check(lender.enqueue(g1.limbs("B")))
        N.check(borrower.enqueue_shared(lender))
        s.check("lender, shared again", lender.finish(), g1.expect("B"))
        s.check("borrower, shared again", borrower.finish(), g2.expect("B"))
        # the borrower on its own afterwards: its lists are its own again
        s.check("borrower alone", borrower.run(g2.limbs("same")), g2.expect("same"))
        s.settle()
    finally:
        lender.destroy()
        borrower.destroy()


# ---- 3. borrowing from a lender that has only sorted -----------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,n", SHARED, ids=SHARED_IDS)
def test_borrowing_the_sort_of_a_lender_that_has_only_sorted(gpu, flags, n):
    g1, g2, g2s = case(0, 1, n), case(0, 2, n), case(0, 2, 64)
    lender, borrower, other = Plan(gpu, g1, flags), Plan(gpu, g2, flags), Plan(gpu, g2s, flags)
    s = Steps()
    try:
        # a borrower of another size is refused after export_sort has marked the lender as lent: nobody records ev_release, and
        # the lender's next run, which waits for it, must neither stall nor go wrong
        N.check(lender.enqueue_sort(g1.limbs("A")))
        assert other.enqueue_shared(lender) == N.ZK_ERR_ARG
        N.check(lender.enqueue_rest())
        s.check("lender of a refused borrower", lender.finish(), g1.expect("A"))
        s.check("lender's next run", lender.run(g1.limbs("B")), g1.expect("B"))
        s.check("refused borrower alone", other.run(g2s.limbs("A")), g2s.expect("A"))
        # twice in a row with other scalars: sorted_ready (ws.ev_acc0) and ws.seg_len are phase 1's
        for tag in ("C", "rm1"):
            N.check(lender.enqueue_sort(g1.limbs(tag)))
            N.check(borrower.enqueue_shared(lender))
            N.check(lender.enqueue_rest())
            s.check(f"lender {tag}", lender.finish(), g1.expect(tag))
            s.check(f"borrower {tag}", borrower.finish(), g2.expect(tag))
        # a shorter vector the same way (the borrower takes q_m from the lender), then each plan alone
        N.check(lender.enqueue_sort(g1.limbs("D"), m=n - 3))
        N.check(borrower.enqueue_shared(lender))
        N.check(lender.enqueue_rest(borrower.h))           # the lender's accumulate kernel behind the borrower's
        s.check("borrower, shorter", borrower.finish(), g2.expect("D", n - 3))
        s.check("lender, shorter", lender.finish(), g1.expect("D", n - 3))
        s.check("borrower alone", borrower.run(g2.limbs("E")), g2.expect("E"))
        s.check("lender alone", lender.run(g1.limbs("E")), g1.expect("E"))
        s.settle()
    finally:
        for p in (lender, borrower, other):
            p.destroy()


# ---- 4. zk_msm_plan_wait_event -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", MODES, ids=MODE_IDS)
def test_wait_event_orders_the_plan_behind_an_upload_on_another_stream(gpu, flags):
    """the device buffer holds A; B arrives by an asynchronous upload from page-locked memory behind a spin of a few milliseconds
    on a second, non-blocking stream.  The event is the one Groth16.prove passes on: zk_qap_uv_dev's, recorded on that stream
    (here with no transform in front of it).  Without the wait the run reads A: another valid point."""
    cs = case(0, 1, N_SMALL)
    p = Plan(gpu, cs, flags)
    st = S.new_stream(gpu)
    try:
        staged = S.Staged(cs.limbs("A"), cs.limbs("B"))
        assert (cs.expect("A") != cs.expect("B")).any()
        assert (p.run(staged.ptr, dev=True) == cs.expect("A")).all()      # also takes the first-launch costs off the timed part
        N.check(gpu.zk_debug_spin_dev(st, 1))
        S.sync(gpu, st)
        N.check(gpu.zk_debug_spin_dev(st, 5000))
        staged.send(gpu, st)
        ev = N._vp()
        N.check(gpu.zk_qap_uv_dev(0, 4, None, None, st, ctypes.byref(ev)))
        assert ev.value
        N.check(gpu.zk_msm_plan_wait_event(p.h, ev))
        got = p.run(staged.ptr, dev=True)
        S.sync(gpu, st)
        assert (got == cs.expect("B")).all(), "reads the buffer's earlier content" if (got == cs.expect("A")).all() else "differs from both"
        assert gpu.zk_msm_plan_wait_event(p.h, None) == N.ZK_ERR_ARG      # null event
        N.check(gpu.zk_msm_plan_wait_event(p.h, ev))                       # a completed event: the next run does not stall
        assert (p.run(cs.limbs("C")) == cs.expect("C")).all()
    finally:
        h = p.h
        p.destroy()
        N.check(gpu.zk_stream_destroy(st))
    assert gpu.zk_msm_plan_wait_event(h, ev) == N.ZK_ERR_ARG              # unknown handle


# ---- 5. through the Python layer ---------------------------------------------------------------------------------------------------------
def test_point_array_plan_over_calls_of_other_lengths_and_release_with_a_run_in_flight(gpu):
    from zksnake_amd._algebra import PointArray
    from zksnake_amd.ecc import EllipticCurve
    cs = case(0, 1, N_SMALL)
    n = cs.n
    curve = EllipticCurve("BN254")
    arr = PointArray(0, 1, cs.bases)

    def known(h):
        c, nw = N._i(0), N._i(0)
        return gpu.zk_msm_plan_windows(h, c, nw) == N.ZK_OK

    def run(h, tag):
        out = np.zeros(cs.words, dtype=np.uint64)
        N.check(gpu.zk_msm_plan_run(h, n, cs.limbs(tag).ctypes.data, 0, 0, 0, N.u64p(out), None))
        return out

    h = arr.plan()
    for tag, m in (("A", n), ("B", 700), ("C", 1), ("D", n)):
        got = curve.multiexp(arr, cs.limbs(tag)[:m])
        assert (got._limbs == cs.expect(tag, m)).all(), (tag, m)
        assert arr.plan() == h                                           # the same plan served them all
    arr.release()
    assert not arr._plans and not arr._plan_layout and not known(h)
    # release() with a whole run, and with a sort only, left enqueued: _drop cancels before it destroys
    h0 = arr.plan(0, precompute=True)
    h1 = arr.plan(1, precompute=True)
    N.check(gpu.zk_msm_plan_enqueue(h0, n, cs.limbs("A").ctypes.data, 0, 0, 0, N.STREAM_PLAN))
    N.check(gpu.zk_msm_plan_enqueue_sort(h1, n, cs.limbs("B").ctypes.data, 0, 0, 0, N.STREAM_PLAN))
    arr.release()
    assert not arr._plans and not arr._plan_concurrent and not known(h0) and not known(h1)
    assert gpu.zk_msm_plan_finish(h0, N.u64p(np.zeros(cs.words, dtype=np.uint64))) == N.ZK_ERR_ARG
    # the same slots again: new plans (handle values are never reused), the oracle's points
    n0, n1 = arr.plan(0, precompute=True), arr.plan(1, precompute=True)
    assert len({h, h0, h1, n0, n1}) == 5
    assert (run(n0, "C") == cs.expect("C")).all() and (run(n1, "rm1") == cs.expect("rm1")).all()
    arr.release()
    assert not known(n0) and not known(n1)
