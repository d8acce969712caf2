"""The MSM bucket reduction stage by stage: tests/native/reduce_stages.hip runs pair_add (csrc/pair.hip.h) and sp_add_affine
(csrc/fp2_split.hip.h) on raw register-form records, one lane PAIR per record, and launches the production kernels of
csrc/msm_reduce.hip.h (combine_kernel, strided_sum_kernel, weighted_sum_kernel) on arrays built here, through the launchers of that
header (launch_combine, launch_strided_sum, launch_weighted_sum) that MsmPlan calls, so with the plan's own grids.  References are
plain integers (tests/reduce_model.py): add-2008-s / dbl-2008-s-1 on Montgomery representatives for the additions, sums of known
multiples of the generator (held against chains of pyref additions on the CPU) for the kernels.  No tolerance: exact integers.

Contracts checked here (p the base field's modulus, per component for the Fp2 groups; "norm" = every limb but the top one < 2^29):

  code                    input contract                                          promised output                          test
  pair_add                X < 4p, Y / ZZ / ZZZ < 2p, norm; ZZ = 0 <=> ZZZ = 0      add-2008-s, X < 4p, rest < 2p, norm;      test_pair_add_*
                          (0 and p both count as zero: half_is_inf uses           P = Q -> dbl-2008-s-1 of P; P = -Q ->
                          F::is_zero on the lane's ZZ or ZZZ); both lanes of a    zeros; an infinite operand -> the other
                          pair in the same control flow                           operand unchanged (limb for limb)
  xyzz_dbl via pair_add   G1: X < 4p unreduced (only products meet it);           dbl-2008-s-1, all < 2p                    test_pair_add_* (double)
                          G2: X reduced below 2p by pair_add first
  sp_add_affine           as xyzz_add_affine_relaxed2 (X < 4p, rest and base      limb-equal to xyzz_add_affine_mem after   test_split_step
                          < 2p), the lane's component of every value              the finishing reduction of X; madd-2008-s
  strided_sum_kernel      rows in memory form, X < 4p, rest < 2p, ZZ = 0 for      out[o] = sum_j in[index(o, j)], same      test_strided_sum
                          infinity; every SumJob index inside the input           ranges; rows outside the jobs untouched
  weighted_sum_kernel     the same rows; m0, m1 >= 1                              (S, T) per block of 128: S = sum j X_j    test_weighted_sum
                                                                                  with LOCAL j, T = sum X_j; same ranges
  combine_kernel          run_start monotone; big_list / big_count by the rule    bucket = sum of its runs; no run ->       test_combine
                          of the run-offset scan (17..2048 runs from the front,   zeros; ONE run -> row left untouched
                          more from the back)                                     (accumulate wrote it); same ranges

The third branch of pair_add (neither RELAXED nor RELAXED2) is instantiated by no group and is NOT covered here (see the comment
there).  The model, the index expressions and the profile builders have CPU tests below (no gpu marker)."""

import ctypes
import os
import random

import numpy as np
import pytest

import reduce_model as M
from reduce_model import GROUPS, KINDS, Pool, SumJob
from test_field_edges import ROOT, StepRef, check_step, step_inputs, step_record, unpack_acc

SRC = os.path.join(ROOT, "tests", "native", "reduce_stages.hip")
G2_GROUPS = [G for G in GROUPS if G.d == 2]
gid = lambda G: G.name  # noqa: E731


# ---- CPU: the reference side ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GROUPS, ids=gid)
def test_model_pair_add_against_pyref(G):
    """the integer model of pair_add / the XYZZ doubling against pyref.Group.add / mul on curve points in random representatives:
    ordinary sums, P = Q, P = -Q, the cube-root-of-unity pairs (same y, other x), infinity on either side"""
    rnd = random.Random(5 + G.gid)
    pts = M.real_points(G, 12, 100 + G.gid)
    seen = set()
    for (a, _), (b, _) in zip(pts, pts[1:]):
        P, Q = G.xyzz(a, rnd), G.xyzz(b, rnd)
        branch, e = G.ref.pair_add(P, Q)
        seen.add(branch)
        assert branch == "ordinary" and G.to_affine(e) == G.g.add(a, b)
        d = G.ref.dbl(P)
        assert G.to_affine(d) == G.g.mul(a, 2) == G.g.add(a, a)
    for P, Q, want in M.pair_add_records(G, 7 + G.gid, n_ordinary=50, n_special=6):
        branch, e = G.ref.pair_add(P, Q)
        seen.add(branch)
        if want is None:
            continue
        assert branch == want
        a, b = G.to_affine(P), G.to_affine(Q)
        assert G.g.is_on_curve(a) and G.g.is_on_curve(b)
        got = {"P": a, "Q": b}.get(e) if isinstance(e, str) else (None if e is None else G.to_affine(e))
        assert got == G.g.add(a, b), want
        if want == "r_zero_only":
            assert a[1] == b[1] and a[0] != b[0]
    assert seen == set(M.PairRef.BRANCHES)


def test_sum_job_index_against_enumeration():
    """SumJob.index with the job shapes of reduce_plan (csrc/msm_reduce_plan.h) against the definition: row r of bucket set g sums buckets g B + r C + [0, C),
    column c sums g B + [0, R) C + c; the two-step form reaches the same buckets through its partial sums"""
    for groups, R, C in ((1, 4, 8), (3, 8, 4), (2, 5, 3), (2, 8, 16)):
        Bk = R * C
        rows, cols = M.one_step_jobs(groups, R, C)
        want_rows = [sorted(g * Bk + r * C + c for c in range(C)) for g in range(groups) for r in range(R)]
        want_cols = [sorted(g * Bk + r * C + c for r in range(R)) for g in range(groups) for c in range(C)]
        assert [sorted(t) for t in M.job_terms(rows)] == want_rows and [sorted(t) for t in M.job_terms(cols)] == want_cols
        assert rows.max_index() == cols.max_index() == groups * Bk - 1
        assert cols.out_offset == rows.n_out
        for K in (2, 4):
            if C % K or R % K or C // K < 2 or R // K < 2:
                continue
            (prow, pcol), (frow, fcol), lpo2 = M.two_step_jobs(groups, R, C, K)
            parts = {}
            for job in (prow, pcol):
                for o, t in enumerate(M.job_terms(job)):
                    assert job.out_offset + o not in parts
                    parts[job.out_offset + o] = t
            assert sorted(parts) == list(range(prow.n_out + pcol.n_out))
            for job, want in ((frow, want_rows), (fcol, want_cols)):
                got = [sorted(b for i in t for b in parts[i]) for t in M.job_terms(job)]
                assert got == want
            assert max(prow.max_index(), pcol.max_index()) == groups * Bk - 1
            assert max(frow.max_index(), fcol.max_index()) == prow.n_out + pcol.n_out - 1
            assert lpo2 >= 2 and lpo2 & (lpo2 - 1) == 0


def test_combine_profile_against_tier_rule():
    counts = [0, 1, 2, 16, 17, 32, 33, 2048, 2049, 5000, 0, 1, 3]
    run_start, big_list, big_count = M.combine_profile(counts)
    assert [M.tier_of(c) for c in counts] == ["empty", "single", "small", "small", "wave", "wave", "wave", "wave", "big", "big", "empty", "single", "small"]
    assert int(run_start[-1]) == sum(counts) and all(int(run_start[k + 1] - run_start[k]) == c for k, c in enumerate(counts))
    assert list(big_count) == [4, 2]
    assert sorted(big_list[:4]) == [4, 5, 6, 7] and sorted(big_list[len(counts) - 2:]) == [8, 9]
    for key in big_list[:4]:
        assert M.COMBINE_SMALL_MAX < counts[key] <= M.COMBINE_WAVE_MAX
    for key in big_list[len(counts) - 2:]:
        assert counts[key] > M.COMBINE_WAVE_MAX


@pytest.mark.parametrize("G", GROUPS, ids=gid)
def test_pool_expected_against_addition(G):
    """the pools' logarithms are those of their points, and the closed-form sums equal chains of pyref additions"""
    for k, kind in enumerate(KINDS):
        pool = Pool(G, kind, 300 + 10 * G.gid + k, size=12)
        for aff, a, pt in zip(pool.affine, pool.scalar, pool.points):
            assert G.mul_gen(a) == aff == G.to_affine(pt) and G.g.is_on_curve(aff)
            G.check_row_range(pt)
            assert G.unrow(G.row(pt)) == pt
            if kind == "x_high":
                assert all(v >= 2 * G.p for v in pt[0])
        idx = pool.draw(9, 1)
        assert pool.expected(idx) == pool.expected_by_addition(idx)
        w = list(range(len(idx)))
        assert pool.expected(idx, w) == pool.expected_by_addition(idx, w)
    pool = Pool(G, "all_equal", 400 + G.gid)
    m = 9
    idx = pool.draw(m, 2)
    assert pool.expected(idx, range(m)) == G.g.mul(pool.affine[0], m * (m - 1) // 2) and pool.expected(idx) == G.g.mul(pool.affine[0], m)
    assert Pool(G, "alternating", 401 + G.gid).expected(pool.draw(10, 3) * 0 + np.arange(10) % 2) is None


# ---- the device harness ---------------------------------------------------------------------------------------------------------------
class Stages:
    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        for name in ("rs_pair_add", "rs_split_step", "rs_lane_step"):
            getattr(lib, name).restype = ci
            getattr(lib, name).argtypes = [ci, u64, vp, vp]
        lib.rs_strided_sum.restype = ci
        lib.rs_strided_sum.argtypes = [ci, vp, u64, vp, u64, vp, vp, u32]
        lib.rs_weighted_sum.restype = ci
        lib.rs_weighted_sum.argtypes = [ci, vp, u32, u32, vp, u32, vp]
        lib.rs_combine.restype = ci
        lib.rs_combine.argtypes = [ci, vp, u64, vp, u32, vp, vp, vp]
        lib.rs_constants.restype = None
        lib.rs_constants.argtypes = [vp]
        c = np.zeros(6, dtype=np.uint32)
        lib.rs_constants(c.ctypes.data)
        assert list(c) == [M.COMBINE_SMALL_MAX, M.COMBINE_WAVE_MAX, M.COMBINE_WAVE_BLOCKS, M.COMBINE_BIG_BLOCKS, M.COMBINE_THREADS, M.WS_BLOCK]

    def pair_add(self, G, recs):
        arr = np.array([G.regs(P) + G.regs(Q) for P, Q in recs], dtype=np.uint32)
        out = np.zeros((len(recs), 4 * G.REGS), dtype=np.uint32)
        rc = self.lib.rs_pair_add(G.gid, len(recs), arr.ctypes.data, out.ctypes.data)
        assert rc == 0, f"rs_pair_add({G}) returned {rc}"
        return out

    def step(self, G, arr, lanes):
        arr = np.ascontiguousarray(arr, dtype=np.uint32)
        out = np.zeros((arr.shape[0], 8 * G.f.N), dtype=np.uint32)
        rc = (self.lib.rs_split_step if lanes == 2 else self.lib.rs_lane_step)(G.gid, arr.shape[0], arr.ctypes.data, out.ctypes.data)
        assert rc == 0, rc
        return out

    def strided_sum(self, G, rows, out, j0, j1, lpo):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        # every index the kernel forms stays inside the arrays it is given
        assert max(j0.max_index(), j1.max_index()) < rows.shape[0]
        assert max(j.out_offset + j.n_out for j in (j0, j1) if j.n_out) <= out.shape[0]
        w0, w1 = j0.words(), j1.words()
        rc = self.lib.rs_strided_sum(G.gid, rows.ctypes.data, rows.shape[0], out.ctypes.data, out.shape[0], w0.ctypes.data, w1.ctypes.data, lpo)
        assert rc == 0, f"rs_strided_sum({G}) returned {rc}"

    def weighted_sum(self, G, in0, m0, n0, in1, m1):
        in0, in1 = np.ascontiguousarray(in0, dtype=np.uint32), np.ascontiguousarray(in1, dtype=np.uint32)
        assert in0.shape == (n0 * m0, G.XW) and in1.shape == (n0 * m1, G.XW)    # the kernel reads n0 arrays from each input
        out = np.full((len(M.weighted_blocks(m0, n0, m1)) * 2, G.XW), 0xA5A5A5A5, dtype=np.uint32)
        rc = self.lib.rs_weighted_sum(G.gid, in0.ctypes.data, m0, n0, in1.ctypes.data, m1, out.ctypes.data)
        assert rc == 0, rc
        return out

    def combine(self, G, partials, run_start, big_list, big_count, buckets):
        partials = np.ascontiguousarray(partials, dtype=np.uint32)
        n_keys = len(run_start) - 1
        assert int(run_start[-1]) == partials.shape[0] and (np.diff(run_start.astype(np.int64)) >= 0).all()
        assert buckets.shape == (n_keys, G.XW) and len(big_list) == n_keys and int(big_count.sum()) <= n_keys
        assert all(int(k) < n_keys for k in big_list[:int(big_count[0])]) and all(int(k) < n_keys for k in big_list[n_keys - int(big_count[1]):])
        rc = self.lib.rs_combine(G.gid, partials.ctypes.data, partials.shape[0], run_start.ctypes.data, n_keys, big_list.ctypes.data,
                                 big_count.ctypes.data, buckets.ctypes.data)
        assert rc == 0, rc


def build_stages(d):
    """the harness through the library's own pipeline, as the device fixture of test_field_edges.py does; ZKMI_STAGES_LIB names an
    already built one (kernel-variant experiments)"""
    from helpers import build_device_harness
    return build_device_harness(SRC, d, "ZKMI_STAGES_LIB")


@pytest.fixture(scope="module")
def stages(tmp_path_factory, gpu):
    return Stages(build_stages(tmp_path_factory.mktemp("rs_dev")))


def run_pair_records(stages, G, recs, counts):
    out = stages.pair_add(G, [(P, Q) for P, Q, _ in recs])
    res = []
    for i, (P, Q, want) in enumerate(recs):
        try:
            branch, got = M.check_pair_add(G, P, Q, out[i])
            assert want is None or branch == want, f"built for {want}, the integers say {branch}"
        except AssertionError as e:
            raise AssertionError(f"{G} pair_add record {i} (wave {i // 32}, pair {i % 32}): P {P} Q {Q} out {[hex(int(x)) for x in out[i]]}: {e}") from None
        counts[branch] = counts.get(branch, 0) + 1
        res.append(got)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("G", GROUPS, ids=gid)
def test_pair_add_records(stages, G):
    """every branch of pair_add, 32 records per wave each on its own branch (shuffled), then one wave where every pair doubles and
    one where exactly one does; the branch of every record is taken from the integers and every branch must have been met"""
    recs = M.pair_add_records(G, 40 + G.gid)
    random.Random(41 + G.gid).shuffle(recs)
    counts = {}
    run_pair_records(stages, G, recs, counts)
    assert all(counts.get(b, 0) > 0 for b in M.PairRef.BRANCHES), counts
    all_dbl, one_dbl = M.wave_layouts(G, 50 + G.gid)
    for layout in (all_dbl, one_dbl, all_dbl + one_dbl):
        c2 = {}
        run_pair_records(stages, G, layout, c2)
        assert c2["double"] == sum(1 for r in layout if r[2] == "double")


@pytest.mark.gpu
@pytest.mark.parametrize("G", GROUPS, ids=gid)
def test_pair_add_chains(stages, G):
    """64 chains of 24 additions, each output fed back in as the left operand.  At steps 11 and 17 the addend is the running sum
    itself in another representative (a repeat of the previous addend would not meet the running sum: only the sum itself makes
    P = Q), at step 13 its negative: doublings and cancellations on relaxed-range intermediates, then a chain that restarts from
    infinity.  The affine value of every chain is followed with pyref."""
    rnd = random.Random(60 + G.gid)
    chains = 64
    pts = M.real_points(G, 64, 61 + G.gid)
    accs = [((0,) * G.d,) * 4 for _ in range(chains)]
    affs = [None] * chains
    counts = {}
    for step in range(24):
        recs, adds = [], []
        for c in range(chains):
            if step in (11, 17):
                Q, a = M.disguise(G, accs[c], rnd), affs[c]
            elif step == 13:
                Q, a = M.disguise(G, G.neg_pt(accs[c]), rnd), G.g.neg(affs[c])
            else:
                a = pts[(c * 7 + step * 13) % 64][0]
                Q = G.xyzz(a, rnd)
            recs.append((accs[c], Q, {11: "double", 17: "double", 13: "cancel"}.get(step)))
            adds.append(a)
        accs = run_pair_records(stages, G, recs, counts)
        for c in range(chains):
            affs[c] = G.g.add(affs[c], adds[c])
            assert G.to_affine(accs[c]) == affs[c], (step, c)
    assert counts["double"] == 2 * chains and counts["cancel"] == chains and counts["left_inf"] >= chains and counts["ordinary"] > 0


def step_branch(f, d, case):
    """the branch of the bucket step, from the integers (the order of sp_add_affine's tests)"""
    acc, x, y, neg = case
    if all(c == 0 for c in x + y):
        return "sentinel"
    if all(c == 0 for c in acc[2]):
        return "empty"
    e = StepRef(f, d)
    yy = tuple((-c) % f.p for c in y) if neg else y
    if e.zero(e.sub(e.mul(x, acc[2]), acc[0])):
        return "double" if e.zero(e.sub(e.mul(yy, acc[3]), acc[1])) else "cancel"
    return "ordinary"


@pytest.mark.gpu
@pytest.mark.parametrize("G", G2_GROUPS, ids=gid)
def test_split_step(stages, G):
    """sp_add_affine on a lane pair: the records of the one-lane bucket step (test_field_edges.step_inputs), against the StepRef
    integers and limb for limb against xyzz_add_affine_mem after the finishing reduction of X (fp_reduce_2p)"""
    f, d = G.f, 2
    cases = step_inputs(f, d, 70 + G.gid, n=640)
    random.Random(71).shuffle(cases)
    arr = np.stack([step_record(f, d, *c) for c in cases])
    pair, lane = stages.step(G, arr, 2), stages.step(G, arr, 1)
    counts = {}
    finish = lambda a: (tuple(v - 2 * f.p if v >= 2 * f.p else v for v in a[0]),) + a[1:]  # noqa: E731
    for i, c in enumerate(cases):
        try:
            got = check_step(f, d, c, pair[i])
            assert finish(got) == finish(unpack_acc(f, d, lane[i])), "differs from the one-lane step"
        except AssertionError as e:
            raise AssertionError(f"{G} sp_add_affine case {i} ({c}): {e}") from None
        b = step_branch(f, d, c)
        counts[b] = counts.get(b, 0) + 1
    assert all(counts.get(b, 0) > 0 for b in ("ordinary", "double", "cancel", "empty", "sentinel")), counts
    # chains of 24 steps through the pair form, each output fed back in
    rnd = random.Random(72 + G.gid)
    accs = [((0,) * d,) * 4 for _ in range(64)]
    last = [None] * 64
    for step in range(24):
        ins = []
        for c in range(64):
            x, y = tuple(M.rand_below(rnd, 2 * f.p) for _ in range(d)), tuple(M.rand_below(rnd, 2 * f.p) for _ in range(d))
            if step in (11, 17):
                x, y = last[c]
            neg = rnd.random() < 0.5
            if step == 13:
                (x, y), neg = last[c], not ins_prev[c][3]
            last[c] = (x, y)
            ins.append((accs[c], x, y, neg))
        out = stages.step(G, np.stack([step_record(f, d, *c) for c in ins]), 2)
        ref = stages.step(G, np.stack([step_record(f, d, *c) for c in ins]), 1)
        for c in range(64):
            accs[c] = check_step(f, d, ins[c], out[c])
            assert finish(accs[c]) == finish(unpack_acc(f, d, ref[c])), (step, c)
        ins_prev = ins


# ---- strided_sum_kernel ----------------------------------------------------------------------------------------------------------------
def _sentinel_rows(G, n):
    return np.full((n, G.XW), 0xA5A5A5A5, dtype=np.uint32)


def _check_outputs(G, pool, idx, out, job, label):
    for o, terms in enumerate(M.job_terms(job)):
        try:
            M.check_out_row(G, out[job.out_offset + o], pool.expected(idx[terms]))
        except AssertionError as e:
            raise AssertionError(f"{G} {pool.kind} {label}: output {o} of the job at offset {job.out_offset} (terms {terms[:6]}..): {e}") from None


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("G", GROUPS, ids=gid)
def test_strided_sum(stages, G, kind):
    """the production strided_sum_kernel at the job shapes of stage_reduce: one-step rows + columns at every lanes-per-output
    (term counts below / equal to / not a multiple of lpo / 2, last waves with dead groups), a launch whose second job is empty,
    and the two-step form (split / outer2, then in_offset) chained through memory"""
    pool = Pool(G, kind, 500 + 10 * G.gid + KINDS.index(kind))
    for groups, R, C in ((1, 4, 8), (3, 8, 4), (2, 5, 3)):
        idx = pool.draw(groups * R * C, 3 * R + C)
        rows_in = pool.rows[idx]
        rows, cols = M.one_step_jobs(groups, R, C)
        for lpo in (2, 4, 8, 16, 32, 64):
            out = _sentinel_rows(G, rows.n_out + cols.n_out + 1)
            stages.strided_sum(G, rows_in, out, rows, cols, lpo)
            _check_outputs(G, pool, idx, out, rows, f"rows {groups}x{R}x{C} lpo {lpo}")
            _check_outputs(G, pool, idx, out, cols, f"cols {groups}x{R}x{C} lpo {lpo}")
            assert (out[-1] == 0xA5A5A5A5).all(), "a row outside the jobs was written"
        # j1.n_out = 0: only the rows
        out = _sentinel_rows(G, rows.n_out + cols.n_out)
        stages.strided_sum(G, rows_in, out, rows, SumJob(0, 1, 0, 0, 0, 1, 0), 8)
        _check_outputs(G, pool, idx, out, rows, "rows only")
        assert (out[rows.n_out:] == 0xA5A5A5A5).all()
    for groups, R, C, K in ((1, 8, 8, 2), (2, 8, 16, 4)):
        idx = pool.draw(groups * R * C, 5 * R + K)
        (prow, pcol), (frow, fcol), lpo2 = M.two_step_jobs(groups, R, C, K)
        parts = _sentinel_rows(G, prow.n_out + pcol.n_out)
        stages.strided_sum(G, pool.rows[idx], parts, prow, pcol, 2)
        _check_outputs(G, pool, idx, parts, prow, "prow")
        _check_outputs(G, pool, idx, parts, pcol, "pcol")
        out = _sentinel_rows(G, frow.n_out + fcol.n_out)
        stages.strided_sum(G, parts, out, frow, fcol, lpo2)
        rows, cols = M.one_step_jobs(groups, R, C)
        _check_outputs(G, pool, idx, out, rows, f"two-step rows lpo2 {lpo2}")
        _check_outputs(G, pool, idx, out, cols, f"two-step cols lpo2 {lpo2}")


# ---- weighted_sum_kernel ---------------------------------------------------------------------------------------------------------------
WS_SIZES = (1, 2, 3, 127, 128, 129, 255, 256, 300)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("G", GROUPS, ids=gid)
def test_weighted_sum(stages, G, kind):
    """the production weighted_sum_kernel: (S, T) per block of 128 points with LOCAL weights, arrays of in0 first; every size of
    WS_SIZES as m0 and as m1, n0 in {1, 3}"""
    pool = Pool(G, kind, 600 + 10 * G.gid + KINDS.index(kind))
    for k, m0 in enumerate(WS_SIZES):
        m1 = WS_SIZES[(k + 4) % len(WS_SIZES)]
        n0 = 1 if k % 2 else 3
        i0, i1 = pool.draw(n0 * m0, 11 * k), pool.draw(n0 * m1, 11 * k + 1)
        out = stages.weighted_sum(G, pool.rows[i0], m0, n0, pool.rows[i1], m1)
        blocks = M.weighted_blocks(m0, n0, m1)
        assert out.shape[0] == 2 * len(blocks)
        for b, (which, a, first, length) in enumerate(blocks):
            src, m = (i0, m0) if which == 0 else (i1, m1)
            terms = src[a * m + first:a * m + first + length]
            try:
                M.check_out_row(G, out[2 * b], pool.expected(terms, range(length)))
                M.check_out_row(G, out[2 * b + 1], pool.expected(terms))
                if kind == "all_equal":
                    P = pool.affine[0]
                    assert G.to_affine(G.unrow(out[2 * b])) == G.g.mul(P, length * (length - 1) // 2)
                    assert G.to_affine(G.unrow(out[2 * b + 1])) == G.g.mul(P, length)
            except AssertionError as e:
                raise AssertionError(f"{G} {kind} m0 {m0} m1 {m1} n0 {n0} block {b} (input {which}, array {a}, points {first}+{length}): {e}") from None


# ---- combine_kernel --------------------------------------------------------------------------------------------------------------------
TIER_PROFILE = [0, 1, 2, 16, 17, 32, 33, 2048, 2049, 5000, 0, 1, 3, 16, 17]
# more wave-tier buckets than the COMBINE_WAVE_BLOCKS * 4 waves and more workgroup-tier buckets than COMBINE_BIG_BLOCKS workgroups:
# both striding loops take a second turn
STRIDE_PROFILE = [17, 0, 1, 2] * 515 + [2049] * (M.COMBINE_BIG_BLOCKS + 3) + [18] * 5


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("random", "all_equal", "alternating", "mostly_inf"))
@pytest.mark.parametrize("G", GROUPS, ids=gid)
def test_combine(stages, G, kind):
    """the production combine_kernel: buckets in every tier and on every tier boundary; a bucket with one run is left untouched
    (the row is pre-filled with a sentinel point), one without runs becomes infinity"""
    pool = Pool(G, kind, 700 + 10 * G.gid + KINDS.index(kind))
    sentinel = np.array(G.row(G.xyzz(M.real_points(G, 1, 9)[0][0], random.Random(1))), dtype=np.uint32)
    assert sum(1 for c in STRIDE_PROFILE if M.tier_of(c) == "wave") > M.COMBINE_WAVE_BLOCKS * M.COMBINE_THREADS // 64
    assert sum(1 for c in STRIDE_PROFILE if M.tier_of(c) == "big") > M.COMBINE_BIG_BLOCKS
    # the small tier's own boundary: with nothing listed, buckets of more than COMBINE_SMALL_MAX runs are nobody's and keep the sentinel
    counts = [M.COMBINE_SMALL_MAX + 1, M.COMBINE_WAVE_MAX + 1, M.COMBINE_SMALL_MAX]
    run_start, big_list, _ = M.combine_profile(counts)
    idx = pool.draw(int(run_start[-1]), 99)
    buckets = np.tile(sentinel, (len(counts), 1))
    stages.combine(G, pool.rows[idx], run_start, big_list, np.zeros(2, dtype=np.uint32), buckets)
    assert (buckets[0] == sentinel).all() and (buckets[1] == sentinel).all(), "the small tier took a bucket above its limit"
    M.check_out_row(G, buckets[2], pool.expected(idx[int(run_start[2]):]))
    for name, counts in (("tiers", TIER_PROFILE), ("stride", STRIDE_PROFILE)):
        run_start, big_list, big_count = M.combine_profile(counts)
        idx = pool.draw(int(run_start[-1]), len(counts))
        buckets = np.tile(sentinel, (len(counts), 1))
        stages.combine(G, pool.rows[idx], run_start, big_list, big_count, buckets)
        sc = np.array(pool.scalar, dtype=np.int64)[idx]
        for key, c in enumerate(counts):
            s0 = int(run_start[key])
            try:
                if c == 1:
                    assert (buckets[key] == sentinel).all(), "a bucket with one run must be left untouched"
                    continue
                if c == 0:
                    assert not buckets[key].any(), "an empty bucket is written as zeros"
                M.check_out_row(G, buckets[key], G.mul_gen(int(sc[s0:s0 + c].sum())))
            except AssertionError as e:
                raise AssertionError(f"{G} {kind} profile {name}: key {key} with {c} runs ({M.tier_of(c)} tier): {e}") from None
