// msm_impl.hip.h -- Pippenger bucket multi-scalar multiplication over G1/G2 of BN254 and BLS12-381 on
// gfx950, plus batched scalar multiplication.
//
// Stands in for multiscalar_mul_g1/_g2 (reference src/bn254/curve.rs:356-392,
// src/bls12_381/curve.rs:366-402 -> ark-ec 0.4.2 VariableBaseMSM::msm) and
// batch_multi_scalar_g1/_g2 (src/bn254/curve.rs:326-354).  The result of an MSM is a single
// group element, returned as its unique affine representative, so any correct bucket method
// is bit-identical with the reference's.
//
// Pipeline (one stream, no host round trip until the tail); stages 1-4 do not depend on the group and live in MsmFront
// (msm_front.h, compiled once in msm_front.hip), stages 5-8 are MsmPlan<G>'s below.  The plan holds the buffers, the options and the
// state of a run; each stage's kernels and launchers (msm_accumulate.hip.h, msm_reduce.hip.h), the reduction geometry
// (msm_reduce_plan.h) and the host tail (msm_host_tail.h) are written once in their own headers, where the stage tests call them too:
//   1. digits      scalar -> signed c-bit window digits (bias trick: s + sum 2^(c-1) 2^(wc),
//                  then plain bit fields), 2 B per (window, scalar), coalesced.
//   2. histogram   one workgroup per (window, chunk): 2^(c-1) counters live in LDS (128 KiB at
//                  c = 16), LDS atomics only; the table is flushed with coalesced stores.
//   3. prefix/scan per-bucket prefix over chunks, bucket offsets, segment offsets.
//   4. scatter     same grid as 2: LDS cursors, point references written bucket-sorted.
//   5. accumulate  THE dominant kernel: one lane per bucket *segment* (<= S entries, so skewed
//                  scalar distributions cannot starve a wave), XYZZ accumulator in registers,
//                  bases gathered as whole 64..192-byte rows.
//   6. combine     per-bucket sum of its segment partials.
//   7. reduce      sum_b (b+1) B_b through the split b = hi*C + lo: wave-per-row / wave-per-column
//                  sums (shuffle trees), then a log-depth suffix-scan on <=256 points per array.
//   8. host tail   3 points per window come back; Horner over windows and the affine
//                  conversion (one inversion) run on the host -- a lone GPU wave needs ~1.3 us per
//                  field multiplication, the host ~50 ns.
#pragma once
#include <algorithm>
#include <chrono>
#include <memory>
#include <vector>
#include "common.hip.h"
#include "msm_plan.h"
#include "pair.hip.h"
#include "setup_impl.hip.h"
#include "codec.hip.h"
#include "glv_params.h"

#include "msm_common.hip.h"
#include "msm_accumulate.hip.h"
#include "msm_reduce.hip.h"
#include "msm_host_tail.h"

namespace zkmi {
using mem::DevBuf;

#if defined(ZK_GROUP) && (!defined(ZK_PART) || ZK_PART == 0)
// the plan's translation unit does not instantiate the heavy kernels (see msm_group.hip)
extern template __global__ void accumulate_kernel<ZK_GROUP>(const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t*, uint32_t*);
extern template __global__ void accumulate_split_kernel<ZK_GROUP>(const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t*, uint32_t*);   // instantiated for the Fp2 groups (msm_group.hip)
extern template __global__ void bases_to_mont_kernel<ZK_GROUP>(const uint32_t*, uint64_t, uint32_t*, int);
extern template __global__ void combine_kernel<ZK_GROUP>(const uint32_t*, const uint32_t*, uint32_t, uint32_t, const uint32_t*, const uint32_t*, uint32_t*);
extern template __global__ void strided_sum_kernel<ZK_GROUP>(const uint32_t*, uint32_t*, SumJob, SumJob, uint32_t);
extern template __global__ void weighted_sum_kernel<ZK_GROUP>(const uint32_t*, uint32_t, uint32_t, const uint32_t*, uint32_t, uint32_t*);
ZK_SETUP_EXTERN_TEMPLATES(ZK_GROUP)
ZK_CODEC_EXTERN_TEMPLATES(ZK_GROUP)
#endif

#if !defined(ZK_PART) || ZK_PART == 0
// ---- host: plan --------------------------------------------------------------------------------------

// ZK_MSM_PRECOMPUTE: table row k = 2^(c (w_first + k)) * P_i (affine, Montgomery) for the w_count windows of the plan; on
// entry row 0 holds the bases themselves.  With these rows every window adds into ONE shared bucket set: the bucket
// reduction and the host tail shrink by the number of windows and the Horner pass disappears.  The chain of doublings
// runs in XYZZ on a scratch vector; each row is normalised with the batched inversion (one Fermat inversion per 1024
// points instead of one per point and row: 46 -> ~15 ms for a 2^20-point BN254 G1 key).
template <class G>
static int precompute_table(uint32_t* table, uint64_t n, int c, int w_first, int w_count) {
    typedef typename G::F F;
    constexpr int AW = 2 * F::LIMBS, XW = 4 * F::LIMBS;
    if (w_first == 0 && w_count == 1) return ZK_OK;
    DevBuf temp_buf;
    ZK_HIP_RC(temp_buf.alloc(n * XW * 4));
    uint32_t* const temp = temp_buf.as();
    const unsigned blocks = (unsigned)((n + 255) / 256);
    const unsigned nblocks = (unsigned)((n + (uint64_t)NORM_THREADS * NORM_E - 1) / ((uint64_t)NORM_THREADS * NORM_E));
    hipLaunchKernelGGL(dbl_rows_kernel<G>, dim3(blocks), dim3(256), 0, 0, temp, n, c * w_first, (const uint32_t*)table);
    if (w_first > 0) hipLaunchKernelGGL(normalize_kernel<G>, dim3(nblocks), dim3(NORM_THREADS), 0, 0, temp, n, table, 0);
    for (int k = 1; k < w_count; ++k) {
        hipLaunchKernelGGL(dbl_rows_kernel<G>, dim3(blocks), dim3(256), 0, 0, temp, n, c, (const uint32_t*)nullptr);
        hipLaunchKernelGGL(normalize_kernel<G>, dim3(nblocks), dim3(NORM_THREADS), 0, 0, temp, n, table + (size_t)k * n * AW, 0);
    }
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipDeviceSynchronize());
    return ZK_OK;
}

// fixed-base table of the last broadcast base of this group (Groth16.setup multiplies the same generator five times)
template <class G>
struct FixedTable {
    std::vector<uint64_t> base;   // canonical affine limbs the table was built for
    DevBuf d_table;
    int nwin = 0;
    std::mutex mu;
    // never destroyed: the table goes back through release() (zk_shutdown) only, and nothing runs at process exit, when the
    // allocator's maps or the HIP runtime may already be gone
    static FixedTable& get() {
        static FixedTable* const t = new FixedTable();
        return *t;
    }
    void release() {
        std::lock_guard<std::mutex> lock(mu);
        d_table.reset();
        base.clear();
    }
    // caller holds mu
    int ensure(const uint64_t* base_limbs) {
        typedef typename G::F F;
        typedef typename G::Fr FrP;
        constexpr int AW = 2 * F::LIMBS, XW = 4 * F::LIMBS;
        const size_t words64 = AW / 2;
        if (d_table && base.size() == words64 && memcmp(base.data(), base_limbs, words64 * 8) == 0) return ZK_OK;
        d_table.reset();
        base.clear();
        nwin = (FrP::BITS + 1 + FIXED_C - 1) / FIXED_C;
        // window bases 2^(16 j) G on the host (16 points)
        std::vector<uint32_t> wb((size_t)nwin * AW);
        {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(base_limbs);
            Affine<F> g = {F::from_canonical(w), F::from_canonical(w + F::LIMBS)};
            XYZZ<F> acc = xyzz_from_affine<F>(g);
            for (int j = 0; j < nwin; ++j) {
                Affine<F> a = xyzz_to_affine<F>(acc);
                F::store(wb.data() + (size_t)j * AW, a.x);
                F::store(wb.data() + (size_t)j * AW + F::LIMBS, a.y);
                if (j + 1 < nwin) for (int k = 0; k < FIXED_C; ++k) acc = xyzz_dbl<F>(acc);
            }
        }
        const uint64_t rows = (uint64_t)nwin * FIXED_HALF;
        DevBuf table, d_wb, temp;  // the table becomes the member once it is complete
        ZK_HIP_RC(table.alloc(rows * AW * 4));
        ZK_HIP_RC(d_wb.alloc(wb.size() * 4));
        ZK_HIP_RC(temp.alloc(rows * XW * 4));
        ZK_HIP(hipMemcpy(d_wb.as(), wb.data(), wb.size() * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(fixed_table_kernel<G>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, 0, d_wb.as(), nwin, temp.as());
        hipLaunchKernelGGL(normalize_kernel<G>, dim3((unsigned)((rows + (uint64_t)NORM_THREADS * NORM_E - 1) / ((uint64_t)NORM_THREADS * NORM_E))),
                           dim3(NORM_THREADS), 0, 0, temp.as(), rows, table.as(), 0);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipDeviceSynchronize());
        d_table = std::move(table);
        base.assign(base_limbs, base_limbs + words64);
        return ZK_OK;
    }
};

template <class G>
struct MsmPlan : MsmPlanBase {
    typedef typename G::F F;
    typedef typename G::Fr FrP;
    static constexpr int AW = 2 * F::LIMBS;
    static constexpr int XW = 4 * F::LIMBS;
    static constexpr uint64_t SEG_TARGET_LANES = 256ull * 1024;  // 4 waves per SIMD on 256 CUs
    static constexpr int MAX_C = 20;           // widest window (fixed-base plans; digits are then 32-bit)
    bool wide = false;                         // c > 16: 32-bit digits, two-level sort only
    enum class Phase { All, SortOnly, Rest };     // what one call of run_stages puts on the stream
    enum class Run { Idle, Sorted, Pending };     // Sorted: enqueue_sort done, enqueue_rest still to come; Pending: finish() to come

    // device workspace of one run (stages 5..7; the sort's is the front's)
    struct Work {
        DevBuf partials, buckets, rows, fin;
        DevBuf parts;  // partial row / column sums of the two-step strided sums
        // A recorded event costs ~3 us of idle GPU between two kernels (tools/event_gap_probe.hip), so a run records only the four
        // that order work or bound a stage: ev_start (plan), ev_acc0 = sorted (also the lender's "sorted_ready"), ev_acc1 =
        // accumulated (the gate of the next plan's accumulate kernel), ev_end (plan); ev_accs only when the accumulate kernel
        // waits for something after the sort (a gate, or the second half of a two-step enqueue)
        hipEvent_t ev_acc0 = nullptr, ev_accs = nullptr, ev_acc1 = nullptr;
        bool acc_from_accs = false;
        hipEvent_t ev_release = nullptr;  // recorded by a borrower of this run's sort (enqueue_shared) after its last read
        bool lent = false;
        uint32_t seg_len = 0;
        int w_first = 0, w_count = 0;  // windows of the run in flight
        uint32_t groups = 0;           // bucket sets of the run in flight
    };

    uint64_t n = 0;      // entries per window (2 n_api with the endomorphism)
    uint64_t n_api = 0;  // points of the plan as the caller counts them
    bool glv = false;    // general G1 plan over (P_i, phi(P_i)) with half-length scalars
    bool pre = false;  // ZK_MSM_PRECOMPUTE: shared bucket set over a table of 2^(c w) P_i
    int pw_first = 0, pw_count = 0;  // windows this plan can run (a sharded rank's share; all of them by default)
    ReduceShape shape;               // buckets per set as rows x columns, weighted-sum blocks (msm_reduce_plan.h)
    Work ws;
    MsmFront front;  // stages 1-4: scalars -> digits -> sorted entry list
    // shared device buffers
    std::shared_ptr<DevBuf> bases_block;  // the (table of) bases: shared by the clones of a plan
    uint32_t* d_bases = nullptr;
    uint32_t* h_final = nullptr;  // pinned: (S, T) per weighted-sum block
    hipEvent_t ev_start = nullptr, ev_end = nullptr;

    ~MsmPlan() override {
        // the blocks of ws, front and bases_block go back to the caching allocator after this body, and that (unlike hipFree)
        // does not wait for the device: make sure no run of this plan is still in flight
        (void)hipDeviceSynchronize();
        pinned_free_cached(h_final);
        for (hipEvent_t e : {ws.ev_acc0, ws.ev_accs, ws.ev_acc1, ws.ev_release, ev_start, ev_end}) if (e) (void)hipEventDestroy(e);
        stream_release((create_flags & ZK_MSM_HIGH_PRIORITY) != 0, own_stream);
    }

    // Every allocation lands in a member that the destructor frees, and the factory deletes the plan when init() fails
    // (msm_group.hip), so a failing hipMalloc half way through leaks nothing.
    // `share` != nullptr: a clone -- same bases (and fixed-base table), own workspace and stream
    int init(uint64_t n_points, const void* bases, int bases_on_device, int flags, int window_bits, int win_first, int win_count,
             const MsmPlan* share = nullptr) {
        const bool trace = opt.trace_init;
        auto t_prev = std::chrono::steady_clock::now();
        auto mark = [&](const char* what) {
            if (!trace) return;
            auto now = std::chrono::steady_clock::now();
            fprintf(stderr, "[plan init] %-24s %8.1f us\n", what, std::chrono::duration<double, std::micro>(now - t_prev).count());
            t_prev = now;
        };
        create_flags = flags;
        seg_lanes_at_init = opt.segment_lanes ? opt.segment_lanes : SEG_TARGET_LANES;
        pre = (flags & ZK_MSM_PRECOMPUTE) != 0;
        if (n_points == 0 || n_points > (1ull << 26)) return fail(ZK_ERR_ARG, "MSM size must be in [1, 2^26]");
        const MsmLayout lay = msm_layout(FrP::BITS, GlvOf<G>::OK, n_points, flags, window_bits, win_count <= 0);
        glv = share ? share->glv : lay.glv;
        n_api = n_points;
        n = glv ? 2 * n_points : n_points;  // entries per window: the kernels see an MSM over (P_i, phi(P_i)) pairs
        entries_per_window = n;
        c = lay.c;
        if (c < 2 || c > MAX_C) return fail(ZK_ERR_ARG, "window bits must be in [2, 20]");
        if (c > 16 && !pre) return fail(ZK_ERR_ARG, "windows wider than 16 bits need a fixed-base plan (ZK_MSM_PRECOMPUTE)");
        wide = c > 16;
        nwin = glv ? glv_window_count(c) : window_count(FrP::BITS + 1, c);
        if (win_count <= 0) { win_first = 0; win_count = nwin; }
        if (win_first < 0 || win_first + win_count > nwin) return fail(ZK_ERR_ARG, "window range out of bounds");
        pw_first = win_first;
        pw_count = win_count;
        if (!reduce_shape(c, wide, &shape)) return fail(ZK_ERR_ARG, "window too wide for the reduction stage");
        const uint64_t entries = (uint64_t)pw_count * n;
        if (entries > 0x7FFFFFFFull) return fail(ZK_ERR_ARG, "MSM too large");

        ZK_HIP_RC(stream_acquire((flags & ZK_MSM_HIGH_PRIORITY) != 0, &own_stream));
        if (share) {
            bases_block = share->bases_block;
            d_bases = share->d_bases;
        } else {
            bases_block = std::make_shared<DevBuf>();
            ZK_HIP_RC(bases_block->alloc((pre ? (uint64_t)pw_count : 1ull) * n * AW * 4));
            d_bases = bases_block->as();
            if (bases_on_device) {
                launch_bases_to_mont<G>((const uint32_t*)bases, n_api, d_bases, glv ? 1 : 0, nullptr);
            } else {
                DevBuf tmp;
                ZK_HIP_RC(tmp.alloc(n_api * AW * 4));
                ZK_HIP(hipMemcpy(tmp.as(), bases, n_api * AW * 4, hipMemcpyHostToDevice));
                launch_bases_to_mont<G>(tmp.as(), n_api, d_bases, glv ? 1 : 0, nullptr);
                ZK_HIP(hipDeviceSynchronize());
            }
            ZK_HIP(hipGetLastError());
            if (pre) {
                // rows 2^(c w) P_i for the windows of this plan only (a sharded rank never builds the other ranks' rows)
                int rc = precompute_table<G>(d_bases, n, c, pw_first, pw_count);
                if (rc) return rc;
            }
        }
        mark("stream + bases");
        {
            FrontLayout fl;
            fl.c = c; fl.B = shape.B; fl.n = n; fl.n_api = n_api; fl.pre = pre; fl.wide = wide; fl.glv = glv ? &GlvOf<G>::P::K : nullptr;
            fl.pw_first = pw_first; fl.pw_count = pw_count; fl.nwin = nwin; fl.curve = G::CURVE;
            ZK_HIP_RC(front.init(fl, &opt));
        }
        const uint64_t max_sets = pre ? 1ull : (uint64_t)pw_count;
        ZK_HIP_RC(pinned_alloc_cached((void**)&h_final, (size_t)max_sets * shape.blocks() * 2 * XW * 4));
        mark("scalars/digits/pinned");
        ZK_HIP(hipEventCreateWithFlags(&ev_start, hipEventDisableSystemFence));   // timing only: nothing synchronises with it
        ZK_HIP(hipEventCreate(&ev_end));
        {
            const uint64_t keys = max_sets * shape.B;
            // a window-range run picks its own (shorter) segments: at most SEG_TARGET_LANES of them, or entries / 8
            const uint32_t seg_full = pick_seg_len(entries);
            const uint64_t max_segs = std::max<uint64_t>(entries / seg_full, std::min<uint64_t>(entries / 8, seg_lanes_at_init)) + keys + 8;
            ZK_HIP_RC(front.alloc_workspace());
            ZK_HIP_RC(ws.partials.alloc(max_segs * XW * 4));
            ZK_HIP_RC(ws.buckets.alloc(keys * XW * 4));
            ZK_HIP_RC(ws.rows.alloc(max_sets * (shape.R + shape.C) * XW * 4));
            if (reduce_parts_per_set(shape)) ZK_HIP_RC(ws.parts.alloc(max_sets * reduce_parts_per_set(shape) * XW * 4));
            ZK_HIP_RC(ws.fin.alloc(max_sets * shape.blocks() * 2 * XW * 4));
            for (hipEvent_t* e : {&ws.ev_acc0, &ws.ev_accs, &ws.ev_acc1, &ws.ev_release}) ZK_HIP(hipEventCreate(e));
        }
        mark("workspace + events");
        // LDS above 64 KiB needs the opt-in
        ZK_HIP_RC(front.set_kernel_attributes());
        ZK_HIP(weighted_sum_set_attributes<G>());
        mark("func attributes");
        ZK_HIP(hipDeviceSynchronize());
        mark("device sync");
        return ZK_OK;
    }

    // Segment length for a run over `entries` sorted entries: aim at >= 4 waves per SIMD worth of lanes (a window-range
    // run of a sharded MSM has far fewer entries than the plan's full set; with the plan-wide length its lanes would
    // be too few and each would walk 64 additions at lone-wave speed).
    uint32_t pick_seg_len(uint64_t entries) const {
        const uint64_t target = opt.segment_lanes ? opt.segment_lanes : SEG_TARGET_LANES;
        uint64_t sl = (entries + target - 1) / target;
        if (sl < 8) sl = 8;
        if (sl > 64) sl = 64;
        if (pre) {
            // shared bucket set: keep a bucket within ~12 runs so that one lane pair can combine it
            uint64_t per_bucket = entries / shape.B;
            uint64_t want = (per_bucket + 11) / 12;
            if (want > sl) sl = want;
            if (sl > 1024) sl = 1024;
        }
        return (uint32_t)sl;
    }

    // ---- the stages of one run after the front's, for the windows [ws.w_first, ws.w_first + ws.w_count) on stream st -----------

    // the pair-split accumulate kernel (Fp2 groups) or the one-lane one: the plan's option, else the group's default
    bool split_pairs_on() const {
        if constexpr (AccumulateSplit<G>::ON) return opt.split_pairs < 0 ? AccumulateSplit<G>::DEFAULT : opt.split_pairs != 0;
        return false;
    }

    // stage 5: the dominant kernel; stage 6: buckets whose entries span several segments (three tiers, one launch)
    int stage_accumulate(uint32_t m, const SortedView& sv, hipStream_t st, bool prio_steps) {
        Work& l = ws;
        const uint32_t n_keys = l.groups * shape.B;
        const uint64_t lanes_needed = ((uint64_t)l.w_count * m + sv.seg_len - 1) / sv.seg_len;
        launch_accumulate<G>(split_pairs_on(), lanes_needed, d_bases, sv.sorted, sv.bstart, sv.sstart, n_keys, sv.seg_len, prio_steps ? 1u : 0u,
                             l.partials.as(), l.buckets.as(), st);
        ZK_HIP(hipEventRecord(l.ev_acc1, st));
        launch_combine<G>(l.partials.as(), sv.sstart, n_keys, sv.big_list, sv.big_count, l.buckets.as(), st);
        ZK_HIP(hipGetLastError());
        return ZK_OK;
    }

    // stage 7: sum_b (b + 1) B_b per bucket set down to (S, T) per block of row / column sums, copied to h_final
    int stage_reduce(hipStream_t st) {
        Work& l = ws;
        const uint32_t groups = l.groups;
        const ReducePlan plan = reduce_plan(shape, groups, opt.sum_one_step, opt.lanes_per_output);
        uint32_t* const row_sums = l.rows.as();
        const uint32_t* in = l.buckets.as();
        for (int k = 0; k < plan.steps; ++k) {
            uint32_t* const out = k + 1 < plan.steps ? l.parts.as() : row_sums;
            launch_strided_sum<G>(in, out, plan.step[k].rows, plan.step[k].cols, plan.step[k].lpo, st);
            in = out;
        }
        launch_weighted_sum<G>(row_sums, shape.R, groups, row_sums + (size_t)groups * shape.R * XW, shape.C, l.fin.as(), st);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpyAsync(h_final, l.fin.as(), (size_t)groups * shape.blocks() * 2 * XW * 4, hipMemcpyDeviceToHost, st));
        return ZK_OK;
    }

    // stages 2..7 + D2H
    // `borrowed`: the digits and the sort of another plan's run over the same scalars (enqueue_shared); stages 1-4 are skipped
    // phase: All, SortOnly = up to the sorted entry list only, Rest = from the accumulate kernel on (after SortOnly).
    // gate: waited for right before the accumulate kernel (another plan's accumulate has finished), so that the
    // accumulate kernels of several plans run one after the other while their sorts and reductions overlap.
    int run_stages(uint32_t m, uint32_t dstride, hipStream_t st, const SortExport* borrowed = nullptr, Phase phase = Phase::All, hipEvent_t gate = nullptr) {
        Work& l = ws;
        int rc;
        const uint32_t seg_len = borrowed ? borrowed->view.seg_len : (phase == Phase::Rest ? l.seg_len : pick_seg_len((uint64_t)l.w_count * m));
        l.seg_len = seg_len;
        if (phase == Phase::Rest) {
            // sorted by the SortOnly half
        } else if (borrowed) {
            ZK_HIP(hipStreamWaitEvent(st, borrowed->sorted_ready, 0));
        } else if ((rc = front.sort(m, dstride, seg_len, l.w_first, l.w_count, l.groups, st))) {
            return rc;
        }
        const SortedView sv = borrowed ? borrowed->view : front.view();
        if (phase != Phase::Rest) ZK_HIP(hipEventRecord(l.ev_acc0, st));
        if (phase == Phase::SortOnly) return ZK_OK;
        if (gate) ZK_HIP(hipStreamWaitEvent(st, gate, 0));
        l.acc_from_accs = gate != nullptr || phase == Phase::Rest;
        if (l.acc_from_accs) ZK_HIP(hipEventRecord(l.ev_accs, st));
        // priority steps (msm_accumulate.hip.h) for a run in one piece that waits for nothing: the two-step, gated and shared forms
        // are what a prover uses to overlap several plans
        const bool prio_steps = opt.priority_steps && phase == Phase::All && !gate && !borrowed;
        if ((rc = stage_accumulate(m, sv, st, prio_steps))) return rc;
        if (borrowed) ZK_HIP(hipEventRecord(borrowed->release, st));  // the lender's buffers are no longer read
        return stage_reduce(st);   // the caller records ev_end
    }

    int set_option(const char* name, int64_t value) override {
        std::lock_guard<std::mutex> lock(mu);
        if (in_flight()) return fail(ZK_ERR_ARG, "MSM plan has a run in flight: options change between runs");
        if (!strcmp(name, "segment_lanes")) {
            if (value < 64) return fail(ZK_ERR_ARG, "segment_lanes must be at least 64");
            // the partials buffer was sized for the creation-time target: more lanes than that would overrun it
            if ((uint64_t)value > seg_lanes_at_init) return fail(ZK_ERR_ARG, "segment_lanes cannot exceed the value the plan was created with");
            opt.segment_lanes = (uint64_t)value;
        } else if (!strcmp(name, "sum_one_step")) {
            opt.sum_one_step = value != 0;
        } else if (!strcmp(name, "lanes_per_output")) {
            if (value != 0 && (value < 2 || value > 64 || (value & (value - 1)))) return fail(ZK_ERR_ARG, "lanes_per_output: 0 or a power of two in [2, 64]");
            opt.lanes_per_output = (uint32_t)value;
        } else if (!strcmp(name, "priority_steps")) {
            opt.priority_steps = value != 0;
        } else if (!strcmp(name, "split_pairs")) {
            if (value < -1 || value > 1) return fail(ZK_ERR_ARG, "split_pairs: -1 (the group's default), 0 or 1");
            if (value == 1 && !AccumulateSplit<G>::ON) return fail(ZK_ERR_ARG, "split_pairs: this group has no pair-split accumulate kernel (base-field groups)");
            opt.split_pairs = (int)value;
        } else if (!strcmp(name, "two_level_sort")) {
            if (value && !front.has_two_level_buffers()) return fail(ZK_ERR_ARG, "the plan was created without the buffers of the two-level sort");
            if (!value && wide) return fail(ZK_ERR_ARG, "windows wider than 16 bits exist in the two-level sort only");
            opt.two_level_sort = value != 0;
        } else {
            return fail(ZK_ERR_ARG, std::string("unknown or creation-time MSM option: ") + name);
        }
        return ZK_OK;
    }

    int debug_view(uint64_t* out, int cap) override {
        std::lock_guard<std::mutex> lock(mu);
        if (in_flight()) return fail(ZK_ERR_ARG, "MSM plan has a run in flight: the view is read between runs");
        if (!out || cap < ZK_MSM_VIEW_SLOTS) return fail(ZK_ERR_ARG, "zk_msm_plan_debug_view needs room for ZK_MSM_VIEW_SLOTS values");
        const SortedView own = front.view();
        const uint64_t v[ZK_MSM_VIEW_SLOTS] = {
            (uint64_t)(uintptr_t)front.digits_buf(), (uint64_t)(uintptr_t)d_bases, (uint64_t)(uintptr_t)own.sorted, (uint64_t)(uintptr_t)own.bstart,
            (uint64_t)(uintptr_t)own.sstart, (uint64_t)(uintptr_t)own.big_list, (uint64_t)(uintptr_t)own.big_count,
            (uint64_t)(uintptr_t)ws.partials.as(), (uint64_t)(uintptr_t)ws.buckets.as(),
            n, n_api, (uint64_t)c, (uint64_t)nwin, shape.B, glv ? 1u : 0u, pre ? 1u : 0u, wide ? 1u : 0u, (uint64_t)pw_first, (uint64_t)pw_count,
            (uint64_t)ws.w_first, (uint64_t)ws.w_count, ws.groups, ws.seg_len, q_m, front.view_dstride,
            (uint64_t)front.view_route, (uint64_t)front.view_fine_log, front.view_split_fine() ? 1u : 0u, split_pairs_on() ? 1u : 0u};
        for (int k = 0; k < ZK_MSM_VIEW_SLOTS; ++k) out[k] = v[k];
        return ZK_OK;
    }

    uint64_t seg_lanes_at_init = 0;
    int create_flags = 0;
    int clone(MsmPlanBase** out) override {
        MsmPlan* p = new MsmPlan();
        p->opt = opt;
        int rc = p->init(n_api, nullptr, 0, create_flags & ~ZK_MSM_HIGH_PRIORITY, c, pw_first, pw_count, this);
        if (rc) {
            delete p;
            return rc;
        }
        *out = p;
        return ZK_OK;
    }

    // state carried from enqueue() to finish()
    Run q_state = Run::Idle;
    int q_first = 0, q_count = 0;
    uint32_t q_m = 0;
    hipStream_t q_stream = nullptr;
    bool in_flight() const { return q_state != Run::Idle; }

    // The prologue of every run (caller holds mu, arguments checked): one run at a time; a borrower of the previous run's sort may
    // still be reading the buffers this run overwrites; note the run; scalars from the host go to the device; ev_start.
    // m = entries per window (0: an empty run puts nothing but the wait on the stream), groups = bucket sets
    int begin_run(hipStream_t st, int w_first, int w_count, uint32_t m, uint32_t groups, const void* host_scalars = nullptr, size_t scalar_bytes = 0) {
        if (in_flight()) return fail(ZK_ERR_ARG, "MSM plan already has a run in flight: call zk_msm_plan_finish first");
        q_first = w_first; q_count = w_count; q_m = m; q_stream = st;
        if (ws.lent) {
            ZK_HIP(hipStreamWaitEvent(st, ws.ev_release, 0));
            ws.lent = false;
        }
        if (m == 0) return ZK_OK;
        if (host_scalars) ZK_HIP(hipMemcpyAsync(front.scalars_buf(), host_scalars, scalar_bytes, hipMemcpyHostToDevice, st));
        ZK_HIP(hipEventRecord(ev_start, st));
        ws.w_first = w_first;
        ws.w_count = w_count;
        ws.groups = groups;
        return ZK_OK;
    }

    int enqueue(uint64_t n_scalars, const void* scalars, int on_device, int w_first, int w_count, hipStream_t st) override {
        return enqueue_phase(n_scalars, scalars, on_device, w_first, w_count, st, Phase::All);
    }
    int enqueue_sort(uint64_t n_scalars, const void* scalars, int on_device, int w_first, int w_count, hipStream_t st) override {
        return enqueue_phase(n_scalars, scalars, on_device, w_first, w_count, st, Phase::SortOnly);
    }
    hipEvent_t accumulate_done_event() override { return ws.ev_acc1; }
    int enqueue_rest(MsmPlanBase* after) override {
        std::lock_guard<std::mutex> lock(mu);
        if (q_state != Run::Sorted) return fail(ZK_ERR_ARG, "zk_msm_plan_enqueue_rest without zk_msm_plan_enqueue_sort");
        q_state = Run::Idle;
        if (q_m > 0) {
            int rc = run_stages(q_m, (q_m + 7u) & ~7u, q_stream, nullptr, Phase::Rest, after ? after->accumulate_done_event() : nullptr);
            if (rc) return rc;
            ZK_HIP(hipEventRecord(ev_end, q_stream));
        }
        q_state = Run::Pending;
        return ZK_OK;
    }

    int enqueue_phase(uint64_t n_scalars, const void* scalars, int on_device, int w_first, int w_count, hipStream_t st, Phase phase) {
        std::lock_guard<std::mutex> lock(mu);
        if (n_scalars > n_api) return fail(ZK_ERR_LENGTH, "Number of points and scalars mismatch");
        if (w_count <= 0) { w_first = pw_first; w_count = pw_count; }
        if (w_first < pw_first || w_first + w_count > pw_first + pw_count)
            return fail(ZK_ERR_ARG, "window range out of bounds (the plan was created for windows [" + std::to_string(pw_first) + ", " +
                                        std::to_string(pw_first + pw_count) + "))");
        const uint32_t m_api = (uint32_t)n_scalars;
        const uint32_t m = glv ? 2 * m_api : m_api;  // entries per window
        int rc = begin_run(st, w_first, w_count, m, pre ? 1u : (uint32_t)w_count, on_device ? nullptr : scalars, (size_t)m_api * FrP::W * 4);
        if (rc) return rc;
        if (m > 0) {
            const uint32_t* sc = on_device ? (const uint32_t*)scalars : front.scalars_buf();
            if ((rc = front.digits(sc, m_api, w_first, w_count, st))) return rc;  // 1. the windows of this run
            if ((rc = run_stages(m, (m + 7u) & ~7u, st, nullptr, phase))) return rc;
            if (phase == Phase::All) ZK_HIP(hipEventRecord(ev_end, st));
        }
        q_state = phase == Phase::SortOnly ? Run::Sorted : Run::Pending;
        return ZK_OK;
    }

    int cancel() override {
        std::lock_guard<std::mutex> lock(mu);
        if (in_flight() && q_stream) ZK_HIP(hipStreamSynchronize(q_stream));
        q_state = Run::Idle;
        return ZK_OK;
    }

    int export_sort(SortExport* out) override {
        std::lock_guard<std::mutex> lock(mu);
        if (!in_flight() || q_m == 0) return fail(ZK_ERR_ARG, "the lending plan has no run in flight");
        out->view = front.view();
        out->view.seg_len = ws.seg_len;
        out->n = n; out->m = q_m; out->groups = ws.groups;
        out->c = c; out->nwin = nwin; out->w_first = q_first; out->w_count = q_count;
        out->pw_first = pw_first; out->pw_count = pw_count; out->scalar_bits = FrP::BITS; out->pre = pre; out->glv = glv;
        out->endo = glv ? G::ENDO_ID : 0;
        out->sorted_ready = ws.ev_acc0;
        out->release = ws.ev_release;
        ws.lent = true;
        return ZK_OK;
    }

    // Run this plan on the digits and the sorted entry list of `lender`'s run in flight: same scalars, other bases
    // (Groth16's <tau_1, v> and <tau_2, v>).  Both plans must have the same size, window layout, mode and window range;
    // the entry list addresses points (or table rows) by index, which is independent of the group.
    int enqueue_shared(MsmPlanBase* lender, hipStream_t st) override {
        SortExport ex;
        int rc = lender->export_sort(&ex);
        if (rc) return rc;
        std::lock_guard<std::mutex> lock(mu);
        if (ex.n != n || ex.c != c || ex.nwin != nwin || ex.pre != pre || ex.glv != glv || ex.endo != (glv ? G::ENDO_ID : 0) || ex.scalar_bits != FrP::BITS ||
            ex.pw_first != pw_first || ex.pw_count != pw_count)
            return fail(ZK_ERR_ARG, "plans differ in size, window layout or mode: the sort cannot be shared");
        if ((rc = begin_run(st, ex.w_first, ex.w_count, ex.m, ex.groups))) return rc;   // ex.m > 0: export_sort lends no empty run
        if ((rc = run_stages(ex.m, (ex.m + 7u) & ~7u, st, &ex))) return rc;
        ZK_HIP(hipEventRecord(ev_end, st));
        q_state = Run::Pending;
        return ZK_OK;
    }

    int finish(uint64_t* out) override {
        std::lock_guard<std::mutex> lock(mu);
        if (q_state == Run::Sorted) return fail(ZK_ERR_ARG, "zk_msm_plan_finish before zk_msm_plan_enqueue_rest");
        if (q_state != Run::Pending) return fail(ZK_ERR_ARG, "zk_msm_plan_finish without a pending run");
        q_state = Run::Idle;
        if (q_m > 0) ZK_HIP(hipEventSynchronize(ev_end));
        // 8. the tail runs on the host: its time comes from the host's clock (an event recorded and awaited here would put a
        // GPU round trip of 10-20 us on the critical path of every MSM just to time it)
        const auto tail_t0 = std::chrono::steady_clock::now();
        int rc = msm_host_tail<G>(h_final, q_m > 0 ? ws.groups : 0u, shape, c, q_first, pre, out);   // no bucket set: the empty MSM, infinity
        if (rc || q_m == 0) return rc;
        timings[3] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - tail_t0).count();
        auto elapsed = [](hipEvent_t from, hipEvent_t to) {
            float t = 0;
            return hipEventElapsedTime(&t, from, to) == hipSuccess ? t : 0.0f;
        };
        timings[0] = elapsed(ev_start, ws.ev_acc0);                                     // digits + sort
        timings[1] = elapsed(ws.acc_from_accs ? ws.ev_accs : ws.ev_acc0, ws.ev_acc1);   // accumulate kernel
        timings[2] = elapsed(ws.ev_acc1, ev_end);                                       // combine + reduction + D2H
        float t = 0;
        timings[4] = hipEventElapsedTime(&t, ev_start, ev_end) == hipSuccess ? t + timings[3] : 0.0f;
        return ZK_OK;
    }
};

// batch_multi_scalar_g1/_g2: out[i] = k_i * P_i (canonical affine).  One base for many scalars (what Groth16.setup
// does) goes through the fixed-base table: <= 16 mixed additions per scalar; everything ends in the batched normalisation.
constexpr uint64_t FIXED_BASE_MIN = 2048;  // below this the table (2^19 rows) costs more than it saves

template <class G>
static int batch_mul_impl(uint64_t n, const uint64_t* scalars, const uint64_t* bases, int broadcast, uint64_t* out) {
    typedef typename G::F F;
    typedef typename G::Fr FrP;
    constexpr int AW = 2 * F::LIMBS, XW = 4 * F::LIMBS;
    if (n == 0) return ZK_OK;
    DevBuf ds, db, dout, temp;
    const bool fixed = broadcast && n >= FIXED_BASE_MIN;
    uint64_t nb = broadcast ? 1 : n;
    ZK_HIP_RC(ds.alloc(n * FrP::W * 4));
    ZK_HIP_RC(temp.alloc(n * XW * 4));
    ZK_HIP_RC(dout.alloc(n * AW * 4));
    ZK_HIP(hipMemcpy(ds.as(), scalars, n * FrP::W * 4, hipMemcpyHostToDevice));
    if (fixed) {
        FixedTable<G>& ft = FixedTable<G>::get();
        std::lock_guard<std::mutex> lock(ft.mu);
        ZK_HIP_RC(ft.ensure(bases));
        FixedBias bias;
        memset(&bias, 0, sizeof(bias));
        for (int j = 0; j < ft.nwin; ++j) {
            int bit = j * FIXED_C + (FIXED_C - 1);
            bias.v[bit >> 5] |= 1u << (bit & 31);
        }
        hipLaunchKernelGGL(fixed_mul_kernel<G>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ds.as(), n, ft.d_table.as(), ft.nwin, bias, temp.as());
        ZK_HIP(hipDeviceSynchronize());
    } else {
        ZK_HIP_RC(db.alloc(nb * AW * 4));
        ZK_HIP(hipMemcpy(db.as(), bases, nb * AW * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(varbase_mul_kernel<G>, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, 0, ds.as(), db.as(), broadcast, n, temp.as());
    }
    hipLaunchKernelGGL(normalize_kernel<G>, dim3((unsigned)((n + (uint64_t)NORM_THREADS * NORM_E - 1) / ((uint64_t)NORM_THREADS * NORM_E))),
                       dim3(NORM_THREADS), 0, 0, temp.as(), n, dout.as(), 1);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpy(out, dout.as(), n * AW * 4, hipMemcpyDeviceToHost));
    return ZK_OK;
}

// batched (de)compression of n points between host buffers: `to_bytes` != 0 encodes canonical affine rows, 0 decodes.
// On a failing point the first one (lowest index) decides the error, as a sequential loop over the file would.
template <class G>
static int codec_impl(uint64_t n, const void* in, void* out, int to_bytes, uint64_t* bad_index) {
    typedef typename G::F F;
    constexpr size_t ROW = (size_t)2 * F::LIMBS * 4, ENC = CodecLayout<G>::TOTAL;
    if (n == 0) return ZK_OK;
    const size_t in_bytes = n * (to_bytes ? ROW : ENC), out_bytes = n * (to_bytes ? ENC : ROW);
    DevBuf din, dout, derr;
    ZK_HIP_RC(din.alloc(in_bytes));
    ZK_HIP_RC(dout.alloc(out_bytes));
    ZK_HIP_RC(derr.alloc(8));
    unsigned long long first = ~0ull;
    ZK_HIP(hipMemcpy(din.as(), in, in_bytes, hipMemcpyHostToDevice));
    ZK_HIP(hipMemcpy(derr.as(), &first, 8, hipMemcpyHostToDevice));
    const dim3 grid((unsigned)((n + 127) / 128)), block(128);
    if (to_bytes) hipLaunchKernelGGL(points_encode_kernel<G>, grid, block, 0, 0, din.as<const uint32_t>(), n, dout.as<uint8_t>(), derr.as<unsigned long long>());
    else hipLaunchKernelGGL(points_decode_kernel<G>, grid, block, 0, 0, din.as<const uint8_t>(), n, dout.as(), derr.as<unsigned long long>());
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpy(&first, derr.as(), 8, hipMemcpyDeviceToHost));
    if (first != ~0ull) {
        if (bad_index) *bad_index = (uint64_t)(first >> 8);
        return fail(ZK_ERR_POINT, codec_message((int)(first & 0xFF)));
    }
    ZK_HIP(hipMemcpy(out, dout.as(), out_bytes, hipMemcpyDeviceToHost));
    return ZK_OK;
}


#endif  // ZK_PART == 0

}  // namespace zkmi
