// msm_reduce_plan.h -- the geometry of the MSM bucket reduction (stage 7, msm_reduce.hip.h): how a set of 2^(c-1) buckets is cut
// into R rows of C columns, and the strided-sum jobs that add them up in one launch or in two.  Plain C++, no HIP include:
// MsmPlan (msm_impl.hip.h) sizes its buffers and launches from it, tests/native/reduce_plan_check.cpp prints it and
// tests/test_host_lib.py compares that with the integer model of the stage tests (tests/reduce_model.py).
#pragma once
#include <algorithm>
#include <cstdint>

namespace zkmi {

// weighted_sum_kernel works on blocks of at most WS_BLOCK row (or column) sums
constexpr int WS_BLOCK = 128;
constexpr int WS_BLOCK_LOG = 7;

// Bucket b = hi * C + lo of a set: sum_b (b + 1) B_b = C sum_hi hi Row_hi + sum_lo lo Col_lo + sum_b B_b
struct ReduceShape {
    uint32_t B = 0, R = 0, C = 0;  // buckets per set, rows, columns
    uint32_t bpr = 0, bpc = 0;     // weighted-sum blocks per row array / per column array
    uint32_t blocks() const { return bpr + bpc; }
};

// false when the window is too wide for the reduction stage (more than 1024 rows or columns)
inline bool reduce_shape(int c, bool wide, ReduceShape* out) {
    ReduceShape s;
    s.B = 1u << (c - 1);
    int rl = (c - 1 + 1) / 2;
    if (rl > 8 && !wide) rl = 8;
    s.R = 1u << rl;
    s.C = s.B / s.R;
    if (s.C > 1024 || s.R > 1024) return false;
    s.bpr = (s.R + WS_BLOCK - 1) / WS_BLOCK;
    s.bpc = (s.C + WS_BLOCK - 1) / WS_BLOCK;
    *out = s;
    return true;
}

// buckets one lane pair adds up in the first step of the two-step strided sums (0 = one step)
inline uint32_t sum_part_len(const ReduceShape& s) {
    const uint32_t k = 16u;
    return (s.R >= 4 * k && s.C >= 4 * k) ? k : 0u;
}

// One strided sum of strided_sum_kernel:
//   out[o] = sum_{j < count} in[(o / per_group) * group_stride + (o % per_group) * outer + j * inner]
struct SumJob {
    uint32_t n_out, per_group, group_stride, outer, inner, count;
    uint32_t out_offset;  // in points, into the shared output array
    uint32_t split = 1, outer2 = 0;  // the index x inside a group is taken apart: (x / split) * outer + (x % split) * outer2
    uint32_t in_offset = 0;          // in points, into the input array
};

// one launch of strided_sum_kernel: rows and columns side by side, lpo lanes (lpo / 2 lane pairs) per output
struct ReduceStep {
    SumJob rows, cols;
    uint32_t lpo;
};
struct ReducePlan {
    int steps = 0;       // 1: buckets -> row / column sums; 2: buckets -> partial sums -> row / column sums
    ReduceStep step[2] = {};
};

// Row sums (over lo) and column sums (over hi) of `groups` bucket sets.  lanes_per_output: the A/B knob of the one-step form
// (0 = by output count).
inline ReducePlan reduce_plan(const ReduceShape& s, uint32_t groups, bool sum_one_step, uint32_t lanes_per_output) {
    const uint32_t B = s.B, R = s.R, C = s.C;
    const uint32_t n_keys = groups * B, n_rows = groups * R, n_cols = groups * C;
    ReducePlan p;
    // Two steps when the sums are long: one lane pair walks a run of K buckets with no idle lanes (the tree of the
    // one-step form leaves half of its lane-steps empty), then a short tree adds the R / K or C / K partial sums.
    // Worth it from 2^18 buckets on (8 windows of 2^15, or the 2^19-bucket set of a fixed-base plan): with fewer the sums
    // are a latency chain and the second launch only lengthens it (measured: 2^17 buckets 0.223 vs 0.212 ms)
    const uint32_t K = (sum_one_step || n_keys < (1u << 18)) ? 0u : sum_part_len(s);
    if (K >= 2 && C % K == 0 && R % K == 0 && C / K >= 2 && R / K >= 2) {
        const uint32_t pr = C / K, pc = R / K;  // partial sums per row sum / per column sum
        p.steps = 2;
        // step 1: partial (row r, part p) = sum of buckets r C + p K + [0, K); (column j, part p) = sum of (p K + i) C + j
        p.step[0].rows = {n_rows * pr, R * pr, B, C, 1u, K, 0u, pr, K};
        p.step[0].cols = {n_cols * pc, C * pc, B, 1u, C, K, n_rows * pr, pc, K * C};
        p.step[0].lpo = 2u;
        // step 2: contiguous runs of pr (pc) partial sums
        p.step[1].rows = {n_rows, n_rows, 0u, pr, 1u, pr, 0u};
        p.step[1].cols = {n_cols, n_cols, 0u, pc, 1u, pc, n_rows, 1u, 0u, n_rows * pr};
        p.step[1].lpo = 2 * std::min<uint32_t>(32u, std::max(pr, pc) / 2);
    } else {
        p.steps = 1;
        p.step[0].rows = {n_rows, R, B, C, 1u, C, 0u};
        p.step[0].cols = {n_cols, C, B, 1u, C, R, n_rows};
        // lanes per output (two lanes = one point): many outputs (one bucket set per window) -> 16 pairs each walk
        // count/16 buckets and finish with a 4-level tree; few outputs (shared bucket set) -> 32 pairs, shortest chain
        p.step[0].lpo = lanes_per_output ? lanes_per_output : ((n_rows + n_cols) >= 4096 ? 32u : 64u);
    }
    return p;
}

// points of the partial-sum array between the two steps, per bucket set (0: the plan never takes two steps)
inline uint64_t reduce_parts_per_set(const ReduceShape& s) {
    const uint32_t k = sum_part_len(s);
    return k >= 2 ? 2 * (uint64_t)(s.B / k) : 0;
}

}  // namespace zkmi
