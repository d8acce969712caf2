// msm_front.h -- stages 1-4 of the MSM pipeline as one group-independent object: scalars -> window digits -> bucket-sorted
// entry list.  They depend on the scalar field, the window layout and a few options, not on the curve group, so the kernels
// (msm_sort.hip.h) and the host code that sizes their buffers and launches them are compiled once, in msm_front.hip; every
// MsmPlan<G> (msm_impl.hip.h) owns one MsmFront and consumes what it produces as a SortedView.  Declarations only.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>
#include "../../include/zkmi.h"
#include "dev_buf.h"

namespace zkmi {

struct MsmOptions;  // msm_plan.h
struct GlvConsts;   // glv_params.h

// what the accumulate and combine kernels read of a finished sort: a plan's own, or the one another plan lends (SortExport)
struct SortedView {
    const uint32_t *sorted = nullptr, *bstart = nullptr, *sstart = nullptr, *big_list = nullptr, *big_count = nullptr;
    uint32_t seg_len = 0;
};

// window layout of the owning plan, under the plan's names (MsmPlan::init derives it; nothing here depends on the group)
struct FrontLayout {
    int c = 0;
    uint32_t B = 0;                  // buckets per window, 2^(c-1)
    uint64_t n = 0, n_api = 0;       // entries per window / points as the caller counts them
    bool pre = false, wide = false;
    const GlvConsts* glv = nullptr;  // split-scalar digits with these constants; nullptr = plain digits
    int pw_first = 0, pw_count = 0, nwin = 0;
    int curve = 0;                   // ZK_CURVE_*: the scalar field
};

class MsmFront : FrontLayout {
public:
    MsmFront() = default;
    MsmFront(const MsmFront&) = delete;
    MsmFront& operator=(const MsmFront&) = delete;
    ~MsmFront() = default;  // blocks go back to the caching allocator: the owner makes sure that nothing of it is in flight

    // Plan creation, in the order MsmPlan::init calls them (its own allocations sit in between).  `opt` is the owning plan's:
    // two_level_sort is read at every sort, fine_log and sort_workgroups here.
    int init(const FrontLayout& layout, const MsmOptions* opt);  // scalars and digits; refuses wide windows the two-level sort cannot take
    int alloc_workspace();                                  // the sort's buffers
    int set_kernel_attributes();                            // LDS above 64 KiB needs the opt-in

    // stage 1 for the windows [w_first, w_first + w_count) of m_api scalars (device pointer)
    int digits(const uint32_t* scalars, uint32_t m_api, int w_first, int w_count, hipStream_t st);
    // stages 2-4 over the m entries per window that digits() left: histogram, scans, scatter -> view()
    int sort(uint32_t m, uint32_t dstride, uint32_t seg_len, int w_first, int w_count, uint32_t groups, hipStream_t st);
    SortedView view() const { return {sorted.as(), bstart.as(), sstart.as(), big_list.as(), big_count.as(), seg_len}; }

    bool two_level_ok() const;
    bool has_two_level_buffers() const { return (bool)tmp_ref; }
    uint32_t* scalars_buf() const { return d_scalars.as(); }  // staging for scalars that arrive from the host

    // zk_msm_plan_debug_view: the digits and what the last sort of this front did (sort() stores it; nothing reads it on the run path)
    const void* digits_buf() const { return d_dig.as<void>(); }
    int view_route = ZK_MSM_ROUTE_NONE, view_fine_log = 0;
    uint32_t view_dstride = 0;
    bool view_split_fine() const { return view_route >= ZK_MSM_ROUTE_TWO_LEVEL_DERIVE && tmp_fine; }

private:
    static int chunks_for(int windows, uint64_t count);
    int fine_log_for(uint64_t points) const;
    bool split_fine() const;
    int exclusive_scan(const uint32_t* in, uint32_t cnt, uint32_t* out, hipStream_t st);
    uintptr_t dig_base(uint32_t dstride) const;
    template <class FrP>
    void launch_digits(const uint32_t* scalars, uint32_t m_api, int w_first, int w_count, hipStream_t st);

    using DevBuf = mem::DevBuf;
    const MsmOptions* opt = nullptr;
    int range_log = 0;      // general mode: log2(buckets per sort workgroup)
    uint32_t bias[13] = {};  // sum_w 2^(c-1) 2^(cw): added to a scalar before it is cut into plain c-bit fields
    uint32_t seg_len = 0;   // of the last sort
    DevBuf d_scalars;
    DevBuf d_dig;  // windows x (n + 8) digits, uint16_t (c <= 16) or uint32_t
    DevBuf hist, total, bstart, sstart, bsums, grand, big_list, big_count, sorted;
    DevBuf tmp_ref, bin_start, slice_sums, bin_tot, bin_runs;  // two-level sort
    DevBuf tmp_fine;  // bytes: fine bucket bits of the level-A entries when the reference needs all 31 bits
};

}  // namespace zkmi
