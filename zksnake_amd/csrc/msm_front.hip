// msm_front.hip -- MsmFront (msm_front.h): the host half of stages 1-4 of the MSM pipeline and the ONLY translation unit that
// includes their kernels (msm_sort.hip.h).  The kernels are static: a second includer would get copies of its own, and the
// large-LDS attributes set here would not cover a launch of those.  Pipeline overview: msm_impl.hip.h.
#include <algorithm>
#include "msm_front.h"
#include "msm_sort.hip.h"

namespace zkmi {

int MsmFront::init(const FrontLayout& layout, const MsmOptions* options) {
    static_cast<FrontLayout&>(*this) = layout;
    opt = options;
    // bucket ranges (general mode, small inputs): about 256 sort workgroups in total, at least 64 buckets each
    {
        const uint32_t wgs = opt->sort_workgroups;
        uint32_t want = std::max<uint32_t>(1u, wgs / (uint32_t)std::max(1, pw_count));
        uint32_t per = std::max<uint32_t>(64u, B / want);
        if (per > B) per = B;
        range_log = log2_u64(per);
        if ((1u << range_log) > B) range_log = c - 1;
    }
    memset(bias, 0, sizeof(bias));
    for (int w = 0; w < nwin; ++w) {
        int bit = w * c + (c - 1);
        bias[bit >> 5] |= 1u << (bit & 31);
    }
    int scalar_words = 0;
#define ZK_FRONT_WORDS(FR) scalar_words = FR::W
    ZK_DISPATCH_FR(curve, ZK_FRONT_WORDS);
#undef ZK_FRONT_WORDS
    ZK_HIP_RC(d_scalars.alloc(n_api * scalar_words * 4));
    ZK_HIP_RC(d_dig.alloc((size_t)pw_count * (n + 8) * (wide ? 4 : 2)));
    if (wide && !two_level_ok()) return fail(ZK_ERR_ARG, "this size does not fit the two-level sort that wide windows need");
    return ZK_OK;
}

int MsmFront::alloc_workspace() {
    const uint64_t max_sets = pre ? 1ull : (uint64_t)pw_count;
    const uint64_t keys = max_sets * B, entries = (uint64_t)pw_count * n;
    // windows x chunks <= max(256, windows) sub-histograms: of all B buckets (one-level sort) or of the coarse bins only
    ZK_HIP_RC(hist.alloc((size_t)std::max<uint64_t>(256, pw_count) * (wide ? (B >> fine_log_for(n)) : B) * 4));
    ZK_HIP_RC(total.alloc(keys * 4));
    ZK_HIP_RC(bstart.alloc((keys + 1) * 4));
    ZK_HIP_RC(sstart.alloc((keys + 1) * 4));
    ZK_HIP_RC(bsums.alloc(((keys + SCAN_BLOCK - 1) / SCAN_BLOCK + 1) * 4));
    ZK_HIP_RC(grand.alloc(4));
    ZK_HIP_RC(big_list.alloc(keys * 4));
    ZK_HIP_RC(big_count.alloc(8));
    ZK_HIP_RC(sorted.alloc(entries * 4));
    if (two_level_ok()) {
        ZK_HIP_RC(tmp_ref.alloc(entries * 4));
        if (split_fine()) ZK_HIP_RC(tmp_fine.alloc(entries));
        ZK_HIP_RC(bin_start.alloc((max_sets * (B >> fine_log_for(n)) + 1) * 4));
        ZK_HIP_RC(slice_sums.alloc(4096 * BINS_SLICES * 4));
        ZK_HIP_RC(bin_tot.alloc(4096 * 4));
        ZK_HIP_RC(bin_runs.alloc(max_sets * (B >> fine_log_for(n)) * 4));
    }
    return ZK_OK;
}

int MsmFront::set_kernel_attributes() {
    int lds_bytes = (int)((wide ? (1u << 15) : B) * 4);  // the one-level kernels never run for wide windows
    ZK_HIP(hipFuncSetAttribute((const void*)hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    ZK_HIP(hipFuncSetAttribute((const void*)scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    ZK_HIP(hipFuncSetAttribute((const void*)hist_range_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    ZK_HIP(hipFuncSetAttribute((const void*)scatter_range_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    ZK_HIP(hipFuncSetAttribute((const void*)scatter_hi_staged_kernel<uint16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    ZK_HIP(hipFuncSetAttribute((const void*)scatter_hi_staged_kernel<uint32_t>, hipFuncAttributeMaxDynamicSharedMemorySize, 104 * 1024));
    ZK_HIP(hipFuncSetAttribute((const void*)sort_lo_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024));
    return ZK_OK;
}

// chunked sort: windows x chunks workgroups of 1024 threads, ONE per CU (the LDS histogram takes 128 KiB at
// c = 16), so their number is kept at or just below the 256 CUs: 272 workgroups would run as 256 + 16,
// i.e. take twice as long
int MsmFront::chunks_for(int windows, uint64_t count) {
    int k = 256 / std::max(1, windows);
    if (k < 1) k = 1;
    uint64_t cap = (count + 4095) / 4096;  // at least 4096 entries per chunk
    if ((uint64_t)k > cap) k = (int)std::max<uint64_t>(1, cap);
    return k;
}

int MsmFront::exclusive_scan(const uint32_t* in, uint32_t cnt, uint32_t* out, hipStream_t st) {
    uint32_t blocks = (cnt + SCAN_BLOCK - 1) / SCAN_BLOCK;
    hipLaunchKernelGGL(scan_block_kernel, dim3(blocks), dim3(SCAN_BLOCK), 0, st, in, cnt, out, bsums.as());
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(SCAN_BLOCK), 0, st, bsums.as(), blocks, grand.as());
    hipLaunchKernelGGL(scan_add_kernel, dim3(blocks), dim3(SCAN_BLOCK), 0, st, out, cnt, bsums.as(), grand.as());
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

// fine bucket bits of the two-level sort for n points: the largest of 8, 7 that leaves room for the index in a 32-bit
// entry, with at least four coarse bins per window and at most 4096 (window, bin) pairs (one-workgroup scan); 0 = n/a
int MsmFront::fine_log_for(uint64_t points) const {
    // fixed-base mode: ONE bucket set over references into the (window, point) table, so the references are wider
    // and the coarse bins are shared by all windows -- more, smaller bins keep level B parallel
    const uint64_t refs = pre ? (uint64_t)pw_count * points : points;
    const uint64_t sets = pre ? 1 : (uint64_t)pw_count;
    if (wide) {
        const int f = c - 13;  // 4096 coarse bins; the fine bits move out of the entry when the reference needs the room
        return refs <= 0x7FFFFFFFull ? f : 0;
    }
    const int f_env = opt->fine_log;  // tuning knob (general mode)
    if (f_env && !pre && refs <= (1ull << (31 - f_env)) && c - 1 >= f_env + 2 && sets * (B >> f_env) <= 4096) return f_env;
    const int f_hi = pre ? 5 : FINE_LOG_MAX, f_lo = pre ? 4 : FINE_LOG_MAX - 1;
    // general mode: the widest bins that still hold about 8192 entries each (one level-B workgroup sorts a bin in LDS;
    // 2^21 split-scalar entries per window: 7 fine bits, 0.175 ms for digits + sort against 0.20 with 8)
    int best = 0;
    for (int f = f_hi; f >= f_lo; --f) {
        if (!(refs <= (1ull << (31 - f)) && c - 1 >= f + 2 && sets * (B >> f) <= 4096)) continue;
        if (pre || (points >> (c - 1 - f)) <= 8192) return f;
        best = f;
    }
    return best;
}

// level-A entries carry (sign, fine bucket bits, reference) in 32 bits while that fits; wide windows over a big table
// (13 x n rows, n > 2^20) keep the fine bits in a byte array beside them
bool MsmFront::split_fine() const {
    return wide && pre && (uint64_t)pw_count * n > (1ull << (31 - (c - 13)));
}

bool MsmFront::two_level_ok() const {
    return opt->two_level_sort && fine_log_for(n) > 0;
}

// digit rows are stored relative to the plan's first window; the kernels index them with absolute windows
uintptr_t MsmFront::dig_base(uint32_t dstride) const {
    return reinterpret_cast<uintptr_t>(d_dig.as<void>()) - (uintptr_t)pw_first * dstride * (wide ? 4 : 2);
}

// 1. digits (the windows of this run)
template <class FrP>
void MsmFront::launch_digits(const uint32_t* sc, uint32_t m_api, int w_first, int w_count, hipStream_t st) {
    const uint32_t m = glv ? 2 * m_api : m_api;  // entries per window
    const uint32_t dstride = (m + 7u) & ~7u;
    DigitBias b;
    memcpy(b.v, bias, sizeof(b.v));
    uint32_t* const big_count = this->big_count.as();
    if (glv) hipLaunchKernelGGL(glv_digits_kernel<FrP>, dim3((m_api + 255) / 256), dim3(256), 0, st, sc, m_api, dstride, c, w_first, w_count, b,
                                *glv, reinterpret_cast<uint16_t*>(dig_base(dstride)), big_count);
    else if (wide) hipLaunchKernelGGL((digits_kernel<FrP, uint32_t>), dim3((m + 255) / 256), dim3(256), 0, st, sc, m, dstride, c, w_first, w_count, b,
                                      reinterpret_cast<uint32_t*>(dig_base(dstride)), big_count);
    else hipLaunchKernelGGL((digits_kernel<FrP, uint16_t>), dim3((m + 255) / 256), dim3(256), 0, st, sc, m, dstride, c, w_first, w_count, b,
                            reinterpret_cast<uint16_t*>(dig_base(dstride)), big_count);
}
int MsmFront::digits(const uint32_t* scalars, uint32_t m_api, int w_first, int w_count, hipStream_t st) {
#define ZK_FRONT_DIGITS(FR) launch_digits<FR>(scalars, m_api, w_first, w_count, st)
    ZK_DISPATCH_FR(curve, ZK_FRONT_DIGITS);
#undef ZK_FRONT_DIGITS
    return ZK_OK;
}

// stages 2-4: histogram, scans, scatter -> sorted / bstart / sstart (+ the lists of buckets with many runs)
int MsmFront::sort(uint32_t m, uint32_t dstride, uint32_t run_seg_len, int w_first, int w_count, uint32_t groups, hipStream_t st) {
    seg_len = run_seg_len;
    const uint32_t n_keys = groups * B;
    const int nchunk = chunks_for(w_count, m);  // this run's windows fill the chip
    const uint32_t ch_len = (m + nchunk - 1) / nchunk;
    const uint16_t* d_dig = reinterpret_cast<const uint16_t*>(dig_base(dstride));
    const uint32_t* d_dig32 = reinterpret_cast<const uint32_t*>(dig_base(dstride));
    // general mode, small inputs: bucket-range partition (measured faster up to 2^18); otherwise the two-level sort
    const bool ranged = !pre && !wide && m < (1u << 19);
    const bool two_level = !ranged && this->tmp_ref && opt->two_level_sort;
    // the kernels take plain pointers: the members' blocks under the members' names
    uint32_t *const hist = this->hist.as(), *const total = this->total.as(), *const bstart = this->bstart.as(), *const sstart = this->sstart.as();
    uint32_t *const bsums = this->bsums.as(), *const grand = this->grand.as(), *const big_list = this->big_list.as(), *const big_count = this->big_count.as();
    uint32_t *const sorted = this->sorted.as(), *const tmp_ref = this->tmp_ref.as(), *const bin_start = this->bin_start.as(), *const slice_sums = this->slice_sums.as();
    uint32_t *const bin_tot = this->bin_tot.as(), *const bin_runs = this->bin_runs.as();
    uint8_t* const tmp_fine = this->tmp_fine.as<uint8_t>();
    view_route = ranged ? ZK_MSM_ROUTE_RANGED : ZK_MSM_ROUTE_ONE_LEVEL;   // zk_msm_plan_debug_view
    view_fine_log = 0;
    view_dstride = dstride;
    if (two_level) {
        const int fl = fine_log_for(n);
        view_fine_log = fl;
        const uint32_t NB = B >> fl;
        const uint32_t ch8 = (ch_len + 7) & ~7u;  // the kernels read eight digits per load
        // fixed-base mode: one bucket set fed by all (window, chunk) sub-histograms; general mode: one set per window
        const int sets = pre ? 1 : w_count, subs = pre ? w_count * nchunk : nchunk;
        const uint32_t pairs = (uint32_t)sets * NB;
        // general mode with a small count matrix: no scan launch, every level-A workgroup derives its own offsets from
        // the raw counts and the row totals (kept behind the count matrix in hist)
        const bool derive = !pre && NB <= (uint32_t)SORT_THREADS && (uint64_t)nchunk * NB <= 8192;
        uint32_t* rowtot = derive ? hist + (size_t)w_count * nchunk * NB : nullptr;
        if (wide) hipLaunchKernelGGL(hist_hi_kernel<uint32_t>, dim3(w_count * nchunk), dim3(SORT_THREADS), (NB + 1) * 4, st, d_dig32, m, dstride, c, w_first, nchunk, ch8, fl, hist, rowtot);
        else hipLaunchKernelGGL(hist_hi_kernel<uint16_t>, dim3(w_count * nchunk), dim3(SORT_THREADS), (NB + 1) * 4, st, d_dig, m, dstride, c, w_first, nchunk, ch8, fl, hist, rowtot);
        view_route = derive ? ZK_MSM_ROUTE_TWO_LEVEL_DERIVE : (uint64_t)pairs * subs >= (1u << 17) ? ZK_MSM_ROUTE_TWO_LEVEL_PARTIAL : ZK_MSM_ROUTE_TWO_LEVEL_SCAN;
        if (derive) {
            // offsets derived in scatter_hi_staged_kernel
        } else if ((uint64_t)pairs * subs >= (1u << 17)) {
            const unsigned bb = (pairs + 63) / 64;
            hipLaunchKernelGGL(bins_partial_kernel, dim3(bb), dim3(1024), 0, st, hist, subs, NB, pairs, slice_sums, bin_tot);
            hipLaunchKernelGGL(bins_scan_tot_kernel, dim3(1), dim3(1024), 0, st, bin_tot, pairs, bin_start, bstart + n_keys);
            hipLaunchKernelGGL(bins_prefix_kernel, dim3(bb), dim3(1024), 0, st, hist, subs, NB, pairs, slice_sums, bin_start);
        } else {
            hipLaunchKernelGGL(bins_scan_kernel, dim3(1), dim3(1024), 0, st, hist, sets, subs, NB, bin_start, bstart + n_keys);
        }
        {
            const uint32_t NBP = (NB + 127) & ~127u;
            const size_t lds_a = (size_t)SCATTER_TILE * 4 + (size_t)NBP * 12 + (size_t)SCATTER_TILE * 2 + (tmp_fine ? SCATTER_TILE : 0);
            if (wide) hipLaunchKernelGGL(scatter_hi_staged_kernel<uint32_t>, dim3(w_count * nchunk), dim3(SORT_THREADS), lds_a, st, d_dig32, m, dstride, c, w_first, nchunk, ch8, fl, pre ? 1 : 0, (uint32_t)n, pw_first, hist, tmp_ref, tmp_fine,
                                         (const uint32_t*)rowtot, bin_start, bstart + n_keys);
            else hipLaunchKernelGGL(scatter_hi_staged_kernel<uint16_t>, dim3(w_count * nchunk), dim3(SORT_THREADS), lds_a, st, d_dig, m, dstride, c, w_first, nchunk, ch8, fl, pre ? 1 : 0, (uint32_t)n, pw_first, hist, tmp_ref, (uint8_t*)nullptr,
                                    (const uint32_t*)rowtot, bin_start, bstart + n_keys);
        }
        // LDS stage of level B: 1.5x the expected entries of a coarse bin, capped at 96 KiB
        uint64_t expect = ((uint64_t)w_count * m) / ((uint64_t)sets * NB);
        uint32_t stage_cap = (uint32_t)std::min<uint64_t>(24576, std::max<uint64_t>(2048, expect + expect / 2));
        hipLaunchKernelGGL(sort_lo_kernel, dim3(sets * NB), dim3(SORT_LO_THREADS), (size_t)stage_cap * 4, st, bin_start, tmp_ref, (const uint8_t*)tmp_fine, B, fl, stage_cap, seg_len, bstart, sorted, bin_runs);
        // run offsets in one launch from the bins' run totals
        hipLaunchKernelGGL(runs_offsets_kernel, dim3((n_keys + SCAN_BLOCK - 1) / SCAN_BLOCK), dim3(SCAN_BLOCK), 0, st, bstart, n_keys, seg_len, fl, (const uint32_t*)bin_runs, sstart, big_list, big_count);
    } else if (ranged) {
        hipLaunchKernelGGL(hist_range_kernel, dim3(w_count * (B >> range_log)), dim3(SORT_THREADS), (4u << range_log), st, d_dig, m, dstride, c, w_first, range_log, total);
    } else {
        hipLaunchKernelGGL(hist_kernel, dim3(w_count * nchunk), dim3(SORT_THREADS), B * 4, st, d_dig, m, dstride, c, w_first, nchunk, ch_len, hist);
        hipLaunchKernelGGL(prefix_kernel, dim3((n_keys + 255) / 256), dim3(256), 0, st, hist, pre ? w_count * nchunk : nchunk, B, n_keys, total);
    }
    int rc;
    if (!two_level && (rc = exclusive_scan(total, n_keys, bstart, st))) return rc;
    if (!two_level) {
        // run offsets of the other sorts: run counts computed on the fly + three-launch scan
        const uint32_t blocks = (n_keys + SCAN_BLOCK - 1) / SCAN_BLOCK;
        hipLaunchKernelGGL(runs_scan_block_kernel, dim3(blocks), dim3(SCAN_BLOCK), 0, st, bstart, n_keys, seg_len, sstart, bsums, big_list, big_count);
        hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(SCAN_BLOCK), 0, st, bsums, blocks, grand);
        hipLaunchKernelGGL(scan_add_kernel, dim3(blocks), dim3(SCAN_BLOCK), 0, st, sstart, n_keys, bsums, grand);
    }
    if (two_level) {
        // already sorted
    } else if (ranged) {
        hipLaunchKernelGGL(scatter_range_kernel, dim3(w_count * (B >> range_log)), dim3(SORT_THREADS), (4u << range_log), st, d_dig, m, dstride, c, w_first, range_log, bstart, sorted);
    } else {
        const unsigned blocks = pre ? (unsigned)(w_count * nchunk) : (unsigned)(8 * ((w_count + 7) / 8) * nchunk);
        hipLaunchKernelGGL(scatter_kernel, dim3(blocks), dim3(SORT_THREADS), B * 4, st, d_dig, m, dstride, c, w_first, w_count, nchunk, ch_len, pre ? 1 : 0, (uint32_t)n, pw_first, hist, bstart, sorted);
    }
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

}  // namespace zkmi
