// msm_host_tail.h -- stage 8 of the MSM pipeline (overview: msm_impl.hip.h): from the (S, T) pairs the weighted sums left per
// block of row / column sums to the one group element of the MSM, on the host in 64-bit-limb arithmetic (host64.hip.h).
// Needs no HIP runtime: MsmPlan::finish calls it, tests/native/host_tail_check.cpp runs it on multiples of the generator.
#pragma once
#include "common.hip.h"
#include "msm_reduce_plan.h"

namespace zkmi {

// The tail is one chain of a few hundred dependent point operations, run once per MSM on code the core has not seen since the
// last one.  Its three operations stay calls.  Left to the optimiser, the additions in the block loops count as hot and are
// expanded in place down to the field products: the BLS12-381 G2 tail grows to 106 KiB (12 KiB as calls) and takes 0.253-0.257 ms
// instead of 0.249-0.253 (EXPERIMENTS.md, "MSM host refactor").
template <class HF> __attribute__((noinline)) XYZZ<HF> tail_add(const XYZZ<HF>& a, const XYZZ<HF>& b) { return xyzz_add<HF>(a, b); }
template <class HF> __attribute__((noinline)) XYZZ<HF> tail_dbl(const XYZZ<HF>& a) { return xyzz_dbl<HF>(a); }
template <class HF> __attribute__((noinline)) XYZZ<HF> tail_point(const uint32_t* row) { return HF::xyzz_from_device(row); }

// h_final: per bucket set its bpr row blocks, then (after the row blocks of all sets) its bpc column blocks, each block (S, T) as
// two XYZZ rows in device form.  Per bucket set, with row blocks (S_k, T_k), column blocks (S'_k, T'_k), C = 2^lc, WS_BLOCK = 2^7:
//     W = 2^(lc+7) X_R + 2^lc sum S_k + 2^7 X_C + (sum S'_k + sum T_k),   X = sum_k k T_k
// general mode: total = sum_g 2^(c (q_first + g)) W_g by Horner from the top window down; the factors ride along the c
// doublings between two windows, so a set costs c doublings whatever its block structure;
// fixed-base mode (pre): one set, the same chain, no shift.
// out: the canonical affine limbs of the total (zeros for infinity; groups = 0 is the empty MSM).
template <class G>
int msm_host_tail(const uint32_t* h_final, uint32_t n_groups, const ReduceShape& shape, int c, int q_first, bool pre, uint64_t* out) {
    typedef typename G::HostF HF;
    constexpr int XW = 4 * G::F::LIMBS;
    const uint32_t bpr = shape.bpr, bpc = shape.bpc;
    XYZZ<HF> total = xyzz_inf<HF>();
    int lc = 0;
    while ((1u << lc) < shape.C) ++lc;
    const int groups = (int)n_groups;
    const uint32_t* rows_fin = h_final;
    const uint32_t* cols_fin = h_final + (size_t)groups * bpr * 2 * XW;
    bool first_set = true;
    for (int g = groups - 1; g >= 0; --g) {
        // X = sum_k k T_k as a running sum of suffixes (from the top block down): two additions per block
        XYZZ<HF> sum_s = xyzz_inf<HF>(), sum_t = xyzz_inf<HF>(), x_r = xyzz_inf<HF>();
        for (int k = (int)bpr - 1; k >= 0; --k) {
            const uint32_t* q = rows_fin + ((size_t)g * bpr + k) * 2 * XW;
            sum_s = tail_add<HF>(sum_s, tail_point<HF>(q));
            if (k > 0) {
                sum_t = tail_add<HF>(sum_t, tail_point<HF>(q + XW));  // T_k + .. + T_top
                x_r = tail_add<HF>(x_r, sum_t);
            } else {
                sum_t = tail_add<HF>(sum_t, tail_point<HF>(q + XW));
            }
        }
        XYZZ<HF> sum_sc = xyzz_inf<HF>(), x_c = xyzz_inf<HF>(), suf_c = xyzz_inf<HF>();
        for (int k = (int)bpc - 1; k >= 0; --k) {
            const uint32_t* q = cols_fin + ((size_t)g * bpc + k) * 2 * XW;
            sum_sc = tail_add<HF>(sum_sc, tail_point<HF>(q));
            if (k > 0) {
                suf_c = tail_add<HF>(suf_c, tail_point<HF>(q + XW));
                x_c = tail_add<HF>(x_c, suf_c);
            }
        }
        // terms in descending order of their exponent; `at` = exponent the accumulator currently sits at
        int at = first_set ? -1 : c;
        auto step = [&](int exp, const XYZZ<HF>& term, bool present) {
            if (!present) return;
            if (at >= 0) for (int k = 0; k < at - exp; ++k) total = tail_dbl<HF>(total);
            total = tail_add<HF>(total, term);
            at = exp;
        };
        if (bpr > 1 && lc + WS_BLOCK_LOG > c && !first_set) return fail(ZK_ERR_ARG, "internal: reduction layout does not fit the window");
        step(lc + WS_BLOCK_LOG, x_r, bpr > 1);
        step(lc, sum_s, true);
        step(WS_BLOCK_LOG, x_c, bpc > 1);
        step(0, tail_add<HF>(sum_sc, sum_t), true);
        first_set = false;
    }
    if (!pre) for (int k = 0; k < c * q_first; ++k) total = tail_dbl<HF>(total);
    HF::affine_to_canonical(xyzz_to_affine<HF>(total), out);
    return ZK_OK;
}

}  // namespace zkmi
