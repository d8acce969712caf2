// spartan.hip -- the two R1CS-specific passes of the Spartan prover and verifier over BN254 Fr / BLS12-381 Fr (gfx950):
//   witness products   az[i], bz[i], cz[i] = (A z)[i], (B z)[i], (C z)[i]                 (zk_r1cs_products_dev)
//   row binding        out[y] = sum_i E[i] (cA A + cB B + cC C)[i, y]                      (zk_r1cs_bind_dev)
// Both walk ONE layout, a merged three-matrix CSR: ptr u32[3 n_seg + 1], sub-segment q = 3 i + m holds the entries of matrix
// m (0 A, 1 B, 2 C) in segment i, idx[ptr[q] .. ptr[q+1]) and val alongside.  There is no tag per entry: the matrix is the
// position of the sub-segment.  Per segment the body keeps three sums acc_m = sum val[k] x[idx[k]] over sub-segment 3 i + m (one
// product per entry, one gather of x); the entry points differ in the epilogue only:
//   products (row-major CSR, segments = constraints, x = z):   az[i], bz[i], cz[i] = acc_A, acc_B, acc_C
//   bind     (column-major CSR, segments = columns, x = E):     out[y] = cA acc_A + cB acc_B + cC acc_C   -- three products per
//            column on top of the one per entry, where scaling the entries would cost two per entry.
// Segments are split by length as spmv_kernel's rows are (spmv.hip): a segment whose three sub-segments all have at most
// R1CS_LONG_ROW entries takes one lane.  A segment with a longer sub-segment (the constant-one column and the input columns of a
// real circuit reach the whole constraint count) is a LONG segment: the host cuts its long sub-segments into work items of a few
// thousand entries, one workgroup sums each item into `partials`, and one workgroup per long segment then adds up the items of
// its long sub-segments, walks its short ones itself and writes the segment.  Every output element is written by exactly one
// thread of one launch: no atomics, nothing needs clearing, and every sum is a fixed tree (fr_sum.hip.h).
//
// Like spmv.hip the kernels multiply canonical data directly: mont(v, x) = v x / R, so a sum is closed with R^2 (products) or with
// c_m R^2 (bind), once per segment.  Workgroups of MLE_TILE threads on strided grids capped at FR_MAX_BLOCKS.
#include "fr_sum.hip.h"

namespace zkmi {

constexpr int R1CS_MAX_LOG = ZK_R1CS_MAX_LOG;
constexpr uint32_t R1CS_LONG_ROW = ZK_R1CS_LONG_ROW;

// where a segment's sums go: products -- out[m] is the table of matrix m, c[m] = R^2; bind -- out[0] alone, c[m] = c_m R^2
template <class P>
struct R1csOut {
    uint32_t* out[3];
    Fp<P> c[3];
};

template <class P>
__device__ __forceinline__ Fp<P> r1cs_entry(uint32_t k, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ val,
                                            const uint32_t* __restrict__ x) {
    return fp_mul<P>(load_fr<P>(val + (size_t)k * P::W), load_fr<P>(x + (size_t)idx[k] * P::W));   // v x / R
}

template <class P, bool BIND>
__device__ __forceinline__ void r1cs_close(const Fp<P> (&acc)[3], uint64_t seg, const R1csOut<P>& o) {
    if (BIND) {
        const Fp<P> s = fp_add<P>(fp_add<P>(fp_mul<P>(acc[0], o.c[0]), fp_mul<P>(acc[1], o.c[1])), fp_mul<P>(acc[2], o.c[2]));
        store_fr<P>(o.out[0] + seg * P::W, fp_reduce_full<P>(s));
    } else {
#pragma unroll
        for (int m = 0; m < 3; ++m) store_fr<P>(o.out[m] + seg * P::W, fp_reduce_full<P>(fp_mul<P>(acc[m], o.c[m])));
    }
}

// one lane per short segment (an empty one writes zeros); long segments are left to the two kernels below
template <class P, bool BIND>
__global__ __launch_bounds__(MLE_TILE) void r1cs_segments_kernel(uint64_t n_seg, const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ idx,
                                                                 const uint32_t* __restrict__ val, const uint32_t* __restrict__ x, R1csOut<P> o) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t seg = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; seg < n_seg; seg += stride) {
        uint32_t p[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) p[m] = ptr[3 * seg + m];
        if (p[1] - p[0] > R1CS_LONG_ROW || p[2] - p[1] > R1CS_LONG_ROW || p[3] - p[2] > R1CS_LONG_ROW) continue;
        Fp<P> acc[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            acc[m] = fp_zero<P>();
            for (uint32_t k = p[m]; k < p[m + 1]; ++k) acc[m] = fp_add<P>(acc[m], r1cs_entry<P>(k, idx, val, x));
        }
        r1cs_close<P, BIND>(acc, seg, o);
    }
}

// one workgroup per work item [k0, k1) of a long sub-segment: partials[item] = the item's sum, still v x / R, canonical
template <class P>
__global__ __launch_bounds__(MLE_TILE) void r1cs_items_kernel(uint32_t n_items, const uint32_t* __restrict__ items, const uint32_t* __restrict__ idx,
                                                              const uint32_t* __restrict__ val, const uint32_t* __restrict__ x,
                                                              uint32_t* __restrict__ partials) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint32_t k0 = items[2 * item], k1 = items[2 * item + 1];
        Fp<P> acc = fp_zero<P>();
        for (uint32_t k = k0 + threadIdx.x; k < k1; k += MLE_TILE) acc = fp_add<P>(acc, r1cs_entry<P>(k, idx, val, x));
        block_sum_store<P>(acc, lds, partials + (size_t)item * P::W);
    }
}

// one workgroup per long segment: a long sub-segment is the sum of its items (item_ptr[3 j + m] .. item_ptr[3 j + m + 1], not
// empty), a short one (no item, at most R1CS_LONG_ROW entries) is walked here, one entry per thread
template <class P, bool BIND>
__global__ __launch_bounds__(MLE_TILE) void r1cs_long_kernel(uint32_t n_long, const uint32_t* __restrict__ long_segs, const uint32_t* __restrict__ item_ptr,
                                                             const uint32_t* __restrict__ partials, const uint32_t* __restrict__ ptr,
                                                             const uint32_t* __restrict__ idx, const uint32_t* __restrict__ val,
                                                             const uint32_t* __restrict__ x, R1csOut<P> o) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    for (uint32_t j = blockIdx.x; j < n_long; j += gridDim.x) {
        const uint64_t seg = long_segs[j];
        Fp<P> tot[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const uint32_t i0 = item_ptr[3 * j + m], i1 = item_ptr[3 * j + m + 1];
            Fp<P> acc = fp_zero<P>();
            if (i0 != i1) {
                for (uint32_t i = i0 + threadIdx.x; i < i1; i += MLE_TILE) acc = fp_add<P>(acc, load_fr<P>(partials + (size_t)i * P::W));
            } else {
                const uint32_t k0 = ptr[3 * seg + m], k1 = ptr[3 * seg + m + 1];
                for (uint32_t k = k0 + threadIdx.x; k < k1; k += MLE_TILE) acc = fp_add<P>(acc, r1cs_entry<P>(k, idx, val, x));
            }
            block_sum<P>(acc, lds);
            tot[m] = fp_zero<P>();
            if (threadIdx.x == 0) tot[m] = lds_get<P>(lds, 0);
        }
        if (threadIdx.x == 0) r1cs_close<P, BIND>(tot, seg, o);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------

struct R1csCsr {
    int log_seg;
    uint64_t n_entries;
    const void *ptr, *idx, *val;
    uint64_t n_long, n_items;
    const void *long_segs, *item_ptr, *items;
    void* partials;
};

// n_out outputs of 2^log_seg elements each; coeff == nullptr: the products epilogue
template <class P, bool BIND>
static int r1cs_impl(const char* who, const R1csCsr& c, int log_x, const void* x, const uint64_t* coeff, void* const* outs, int n_out, hipStream_t st) {
    const std::string name(who);
    if (c.log_seg < 0 || c.log_seg > R1CS_MAX_LOG || log_x < 0 || log_x > R1CS_MAX_LOG)
        return fail(ZK_ERR_ARG, name + ": need 0 <= log_seg, log_x <= 24");
    if (c.n_entries >> 32) return fail(ZK_ERR_ARG, name + ": the entries are addressed with 32 bits");
    if (!c.ptr || !x || (BIND && !coeff) || (c.n_entries && (!c.idx || !c.val))) return fail(ZK_ERR_ARG, name + ": null argument");
    for (int i = 0; i < n_out; ++i)
        if (!outs[i]) return fail(ZK_ERR_ARG, name + ": null output");
    const uint64_t eb = P::W * 4, n_seg = 1ull << c.log_seg;
    if (c.n_long > c.n_items || c.n_items > c.n_entries || c.n_long > n_seg || (c.n_items && !c.n_long))
        return fail(ZK_ERR_ARG, name + ": the counts of long segments, work items and entries do not fit together");
    if (c.n_long && (!c.long_segs || !c.item_ptr || !c.items || !c.partials)) return fail(ZK_ERR_ARG, name + ": null long-segment argument");
    const void* ins[7] = {x, c.ptr, c.idx, c.val, c.long_segs, c.item_ptr, c.items};
    const uint64_t in_len[7] = {eb << log_x, 4 * (3 * n_seg + 1), 4 * c.n_entries, eb * c.n_entries, 4 * c.n_long, 4 * (3 * c.n_long + 1), 8 * c.n_items};
    const void* w[4] = {outs[0], n_out > 1 ? outs[1] : nullptr, n_out > 2 ? outs[2] : nullptr, c.n_long ? c.partials : nullptr};
    const uint64_t w_len[4] = {eb * n_seg, eb * n_seg, eb * n_seg, eb * c.n_items};
    for (int i = 0; i < 4; ++i) {
        if (!w[i]) continue;
        if (overlaps_any(w[i], w_len[i], ins, in_len, 7)) return fail(ZK_ERR_ARG, name + ": an output overlaps an input");
        if (overlaps_any(w[i], w_len[i], w, w_len, i)) return fail(ZK_ERR_ARG, name + ": two outputs overlap");
    }
    R1csOut<P> o;
    const Fp<P> r2 = fp_const<P>(P::R2);
    for (int m = 0; m < 3; ++m) {
        o.out[m] = (uint32_t*)(BIND ? outs[0] : outs[m]);
        o.c[m] = BIND ? fp_mul<P>(fr_mont<P>(coeff + 4 * m), r2) : r2;   // c_m R R^2 / R
    }
    const uint32_t *ptr = (const uint32_t*)c.ptr, *idx = (const uint32_t*)c.idx, *val = (const uint32_t*)c.val, *xs = (const uint32_t*)x;
    hipLaunchKernelGGL((r1cs_segments_kernel<P, BIND>), dim3(fr_blocks(n_seg)), dim3(MLE_TILE), 0, st, n_seg, ptr, idx, val, xs, o);
    if (c.n_long) {
        const unsigned item_blocks = (unsigned)std::min<uint64_t>(c.n_items, FR_MAX_BLOCKS), long_blocks = (unsigned)std::min<uint64_t>(c.n_long, FR_MAX_BLOCKS);
        hipLaunchKernelGGL(r1cs_items_kernel<P>, dim3(item_blocks), dim3(MLE_TILE), 0, st, (uint32_t)c.n_items, (const uint32_t*)c.items, idx, val, xs,
                           (uint32_t*)c.partials);
        hipLaunchKernelGGL((r1cs_long_kernel<P, BIND>), dim3(long_blocks), dim3(MLE_TILE), 0, st, (uint32_t)c.n_long, (const uint32_t*)c.long_segs,
                           (const uint32_t*)c.item_ptr, (const uint32_t*)c.partials, ptr, idx, val, xs, o);
    }
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

#define R1CS_CSR_ARGS const R1csCsr csr = {log_seg, n_entries, d_ptr, d_idx, d_val, n_long, n_items, d_long_segs, d_item_ptr, d_items, d_partials}

int zk_r1cs_products_dev(int curve, int log_seg, uint64_t n_entries, const void* d_ptr, const void* d_idx, const void* d_val, uint64_t n_long,
                         const void* d_long_segs, const void* d_item_ptr, uint64_t n_items, const void* d_items, void* d_partials, int log_x,
                         const void* d_z, void* d_az, void* d_bz, void* d_cz, void* stream) {
    R1CS_CSR_ARGS;
    void* const outs[3] = {d_az, d_bz, d_cz};
#define CALL(P) return r1cs_impl<P, false>("r1cs_products", csr, log_x, d_z, nullptr, outs, 3, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_r1cs_bind_dev(int curve, int log_seg, uint64_t n_entries, const void* d_ptr, const void* d_idx, const void* d_val, uint64_t n_long,
                     const void* d_long_segs, const void* d_item_ptr, uint64_t n_items, const void* d_items, void* d_partials, int log_x,
                     const void* d_e, const uint64_t* coeff, void* d_out, void* stream) {
    R1CS_CSR_ARGS;
    void* const outs[1] = {d_out};
#define CALL(P) return r1cs_impl<P, true>("r1cs_bind", csr, log_x, d_e, coeff, outs, 1, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}
#undef R1CS_CSR_ARGS

}  // extern "C"
