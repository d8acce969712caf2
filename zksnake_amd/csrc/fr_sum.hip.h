// fr_sum.hip.h -- exact, repeatable sums of Fr elements over a grid of any size: every workgroup of MLE_TILE threads adds its
// values in a fixed tree and stores one canonical partial sum, and ONE workgroup adds the partial sums (mle_combine_kernel).
// Shared by mle.hip and ipa.hip, with the tile constants both are launched with.
#pragma once
#include "common.hip.h"
#include "fr_mem.hip.h"

namespace zkmi {

constexpr int MLE_TILE_LOG = ZK_MLE_TILE_LOG;
constexpr int MLE_TILE = 1 << MLE_TILE_LOG;   // elements per tile == threads per workgroup
static_assert(MLE_TILE == 256, "the kernels of mle.hip and ipa.hip are launched with 256 threads");

template <class P>
__device__ __forceinline__ void lds_put(uint32_t (*lds)[MLE_TILE], int i, const Fp<P>& a) {
#pragma unroll
    for (int l = 0; l < P::N; ++l) lds[l][i] = a.v[l];
}
template <class P>
__device__ __forceinline__ Fp<P> lds_get(uint32_t (*lds)[MLE_TILE], int i) {
    Fp<P> a;
#pragma unroll
    for (int l = 0; l < P::N; ++l) a.v[l] = lds[l][i];
    return a;
}

// the workgroup's MLE_TILE values are added in a fixed tree and thread 0 stores the canonical sum (exact and the same on every run)
template <class P>
__device__ __forceinline__ void block_sum_store(const Fp<P>& acc, uint32_t (*lds)[MLE_TILE], uint32_t* dst) {
    __syncthreads();  // the tile may still be read from an earlier use
    lds_put<P>(lds, threadIdx.x, acc);
    __syncthreads();
    for (int s = MLE_TILE / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds_put<P>(lds, threadIdx.x, fp_add<P>(lds_get<P>(lds, threadIdx.x), lds_get<P>(lds, threadIdx.x + s)));
        __syncthreads();
    }
    if (threadIdx.x == 0) store_fr<P>(dst, fp_reduce_full<P>(lds_get<P>(lds, 0)));
}

// second level: partial[b * k + s] over b < count is added into out[s], s < k, by one workgroup
template <class P>
__global__ __launch_bounds__(MLE_TILE) void mle_combine_kernel(uint32_t count, int k, const uint32_t* __restrict__ partial, uint32_t* __restrict__ out) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    for (int s = 0; s < k; ++s) {
        Fp<P> acc = fp_zero<P>();
        for (uint32_t b = threadIdx.x; b < count; b += MLE_TILE) acc = fp_add<P>(acc, load_fr<P>(partial + ((size_t)b * k + s) * P::W));
        block_sum_store<P>(acc, lds, out + (size_t)s * P::W);
    }
}

static inline bool ranges_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

}  // namespace zkmi
