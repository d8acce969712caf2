// fr_sum.hip.h -- what the kernels over Fr (mle.hip, ipa.hip, rangeproof.hip, gkr.hip, plonk.hip, frvec.hip, spmv.hip) share: the
// tile they are launched with, the capped strided grid, host scalars into kernel arguments, and exact, repeatable sums over a grid
// of any size: every workgroup of MLE_TILE threads adds its values in a fixed tree (block_sum) and stores one canonical partial
// sum, and ONE workgroup adds the partial sums (mle_combine_kernel; FrSum is the host side of that).
#pragma once
#include <algorithm>
#include "common.hip.h"
#include "fr_mem.hip.h"

namespace zkmi {

constexpr int MLE_TILE_LOG = ZK_MLE_TILE_LOG;
constexpr int MLE_TILE = 1 << MLE_TILE_LOG;   // elements per tile == threads per workgroup
static_assert(MLE_TILE == 256, "the kernels over Fr are launched with 256 threads");

// the cap of every strided grid: 2^18 threads, so a pass over more items strides; also the most partial sums ONE workgroup adds
constexpr unsigned FR_MAX_BLOCKS = 1024;
static inline unsigned fr_blocks(uint64_t items) {
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>((items + MLE_TILE - 1) / MLE_TILE, 1), FR_MAX_BLOCKS);
}

// a host scalar (4 x 64-bit limbs, any value) as a kernel argument: x R, below 2r -- mont(d, x R) = x d
template <class P>
static Fp<P> fr_mont(const uint64_t* x) {
    return fp_from_canonical<P>(reinterpret_cast<const uint32_t*>(x));
}
// x mod r as an integer, below 2r: the start of a chain of products by Montgomery-form factors
template <class P>
static Fp<P> fr_canon(const uint64_t* x) {
    return fp_mul<P>(fr_mont<P>(x), fp_raw_one<P>());
}
// a CANONICAL host scalar as it is: the integer as limbs
template <class P>
__host__ Fp<P> scalar_in(const uint64_t* s) {
    return fp_unpack<P>(reinterpret_cast<const uint32_t*>(s));
}
// s * R^k as an integer (k >= 0): what mont() must be fed to undo k divisions by R
template <class P>
__host__ Fp<P> scalar_times_r(const uint64_t* s, int k) {
    Fp<P> v = scalar_in<P>(s);
    for (int i = 0; i < k; ++i) v = fp_mul<P>(v, fp_const<P>(P::R2));
    return fp_reduce_full<P>(v);
}

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

// the workgroup's MLE_TILE values are added in a fixed tree (exact and the same on every run).  Afterwards element 0 of the tile
// holds the sum, below 2r: thread 0 reads it with lds_get<P>(lds, 0).  (It is left in the tile and not returned so that the read
// stays inside the caller's `threadIdx.x == 0` branch: returned, it changed the code of every kernel that stores the sum.)
template <class P>
__device__ __forceinline__ void block_sum(const Fp<P>& acc, uint32_t (*lds)[MLE_TILE]) {
    __syncthreads();  // the tile may still be read from an earlier use
    lds_put<P>(lds, threadIdx.x, acc);
    __syncthreads();
    for (int s = MLE_TILE / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds_put<P>(lds, threadIdx.x, fp_add<P>(lds_get<P>(lds, threadIdx.x), lds_get<P>(lds, threadIdx.x + s)));
        __syncthreads();
    }
}
// ... and thread 0 stores the canonical sum
template <class P>
__device__ __forceinline__ void block_sum_store(const Fp<P>& acc, uint32_t (*lds)[MLE_TILE], uint32_t* dst) {
    block_sum<P>(acc, lds);
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

// The host side of a two-level sum of k values: alloc(), then the caller launches its own kernel on `blocks` workgroups, each of
// which stores k partial sums at part() + blockIdx.x * k (block_sum_store), then finish().
template <class P>
struct FrSum {
    mem::DevBuf buf;   // blocks x k partial sums | the k results
    unsigned blocks = 0;
    int k = 0;

    int alloc(unsigned blocks_, int k_) {
        blocks = blocks_;
        k = k_;
        return buf.alloc((size_t)(blocks + 1) * k * P::W * 4);
    }
    uint32_t* part() const { return buf.as(); }
    // the combine behind the caller's kernel, ONE error check for both launches, the k results to `out` on the host; returns
    // after the stream has run, so the block may go back to the allocator
    int finish(uint64_t* out, hipStream_t st) const {
        uint32_t* res = part() + (size_t)blocks * k * P::W;
        hipLaunchKernelGGL(mle_combine_kernel<P>, dim3(1), dim3(MLE_TILE), 0, st, blocks, k, part(), res);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpyAsync(out, res, (size_t)k * P::W * 4, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        return ZK_OK;
    }
};

}  // namespace zkmi
