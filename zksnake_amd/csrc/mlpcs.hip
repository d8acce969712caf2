// mlpcs.hip -- the scalar side of a multilinear KZG opening (PST13, as arkworks' MultilinearPC) over BN254 Fr / BLS12-381 Fr
// (gfx950).
//
// Opening f (2^log_n evaluations, variable 0 the least significant index bit, as in mle.hip) at z runs the chain
//     q_k[b] = f_k[2b+1] - f_k[2b],    f_(k+1)[b] = f_k[2b] + z_k q_k[b],    f_0 = f,
// whose last table f_(log_n) is the one value f(z) and whose q_k are the scalars of the proof's MSMs: f(x) - f(z) =
// sum_k (x_k - z_k) q_k(x_(k+1) ..).  It is the variable fold of mle.hip with the difference kept instead of dropped, so it is
// built the same way (mle_fold.hip.h): a workgroup of MLE_TILE threads holds a tile of MLE_TILE contiguous elements in LDS, folds up
// to MLE_TILE_LOG variables there and writes only the last fold of the tile, so the table is read once per MLE_TILE_LOG variables,
// each pass on a table 2^MLE_TILE_LOG times smaller.  Every quotient is written once, from the registers of the thread that formed
// it: in level s of a tile thread t holds entry t of the tile's 2^(MLE_TILE_LOG-1-s) consecutive entries of that level's slice, so
// each store instruction of a wave covers one contiguous run of 32-byte elements.
//
// LDS: the tile is limb-major (lds[limb][element], fr_sum.hip.h), 9 rows of 256 words.  In EVERY in-tile level thread t reads
// elements 2t and 2t+1 (neighbouring lanes 8 bytes apart in a row: the two words of a lane are adjacent and 8-byte aligned) and
// the level's result goes back to element t (neighbouring lanes 4 bytes apart), because the tile is compacted after each level.  An
// in-place butterfly would double the stride per level and end 32-way conflicted on the 32 banks of a word access; compacted, the
// deep levels have the stride of the first one and merely fewer active lanes.
//
// Like mle.hip the kernel multiplies canonical data by challenges carried in Montgomery form (mont(d, z R) = z d): no table is
// converted.
#include <algorithm>
#include "mle_fold.hip.h"

namespace zkmi {
using mem::DevBuf;

constexpr int MLPCS_MAX_LOG = ZK_MLPCS_MAX_LOG;

// One pass: n elements of `in` (a power of two), f >= 1 variables folded per tile of min(n, MLE_TILE) elements, (tile >> f) survivors
// per tile to `out`.  The pass starts at level `done` of a chain over q_total = 2^log_n elements: level k = done + s has
// q_total >> (k + 1) entries behind the q_total - (q_total >> k) entries of the levels before it, and this tile owns entries
// blockIdx.x * half .. + half - 1 of it, half = tile >> (s + 1).
template <class P>
__global__ __launch_bounds__(MLE_TILE) void mlpcs_quotients_kernel(uint64_t n, int f, uint64_t q_total, int done, FixArgs<P> a,
                                                                   const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                   uint32_t* __restrict__ q) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    const int t = threadIdx.x;
    const int tile = n < MLE_TILE ? (int)n : MLE_TILE;
    const uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + t;
    lds_put<P>(lds, t, t < tile ? load_fr<P>(in + i * P::W) : fp_zero<P>());
    __syncthreads();
    Fp<P> res = fp_zero<P>();
    for (int s = 0; s < f; ++s) {
        const int half = tile >> (s + 1);
        if (t < half) {
            const Fp<P> lo = lds_get<P>(lds, 2 * t), d = fp_sub<P>(lds_get<P>(lds, 2 * t + 1), lo);
            const uint64_t at = q_total - (q_total >> (done + s)) + (uint64_t)blockIdx.x * half + t;
            store_fr<P>(q + at * P::W, fp_reduce_full<P>(d));
            res = fold_step<P>(lo, d, a.r_m[s]);
        }
        if (s + 1 == f) break;  // the last level goes straight to memory
        __syncthreads();
        if (t < half) lds_put<P>(lds, t, res);
        __syncthreads();
    }
    const int keep = tile >> f;
    if (t < keep) store_fr<P>(out + ((uint64_t)blockIdx.x * keep + t) * P::W, fp_reduce_full<P>(res));
}

// ---- host side -----------------------------------------------------------------------------------------------------

// elements of work memory: the chain's intermediate tables, then the one-element result (zk_mle_eval_dev's layout)
static uint64_t mlpcs_work_elems(int log_n) { return fix_work_elems(log_n, log_n) + 1; }

template <class P>
static int mlpcs_quotients_impl(int log_n, const void* d_f, const uint64_t* point, void* d_q, uint64_t* eval_out, void* d_work,
                                hipStream_t st) {
    if (log_n < 0 || log_n > MLPCS_MAX_LOG) return fail(ZK_ERR_ARG, "mlpcs_quotients: need 0 <= log_n <= 24");
    if (!d_f || !eval_out || (log_n && (!point || !d_q))) return fail(ZK_ERR_ARG, "mlpcs_quotients: null argument");
    const uint64_t eb = P::W * 4, n = 1ull << log_n, need = mlpcs_work_elems(log_n);
    if (log_n && ranges_overlap(d_f, n * eb, d_q, (n - 1) * eb)) return fail(ZK_ERR_ARG, "mlpcs_quotients: d_q overlaps d_f");
    if (d_work && ranges_overlap(d_f, n * eb, d_work, need * eb)) return fail(ZK_ERR_ARG, "mlpcs_quotients: d_work overlaps d_f");
    if (d_work && log_n && ranges_overlap(d_q, (n - 1) * eb, d_work, need * eb)) return fail(ZK_ERR_ARG, "mlpcs_quotients: d_work overlaps d_q");
    if (log_n == 0) {   // no variable: no quotient, the value is the table
        ZK_HIP(hipMemcpyAsync(eval_out, d_f, eb, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        return ZK_OK;
    }
    DevBuf own;  // the work memory, when the caller passed none
    if (!d_work) ZK_HIP_RC(own.alloc(need * eb));
    uint32_t* work = d_work ? (uint32_t*)d_work : own.as();
    uint32_t* res = work + (need - 1) * P::W;
    uint32_t* tmp[2] = {work, work + ((size_t)P::W << std::max(log_n - MLE_TILE_LOG, 0))};   // used only by chains of 2 / 3 passes
    const uint32_t* cur = (const uint32_t*)d_f;
    int done = 0;
    for (int pass = 0; done < log_n; ++pass) {
        const int f = std::min(MLE_TILE_LOG, log_n - done);
        uint32_t* dst = done + f == log_n ? res : tmp[pass & 1];
        const uint64_t m = n >> done;
        hipLaunchKernelGGL(mlpcs_quotients_kernel<P>, dim3((unsigned)((m + MLE_TILE - 1) / MLE_TILE)), dim3(MLE_TILE), 0, st, m, f, n, done,
                           fix_args<P>(point + 4 * done, f), cur, dst, (uint32_t*)d_q);
        ZK_HIP(hipGetLastError());
        cur = dst;
        done += f;
    }
    ZK_HIP(hipMemcpyAsync(eval_out, res, eb, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));   // also: the work memory goes back to the allocator only after the chain has run
    return ZK_OK;
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_mlpcs_quotients_dev(int curve, int log_n, const void* d_f, const uint64_t* point, void* d_q, uint64_t* eval_out, void* d_work,
                           void* stream) {
#define CALL(P) return mlpcs_quotients_impl<P>(log_n, d_f, point, d_q, eval_out, d_work, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

}  // extern "C"
