// ipa.hip -- the scalar side of the Bulletproofs inner-product argument over BN254 Fr / BLS12-381 Fr (gfx950).
//
// Stands in for the per-round list arithmetic of InnerProductArgument.prove / .verify
// (python/zksnake/subprotocol/bulletproofs/ipa.py:105-145, :178-198).  The reference folds the generators every round,
// G' = u^-1 G_lo + u G_hi; here they are never folded.  With s_i = prod_{t<k} (bit (log_n-1-t) of i ? u_t : u_t^-1) the
// folded generator is G^(k)_j = sum_{i = j mod m} s_i G_i (and H^(k)_j the same with s_i^-1), so every L_k, R_k is an MSM
// over the ORIGINAL G || H whose scalars this file writes: one MSM plan serves the commitment, every round and the verifier.
//
// Like mle.hip the kernels multiply canonical data by scalars carried in Montgomery form (mont(x, s R) = x s), so no
// vector is ever converted; a product of two canonical values is closed with R^2.  Workgroups of MLE_TILE threads, the
// grid capped at FR_MAX_BLOCKS workgroups (2^18 threads, so a pass over 2^19 items strides); the cross products are per-workgroup
// partial sums added by one workgroup (fr_sum.hip.h).
#include "ipa_chain.hip.h"

namespace zkmi {

constexpr int IPA_MAX_LOG = ZK_IPA_MAX_LOG;

template <class P>
struct IpaChallenge {
    Fp<P> u_m, ui_m;  // u R and u^-1 R
};

// in place, j < m: a[j] = u a[j] + u^-1 a[j+m], b[j] = u^-1 b[j] + u b[j+m].  Element j is read and written by one thread only,
// element j+m only read.
template <class P>
__global__ __launch_bounds__(MLE_TILE) void ipa_fold_kernel(uint64_t m, IpaChallenge<P> c, uint32_t* a, uint32_t* b) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t j = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; j < m; j += stride) {
        const Fp<P> a_lo = load_fr<P>(a + j * P::W), a_hi = load_fr<P>(a + (j + m) * P::W);
        store_fr<P>(a + j * P::W, fp_reduce_full<P>(fp_add<P>(fp_mul<P>(a_lo, c.u_m), fp_mul<P>(a_hi, c.ui_m))));
        const Fp<P> b_lo = load_fr<P>(b + j * P::W), b_hi = load_fr<P>(b + (j + m) * P::W);
        store_fr<P>(b + j * P::W, fp_reduce_full<P>(fp_add<P>(fp_mul<P>(b_lo, c.ui_m), fp_mul<P>(b_hi, c.u_m))));
    }
}

// i < n: s[i], s_inv[i] take the challenge of the round before (init: they become 1, or s_inv[i] the caller's h_weight[i]), and --
// write != 0, m >= 2 live elements of a, b -- the 2n scalars of L and of R are written, zeros included.  With j = i mod m,
// h = m / 2 the partner of j is j ^ h.
template <class P>
__global__ __launch_bounds__(MLE_TILE) void ipa_scalars_kernel(uint64_t n, uint64_t m, int shift, int init, int write, IpaChallenge<P> c,
                                                               const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                               uint32_t* __restrict__ s, uint32_t* __restrict__ s_inv,
                                                               const uint32_t* __restrict__ h_weight, uint32_t* __restrict__ scal_l,
                                                               uint32_t* __restrict__ scal_r) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    const Fp<P> r2 = fp_const<P>(P::R2), zero = fp_zero<P>();
    for (uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; i < n; i += stride) {
        Fp<P> sv, si;
        if (init) {
            sv = si = fp_raw_one<P>();
            if (h_weight) si = load_fr<P>(h_weight + i * P::W);
        } else {
            const bool bit = (i >> shift) & 1;
            sv = fp_reduce_full<P>(fp_mul<P>(load_fr<P>(s + i * P::W), bit ? c.u_m : c.ui_m));
            si = fp_reduce_full<P>(fp_mul<P>(load_fr<P>(s_inv + i * P::W), bit ? c.ui_m : c.u_m));
        }
        store_fr<P>(s + i * P::W, sv);
        store_fr<P>(s_inv + i * P::W, si);
        if (!write) continue;
        const uint64_t h = m >> 1, j = i & (m - 1), p = j ^ h;
        const bool upper = (j & h) != 0;
        const Fp<P> pa = fp_reduce_full<P>(fp_mul<P>(load_fr<P>(a + p * P::W), fp_mul<P>(sv, r2)));
        const Fp<P> pb = fp_reduce_full<P>(fp_mul<P>(load_fr<P>(b + p * P::W), fp_mul<P>(si, r2)));
        store_fr<P>(scal_l + i * P::W, upper ? pa : zero);        // a_lo against G_hi
        store_fr<P>(scal_l + (n + i) * P::W, upper ? zero : pb);  // b_hi against H_lo
        store_fr<P>(scal_r + i * P::W, upper ? zero : pa);        // a_hi against G_lo
        store_fr<P>(scal_r + (n + i) * P::W, upper ? pb : zero);  // b_lo against H_hi
    }
}

// partial[2 blk] = sum a[j] b[j+h], partial[2 blk + 1] = sum a[j+h] b[j] over the workgroup's j < h
template <class P>
__global__ __launch_bounds__(MLE_TILE) void ipa_cross_kernel(uint64_t h, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                             uint32_t* __restrict__ partial) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    Fp<P> cl = fp_zero<P>(), cr = cl;
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t j = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; j < h; j += stride) {
        cl = fp_add<P>(cl, fp_mul<P>(load_fr<P>(a + j * P::W), load_fr<P>(b + (j + h) * P::W)));
        cr = fp_add<P>(cr, fp_mul<P>(load_fr<P>(a + (j + h) * P::W), load_fr<P>(b + j * P::W)));
    }
    const Fp<P> r2 = fp_const<P>(P::R2);   // every term carries R^-1: closed once per thread
    uint32_t* dst = partial + (size_t)blockIdx.x * 2 * P::W;
    block_sum_store<P>(fp_mul<P>(cl, r2), lds, dst);
    block_sum_store<P>(fp_mul<P>(cr, r2), lds, dst + P::W);
}

template <class P>
struct IpaVerifyArgs {
    IpaChain<P> c;
    Fp<P> a, b;   // the proof's scalars, below 2r
};

// out[i] = a s_i, out[n+i] = b s_i^-1: log_n products each, the chain starting at the canonical a (b)
template <class P>
__global__ __launch_bounds__(MLE_TILE) void ipa_verify_scalars_kernel(uint64_t n, int log_n, IpaVerifyArgs<P> v, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; i < n; i += stride) {
        Fp<P> sa = v.a, sb = v.b;
        // ipa_chain_run's loop, written out: through the call the BN254 instance comes out 4 VALU instructions longer (572 for 568)
        for (int t = 0; t < log_n; ++t) {
            const bool bit = (i >> (log_n - 1 - t)) & 1;
            sa = fp_mul<P>(sa, bit ? v.c.u_m[t] : v.c.ui_m[t]);
            sb = fp_mul<P>(sb, bit ? v.c.ui_m[t] : v.c.u_m[t]);
        }
        store_fr<P>(out + i * P::W, fp_reduce_full<P>(sa));
        store_fr<P>(out + (n + i) * P::W, fp_reduce_full<P>(sb));
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------

template <class P>
static int ipa_round_impl(int log_n, int k, void* d_a, void* d_b, void* d_s, void* d_s_inv, const void* d_h_weight, const uint64_t* u,
                          const uint64_t* u_inv, void* d_scal_l, void* d_scal_r, uint64_t* cross, hipStream_t st) {
    if (log_n < 0 || log_n > IPA_MAX_LOG || k < 0 || k > log_n) return fail(ZK_ERR_ARG, "ipa_round: need 0 <= k <= log_n <= 22");
    if (!d_a || !d_b || !d_s || !d_s_inv) return fail(ZK_ERR_ARG, "ipa_round: null vector");
    if (k == 0 ? (u || u_inv) : (!u || !u_inv)) return fail(ZK_ERR_ARG, "ipa_round: a challenge goes with every round but the first, and only those");
    if (k && d_h_weight) return fail(ZK_ERR_ARG, "ipa_round: the weights of s_inv go with round 0 only");
    const bool write = k < log_n;
    if (write && (!d_scal_l || !d_scal_r || !cross)) return fail(ZK_ERR_ARG, "ipa_round: null output");
    const uint64_t eb = P::W * 4, n = 1ull << log_n, m = n >> k;
    const void* buf[7] = {d_a, d_b, d_s, d_s_inv, write ? d_scal_l : nullptr, write ? d_scal_r : nullptr, d_h_weight};
    const uint64_t len[7] = {n * eb, n * eb, n * eb, n * eb, 2 * n * eb, 2 * n * eb, n * eb};
    for (int x = 1; x < 7; ++x)   // every buffer against the ones before it
        if (buf[x] && overlaps_any(buf[x], len[x], buf, len, x)) return fail(ZK_ERR_ARG, "ipa_round: two buffers overlap");

    IpaChallenge<P> c;
    c.u_m = c.ui_m = fp_zero<P>();
    if (k) {
        c.u_m = fr_mont<P>(u);
        c.ui_m = fr_mont<P>(u_inv);
        hipLaunchKernelGGL(ipa_fold_kernel<P>, dim3(fr_blocks(m)), dim3(MLE_TILE), 0, st, m, c, (uint32_t*)d_a, (uint32_t*)d_b);
        ZK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ipa_scalars_kernel<P>, dim3(fr_blocks(n)), dim3(MLE_TILE), 0, st, n, m, log_n - k, k == 0 ? 1 : 0, write ? 1 : 0, c,
                       (const uint32_t*)d_a, (const uint32_t*)d_b, (uint32_t*)d_s, (uint32_t*)d_s_inv, (const uint32_t*)d_h_weight, (uint32_t*)d_scal_l,
                       (uint32_t*)d_scal_r);
    ZK_HIP(hipGetLastError());
    if (!write) return ZK_OK;

    const uint64_t h = m >> 1;
    FrSum<P> sum;
    ZK_HIP_RC(sum.alloc(fr_blocks(h), 2));
    hipLaunchKernelGGL(ipa_cross_kernel<P>, dim3(sum.blocks), dim3(MLE_TILE), 0, st, h, (const uint32_t*)d_a, (const uint32_t*)d_b, sum.part());
    return sum.finish(cross, st);
}

template <class P>
static int ipa_verify_scalars_impl(int log_n, const uint64_t* u, const uint64_t* u_inv, const uint64_t* a, const uint64_t* b, void* d_out,
                                   hipStream_t st) {
    if (log_n < 0 || log_n > IPA_MAX_LOG) return fail(ZK_ERR_ARG, "ipa_verify_scalars: need 0 <= log_n <= 22");
    if (!a || !b || !d_out || (log_n && (!u || !u_inv))) return fail(ZK_ERR_ARG, "ipa_verify_scalars: null argument");
    IpaVerifyArgs<P> v;
    v.c = ipa_chain_fill<P>(log_n, u, u_inv);
    v.a = fr_canon<P>(a);   // the start of a chain of products
    v.b = fr_canon<P>(b);
    const uint64_t n = 1ull << log_n;
    hipLaunchKernelGGL(ipa_verify_scalars_kernel<P>, dim3(fr_blocks(n)), dim3(MLE_TILE), 0, st, n, log_n, v, (uint32_t*)d_out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_ipa_round_dev(int curve, int log_n, int k, void* d_a, void* d_b, void* d_s, void* d_s_inv, const uint64_t* u, const uint64_t* u_inv,
                     void* d_scal_L, void* d_scal_R, uint64_t* cross, void* stream) {
    return zk_ipa_round_seeded_dev(curve, log_n, k, d_a, d_b, d_s, d_s_inv, nullptr, u, u_inv, d_scal_L, d_scal_R, cross, stream);
}

int zk_ipa_round_seeded_dev(int curve, int log_n, int k, void* d_a, void* d_b, void* d_s, void* d_s_inv, const void* d_h_weight,
                            const uint64_t* u, const uint64_t* u_inv, void* d_scal_L, void* d_scal_R, uint64_t* cross, void* stream) {
#define CALL(P) return ipa_round_impl<P>(log_n, k, d_a, d_b, d_s, d_s_inv, d_h_weight, u, u_inv, d_scal_L, d_scal_R, cross, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_ipa_verify_scalars_dev(int curve, int log_n, const uint64_t* u, const uint64_t* u_inv, const uint64_t* a, const uint64_t* b,
                              void* d_out, void* stream) {
#define CALL(P) return ipa_verify_scalars_impl<P>(log_n, u, u_inv, a, b, d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

}  // extern "C"
