// pcs.hip -- the scalar side of the inner-product polynomial commitment's opening (BCMS20 appendix A) over BN254 Fr /
// BLS12-381 Fr (gfx950).
//
// Stands in for the per-round list arithmetic of IPA.open / IPA.verify (python/zksnake/commitment/polynomial/ipa.py:104-151,
// :191-217).  This halving argument differs from the Bulletproofs one of ipa.hip: ONE generator vector, asymmetric folds
// (c' = c_lo + u^-1 c_hi, G' = G_lo + u G_hi, b' = b_lo + u b_hi) and b = the powers of the opening point z.  The reference folds G
// and b every round; here neither exists as a vector.  With s_i = prod_{t<k} (bit (log_n-1-t) of i ? u_t : 1) the folded generator
// is G^(k)_j = sum_{i = j mod m} s_i G_i, so every L_k, R_k is an MSM over the ORIGINAL G whose scalars this file writes, and the
// folded b^(k)_j is B_k z^j with ONE scalar B_k the host keeps, so the round's two inner products are two evaluations at z of
// halves of c.
//
// Like ipa.hip the kernels multiply canonical data by scalars carried in Montgomery form (mont(x, s R) = x s): no vector is ever
// converted.  z^j comes per thread from the squarings of fr_powers.hip.h.  Workgroups of MLE_TILE threads on the capped grid of
// fr_sum.hip.h; the two evaluations are per-workgroup partial sums added by one workgroup.
#include "fr_powers.hip.h"

namespace zkmi {

constexpr int PCS_MAX_LOG = ZK_PCS_MAX_LOG;

// in place, j < m: c[j] += u^-1 c[j+m].  Element j is read and written by one thread only, element j+m only read.
template <class P>
__global__ __launch_bounds__(MLE_TILE) void pcs_fold_kernel(uint64_t m, Fp<P> ui_m, uint32_t* c) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t j = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; j < m; j += stride) {
        const Fp<P> lo = load_fr<P>(c + j * P::W), hi = load_fr<P>(c + (j + m) * P::W);
        store_fr<P>(c + j * P::W, fp_reduce_full<P>(fp_add<P>(lo, fp_mul<P>(hi, ui_m))));
    }
}

// i < n: s[i] takes the challenge of the round before where its bit is set (init: it becomes 1), and -- write != 0, m >= 2 live
// elements of c -- the n scalars of L and of R are written, zeros included.  With j = i mod m, h = m / 2 the partner of j is j ^ h.
template <class P>
__global__ __launch_bounds__(MLE_TILE) void pcs_scalars_kernel(uint64_t n, uint64_t m, int shift, int init, int write, Fp<P> u_m,
                                                               const uint32_t* __restrict__ c, uint32_t* __restrict__ s,
                                                               uint32_t* __restrict__ scal_l, uint32_t* __restrict__ scal_r) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    const Fp<P> r2 = fp_const<P>(P::R2), zero = fp_zero<P>();
    for (uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; i < n; i += stride) {
        Fp<P> sv;
        if (init) {
            sv = fp_raw_one<P>();
            store_fr<P>(s + i * P::W, sv);
        } else {
            sv = load_fr<P>(s + i * P::W);
            if ((i >> shift) & 1) {
                sv = fp_reduce_full<P>(fp_mul<P>(sv, u_m));
                store_fr<P>(s + i * P::W, sv);
            }
        }
        if (!write) continue;
        const uint64_t h = m >> 1, j = i & (m - 1), p = j ^ h;
        const bool upper = (j & h) != 0;
        const Fp<P> pc = fp_reduce_full<P>(fp_mul<P>(load_fr<P>(c + p * P::W), fp_mul<P>(sv, r2)));
        store_fr<P>(scal_l + i * P::W, upper ? zero : pc);   // c_hi against G_lo
        store_fr<P>(scal_r + i * P::W, upper ? pc : zero);   // c_lo against G_hi
    }
}

// partial[2 blk] = sum c[j+h] z^j, partial[2 blk + 1] = sum c[j] z^j over the workgroup's j < h.  z^j is in Montgomery form, so a
// term is the canonical product: nothing to close.
template <class P>
__global__ __launch_bounds__(MLE_TILE) void pcs_evals_kernel(uint64_t h, int seed_bits, RpPowers<P> z, const uint32_t* __restrict__ c,
                                                             uint32_t* __restrict__ partial) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    const Fp<P> z_step = z.sq[RP_SEED_BITS];
    uint64_t j = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x;
    Fp<P> zj = rp_power<P>(z, j, seed_bits, fp_one<P>());
    Fp<P> hi = fp_zero<P>(), lo = hi;
    for (; j < h; j += stride) {
        hi = fp_add<P>(hi, fp_mul<P>(load_fr<P>(c + (j + h) * P::W), zj));
        lo = fp_add<P>(lo, fp_mul<P>(load_fr<P>(c + j * P::W), zj));
        zj = fp_mul<P>(zj, z_step);
    }
    uint32_t* dst = partial + (size_t)blockIdx.x * 2 * P::W;
    block_sum_store<P>(hi, lds, dst);
    block_sum_store<P>(lo, lds, dst + P::W);
}

template <class P>
struct PcsVerifyArgs {
    Fp<P> u_m[PCS_MAX_LOG];   // u_t R; zero past log_n
    Fp<P> c;                  // the proof's scalar, below 2r
};

// out[i] = c s_i: one product per set bit of i, the chain starting at the canonical c
template <class P>
__global__ __launch_bounds__(MLE_TILE) void pcs_verify_scalars_kernel(uint64_t n, int log_n, PcsVerifyArgs<P> v, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; i < n; i += stride) {
        Fp<P> sc = v.c;
        for (int t = 0; t < log_n; ++t)
            if ((i >> (log_n - 1 - t)) & 1) sc = fp_mul<P>(sc, v.u_m[t]);
        store_fr<P>(out + i * P::W, fp_reduce_full<P>(sc));
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------

template <class P>
static int pcs_round_impl(int log_n, int k, void* d_c, void* d_s, const uint64_t* u, const uint64_t* u_inv, const uint64_t* z, void* d_scal_l,
                          void* d_scal_r, uint64_t* evals, hipStream_t st) {
    if (log_n < 0 || log_n > PCS_MAX_LOG || k < 0 || k > log_n) return fail(ZK_ERR_ARG, "pcs_round: need 0 <= k <= log_n <= 21");
    if (!d_c || !d_s) return fail(ZK_ERR_ARG, "pcs_round: null vector");
    if (k == 0 ? (u || u_inv) : (!u || !u_inv)) return fail(ZK_ERR_ARG, "pcs_round: a challenge goes with every round but the first, and only those");
    const bool write = k < log_n;
    if (write && (!z || !d_scal_l || !d_scal_r || !evals)) return fail(ZK_ERR_ARG, "pcs_round: null point or output");
    const uint64_t eb = P::W * 4, n = 1ull << log_n, m = n >> k;
    const void* buf[4] = {d_c, d_s, write ? d_scal_l : nullptr, write ? d_scal_r : nullptr};
    const uint64_t len[4] = {n * eb, n * eb, n * eb, n * eb};
    for (int x = 1; x < 4; ++x)   // every buffer against the ones before it
        if (buf[x] && overlaps_any(buf[x], len[x], buf, len, x)) return fail(ZK_ERR_ARG, "pcs_round: two buffers overlap");

    Fp<P> u_m = fp_zero<P>();
    if (k) {
        u_m = fr_mont<P>(u);
        hipLaunchKernelGGL(pcs_fold_kernel<P>, dim3(fr_blocks(m)), dim3(MLE_TILE), 0, st, m, fr_mont<P>(u_inv), (uint32_t*)d_c);
        ZK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(pcs_scalars_kernel<P>, dim3(fr_blocks(n)), dim3(MLE_TILE), 0, st, n, m, log_n - k, k == 0 ? 1 : 0, write ? 1 : 0, u_m,
                       (const uint32_t*)d_c, (uint32_t*)d_s, (uint32_t*)d_scal_l, (uint32_t*)d_scal_r);
    ZK_HIP(hipGetLastError());
    if (!write) return ZK_OK;

    const uint64_t h = m >> 1;
    FrSum<P> sum;
    ZK_HIP_RC(sum.alloc(fr_blocks(h), 2));
    hipLaunchKernelGGL(pcs_evals_kernel<P>, dim3(sum.blocks), dim3(MLE_TILE), 0, st, h, std::min(log_n - k - 1, RP_SEED_BITS), rp_squarings<P>(z),
                       (const uint32_t*)d_c, sum.part());
    return sum.finish(evals, st);
}

template <class P>
static int pcs_verify_scalars_impl(int log_n, const uint64_t* u, const uint64_t* c, void* d_out, hipStream_t st) {
    if (log_n < 0 || log_n > PCS_MAX_LOG) return fail(ZK_ERR_ARG, "pcs_verify_scalars: need 0 <= log_n <= 21");
    if (!c || !d_out || (log_n && !u)) return fail(ZK_ERR_ARG, "pcs_verify_scalars: null argument");
    PcsVerifyArgs<P> v;
    for (int t = 0; t < PCS_MAX_LOG; ++t) v.u_m[t] = t < log_n ? fr_mont<P>(u + 4 * t) : fp_zero<P>();
    v.c = fr_canon<P>(c);   // the start of a chain of products
    const uint64_t n = 1ull << log_n;
    hipLaunchKernelGGL(pcs_verify_scalars_kernel<P>, dim3(fr_blocks(n)), dim3(MLE_TILE), 0, st, n, log_n, v, (uint32_t*)d_out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_pcs_round_dev(int curve, int log_n, int k, void* d_c, void* d_s, const uint64_t* u, const uint64_t* u_inv, const uint64_t* z,
                     void* d_scal_L, void* d_scal_R, uint64_t* evals, void* stream) {
#define CALL(P) return pcs_round_impl<P>(log_n, k, d_c, d_s, u, u_inv, z, d_scal_L, d_scal_R, evals, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_pcs_verify_scalars_dev(int curve, int log_n, const uint64_t* u, const uint64_t* c, void* d_out, void* stream) {
#define CALL(P) return pcs_verify_scalars_impl<P>(log_n, u, c, d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

}  // extern "C"
