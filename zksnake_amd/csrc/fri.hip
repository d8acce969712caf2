// fri.hip -- the three passes a FRI polynomial commitment adds to the NTT and the Merkle kernels, over BN254 Fr / BLS12-381 Fr
// (gfx950): the low-degree extension onto a coset in pair order, one halving fold, and a gather of rows by index.
//
// The reference has no FRI; the protocol is the one of zksnake_amd/commitment/polynomial/fri.py (include/zkmi.h has the
// contracts).  A layer f of M = 2h values on the coset s <w> is stored in PAIR ORDER, g[2j] = f[j], g[2j+1] = f[j+h]: the two
// values at x_j = s w^j and at -x_j are the 64 bytes of leaf j of the layer's Merkle tree, hashed in place by
// zk_blake2b_rows_dev, and the fold reads them with contiguous loads:
//     f'[j] = (f[j] + f[j+h]) / 2 + alpha (f[j] - f[j+h]) / (2 s w^j),   j < h.
//
// Like pcs.hip the kernels multiply canonical data by scalars carried in Montgomery form (mont(x, s R) = x s): no vector is
// ever converted.  shift^i and w^-j come per thread from the squarings of fr_powers.hip.h, the fold's constant alpha / (2 s)
// is the start of that chain, so a folded value costs two products and the step of the power.  Workgroups of MLE_TILE threads
// on the capped grid of fr_sum.hip.h; plain C++, no atomics, no LDS.
#include "fr_powers.hip.h"

namespace zkmi {

constexpr int FRI_MAX_LOG = ZK_FRI_MAX_LOG;
constexpr uint64_t FRI_MAX_ROW_BYTES = ZK_FRI_MAX_ROW_BYTES;

// i < size: work[i] = c[i] shift^i for i < n_coeffs, zero beyond
template <class P>
__global__ __launch_bounds__(MLE_TILE) void fri_scale_kernel(uint64_t size, uint64_t n_coeffs, int seed_bits, RpPowers<P> shift,
                                                             const uint32_t* __restrict__ c, uint32_t* __restrict__ work) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    const Fp<P> step = shift.sq[RP_SEED_BITS], zero = fp_zero<P>();
    uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x;
    Fp<P> si = rp_power<P>(shift, i, seed_bits, fp_one<P>());
    for (; i < size; i += stride) {
        store_fr<P>(work + i * P::W, i < n_coeffs ? fp_reduce_full<P>(fp_mul<P>(load_fr<P>(c + i * P::W), si)) : zero);
        si = fp_mul<P>(si, step);
    }
}

// natural order -> pair order, j < h: out[2j] = f[j], out[2j+1] = f[j+h].  A thread writes one 64-byte pair.
template <class P>
__global__ __launch_bounds__(MLE_TILE) void fri_pairs_kernel(uint64_t h, const uint32_t* __restrict__ f, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t j = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; j < h; j += stride) {
        const Fp<P> lo = load_fr<P>(f + j * P::W), hi = load_fr<P>(f + (j + h) * P::W);
        store_fr<P>(out + 2 * j * P::W, lo);
        store_fr<P>(out + (2 * j + 1) * P::W, hi);
    }
}

// pair j < h of a layer of 2h values -> value j of the next layer, stored at its place in the pair order of h values (a layer
// of one value is that value).  c_m = alpha / (2 s) R, half_m = R / 2, w = the squarings of the layer's w^-1.
template <class P>
__global__ __launch_bounds__(MLE_TILE) void fri_fold_kernel(uint64_t h, int seed_bits, RpPowers<P> w, Fp<P> c_m, Fp<P> half_m,
                                                            const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE, h2 = h >> 1;
    const Fp<P> step = w.sq[RP_SEED_BITS];
    uint64_t j = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x;
    Fp<P> t = rp_power<P>(w, j, seed_bits, c_m);   // alpha / (2 s w^j), Montgomery form
    for (; j < h; j += stride) {
        const Fp<P> a = load_fr<P>(in + 2 * j * P::W), b = load_fr<P>(in + (2 * j + 1) * P::W);
        const Fp<P> v = fp_add<P>(fp_mul<P>(fp_add<P>(a, b), half_m), fp_mul<P>(fp_sub<P>(a, b), t));
        const uint64_t pos = h == 1 ? 0 : (j < h2 ? 2 * j : 2 * (j - h2) + 1);
        store_fr<P>(out + pos * P::W, fp_reduce_full<P>(v));
        t = fp_mul<P>(t, step);
    }
}

// chunk e of the output: 16 bytes of row min(indices[e / chunks], n_rows - 1)
__global__ __launch_bounds__(MLE_TILE) void fri_rows_kernel(uint64_t n_rows, uint64_t chunks, const uint4* __restrict__ rows, uint64_t k,
                                                            const uint64_t* __restrict__ indices, uint4* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE, items = k * chunks;
    for (uint64_t e = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; e < items; e += stride) {
        const uint64_t q = e / chunks, c = e - q * chunks, idx = indices[q];
        out[e] = rows[(idx < n_rows ? idx : n_rows - 1) * chunks + c];
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------

// 1 / 2 = (r + 1) / 2 as limbs: (r - 1) / 2 + 1
template <class P>
static Fp<P> fri_half_mont() {
    uint32_t w[P::W];
    uint64_t carry = 1;
    for (int i = 0; i < P::W; ++i) {
        carry += P::HALF[i];
        w[i] = (uint32_t)carry;
        carry >>= 32;
    }
    return fp_from_canonical<P>(w);
}

template <class P>
static int fri_lde_impl(int curve, int log_n, int log_blowup, uint64_t n_coeffs, const void* d_coeffs, const uint64_t* shift, void* d_work,
                        void* d_out, hipStream_t st) {
    if (log_n < 0 || log_blowup < 1 || log_n > FRI_MAX_LOG || log_blowup > FRI_MAX_LOG || log_n + log_blowup > FRI_MAX_LOG)
        return fail(ZK_ERR_ARG, "fri_lde: need log_n >= 0, log_blowup >= 1 and log_n + log_blowup <= 26");
    if (n_coeffs > (1ull << log_n)) return fail(ZK_ERR_ARG, "fri_lde: more than 2^log_n coefficients");
    if (!shift || !d_work || !d_out || (!d_coeffs && n_coeffs)) return fail(ZK_ERR_ARG, "fri_lde: null pointer");
    if (!aligned16(d_coeffs) || !aligned16(d_work) || !aligned16(d_out))
        return fail(ZK_ERR_ARG, "fri_lde: vectors start at a multiple of 16");
    const int log_size = log_n + log_blowup;
    const uint64_t eb = P::W * 4, size = 1ull << log_size, h = size >> 1;
    const void* buf[3] = {n_coeffs ? d_coeffs : nullptr, d_work, d_out};
    const uint64_t len[3] = {n_coeffs * eb, size * eb, size * eb};
    for (int x = 1; x < 3; ++x)   // every buffer against the ones before it
        if (overlaps_any(buf[x], len[x], buf, len, x)) return fail(ZK_ERR_ARG, "fri_lde: two buffers overlap");
    hipLaunchKernelGGL(fri_scale_kernel<P>, dim3(fr_blocks(size)), dim3(MLE_TILE), 0, st, size, n_coeffs, std::min(log_size, RP_SEED_BITS),
                       rp_squarings<P>(shift), (const uint32_t*)d_coeffs, (uint32_t*)d_work);
    ZK_HIP(hipGetLastError());
    ZK_HIP_RC(zk_ntt_dev(curve, 0, log_size, d_work, (void*)st));
    hipLaunchKernelGGL(fri_pairs_kernel<P>, dim3(fr_blocks(h)), dim3(MLE_TILE), 0, st, h, (const uint32_t*)d_work, (uint32_t*)d_out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int fri_fold_impl(int log_m, const void* d_in, const uint64_t* c, const uint64_t* w_inv, void* d_out, hipStream_t st) {
    if (log_m < 1 || log_m > FRI_MAX_LOG) return fail(ZK_ERR_ARG, "fri_fold: need 1 <= log_m <= 26");
    if (!d_in || !d_out || !c || !w_inv) return fail(ZK_ERR_ARG, "fri_fold: null pointer");
    if (!aligned16(d_in) || !aligned16(d_out)) return fail(ZK_ERR_ARG, "fri_fold: layers start at a multiple of 16");
    const uint64_t eb = P::W * 4, h = 1ull << (log_m - 1);
    const void* in[1] = {d_in};
    const uint64_t len[1] = {2 * h * eb};
    if (overlaps_any(d_out, h * eb, in, len, 1)) return fail(ZK_ERR_ARG, "fri_fold: the folded layer overlaps the layer");
    hipLaunchKernelGGL(fri_fold_kernel<P>, dim3(fr_blocks(h)), dim3(MLE_TILE), 0, st, h, std::min(log_m - 1, RP_SEED_BITS), rp_squarings<P>(w_inv),
                       fr_mont<P>(c), fri_half_mont<P>(), (const uint32_t*)d_in, (uint32_t*)d_out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

static int fri_rows(uint64_t n_rows, uint64_t row_bytes, const void* d_rows, uint64_t k, const void* d_indices, void* d_out, hipStream_t st) {
    if (n_rows == 0 || n_rows > (1ull << 32)) return fail(ZK_ERR_ARG, "fri_rows: need 1 <= n_rows <= 2^32");
    if (row_bytes == 0 || row_bytes > FRI_MAX_ROW_BYTES || (row_bytes & 15))
        return fail(ZK_ERR_ARG, "fri_rows: a row is a multiple of 16 bytes, at most 2^16");
    if (k > (1ull << 32)) return fail(ZK_ERR_ARG, "fri_rows: at most 2^32 rows a call");
    if (!d_rows) return fail(ZK_ERR_ARG, "fri_rows: null rows");
    if (k == 0) return ZK_OK;
    if (!d_indices || !d_out) return fail(ZK_ERR_ARG, "fri_rows: null pointer");
    if (!aligned16(d_rows) || !aligned16(d_out) || ((uintptr_t)d_indices & 7))
        return fail(ZK_ERR_ARG, "fri_rows: rows and output start at a multiple of 16, the indices at a multiple of 8");
    const void* in[2] = {d_rows, d_indices};
    const uint64_t len[2] = {n_rows * row_bytes, k * 8};
    if (overlaps_any(d_out, k * row_bytes, in, len, 2)) return fail(ZK_ERR_ARG, "fri_rows: the output overlaps an input");
    const uint64_t chunks = row_bytes / 16;
    hipLaunchKernelGGL(fri_rows_kernel, dim3(fr_blocks(k * chunks)), dim3(MLE_TILE), 0, st, n_rows, chunks, (const uint4*)d_rows, k,
                       (const uint64_t*)d_indices, (uint4*)d_out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_fri_lde_dev(int curve, int log_n, int log_blowup, uint64_t n_coeffs, const void* d_coeffs, const uint64_t* shift, void* d_work,
                   void* d_out, void* stream) {
#define CALL(P) return fri_lde_impl<P>(curve, log_n, log_blowup, n_coeffs, d_coeffs, shift, d_work, d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_fri_fold_dev(int curve, int log_m, const void* d_in, const uint64_t* c, const uint64_t* w_inv, void* d_out, void* stream) {
#define CALL(P) return fri_fold_impl<P>(log_m, d_in, c, w_inv, d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_fri_rows_dev(uint64_t n_rows, uint64_t row_bytes, const void* d_rows, uint64_t k, const void* d_indices, void* d_out, void* stream) {
    return fri_rows(n_rows, row_bytes, d_rows, k, d_indices, d_out, (hipStream_t)stream);
}

}  // extern "C"
