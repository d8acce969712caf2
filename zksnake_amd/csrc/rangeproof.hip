// rangeproof.hip -- the scalar side of a Bulletproofs range proof, single or aggregated, over BN254 Fr / BLS12-381 Fr (gfx950).
//
// Stands in for the list arithmetic of RangeProof.prove / .verify (python/zksnake/subprotocol/bulletproofs/range_proof.py:
// 114-190, :262-280), generalised from one value of n bits to m values in one argument over N = n m positions: position
// k = j n + i is bit i of value j, and value j is weighted by z^(2+j) where the reference has z^2.  Four passes: the bit vectors
// a_L || a_R (the scalars of A), the three coefficients of t(X) in one pass with three sums, l || r at the challenge x together
// with the weights y^-k the inner-product argument seeds its s_inv vector with (ipa.hip), and the verifier's 2N scalars.
//
// Powers.  Every element needs y^k (or y^-k) and z^(2+j).  They are NOT read from tables: the squarings g^(2^t), t <= 18, travel
// as kernel arguments, a thread builds the power of its first index from them (one product per set bit; bits 6 and up are the
// same across a wave, so those branches are uniform) and steps by g^(2^18) per grid-stride item -- the stride is 2^18 whenever a
// thread takes a second item, and it is a multiple of n, so z^(2+j) steps by a fixed power too (RpPowers / rp_power / rp_squarings,
// fr_powers.hip.h, shared with pcs.hip).  2^i is the integer with bit i set, written into its limb: no product.  DESIGN 4.10 has
// the count of products and bytes per element against the tables.
//
// Like ipa.hip the kernels keep data canonical and carry host scalars in Montgomery form: mont(x, s R) = x s.  A product of two
// canonical values carries R^-1, which the sums close once per thread with R^2.
#include "fr_powers.hip.h"
#include "ipa_chain.hip.h"

namespace zkmi {

constexpr int RP_MAX_BITS_LOG = 7;           // bitsize <= 128: 2^i stays a plain integer below r

// the integer 2^i, i < 128, as limbs (no limb is indexed by a register: the selects keep the element in VGPRs)
template <class P>
__device__ __forceinline__ Fp<P> rp_two_pow(unsigned i) {
    const unsigned limb = i / LIMB_BITS, bit = 1u << (i % LIMB_BITS);
    Fp<P> o;
#pragma unroll
    for (int l = 0; l < P::N; ++l) o.v[l] = (unsigned)l == limb ? bit : 0u;
    return o;
}

// bit i of value j for k = j n + i; a value is two 64-bit limbs, low first
__device__ __forceinline__ bool rp_bit(const uint64_t* __restrict__ values, uint64_t k, int log_bits) {
    const uint64_t j = k >> log_bits;
    const unsigned i = (unsigned)(k & ((1u << log_bits) - 1));
    return (values[2 * j + (i >> 6)] >> (i & 63)) & 1;
}

// out[k] = a_L[k], out[N+k] = a_R[k] = a_L[k] - 1: the two canonical constants 1 | 0 and 0 | r-1
template <class P>
__global__ __launch_bounds__(MLE_TILE) void rp_bits_kernel(uint64_t n_pos, int log_bits, const uint64_t* __restrict__ values,
                                                           uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    const Fp<P> zero = fp_zero<P>(), one = fp_raw_one<P>();
    Fp<P> minus_one = fp_const<P>(P::M);
    minus_one.v[0] -= 1;   // r is odd
    for (uint64_t k = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; k < n_pos; k += stride) {
        const bool bit = rp_bit(values, k, log_bits);
        store_fr<P>(out + k * P::W, bit ? one : zero);
        store_fr<P>(out + (n_pos + k) * P::W, bit ? zero : minus_one);
    }
}

// what the two prover passes share.  l0 and a_R + z take one of two values each, chosen by the bit: canonical, below 2r.
template <class P>
struct RpProverArgs {
    RpPowers<P> y, z;
    Fp<P> z2_m;               // z^2 R: the weight of value 0
    Fp<P> l0[2];              // -z, 1 - z
    Fp<P> ar_z[2];            // z - 1, z
};

// partial[3 blk + c] = the workgroup's share of t_c:  t0 = <l0, r0>, t1 = <l0, r1> + <l1, r0>, t2 = <l1, r1> with
// l1 = s_L, r0[k] = y^k (a_R[k] + z) + z^(2+j) 2^i, r1[k] = y^k s_R[k].  7 products per element (t1's two share a reduction).
template <class P>
__global__ __launch_bounds__(MLE_TILE) void rp_poly_kernel(uint64_t n_pos, int log_bits, int seed_bits, RpProverArgs<P> c,
                                                           const uint64_t* __restrict__ values, const uint32_t* __restrict__ s,
                                                           uint32_t* __restrict__ partial) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    const Fp<P> y_step = c.y.sq[RP_SEED_BITS], z_step = c.z.sq[RP_SEED_BITS - log_bits];
    uint64_t k = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x;
    Fp<P> yk = rp_power<P>(c.y, k, seed_bits, fp_one<P>());
    Fp<P> zj = rp_power<P>(c.z, k >> log_bits, seed_bits - log_bits, c.z2_m);
    Fp<P> t0 = fp_zero<P>(), t1 = t0, t2 = t0;
    for (; k < n_pos; k += stride) {
        const bool bit = rp_bit(values, k, log_bits);
        const unsigned i = (unsigned)(k & ((1u << log_bits) - 1));
        const Fp<P> l1 = load_fr<P>(s + k * P::W), sr = load_fr<P>(s + (n_pos + k) * P::W);
        const Fp<P> l0 = bit ? c.l0[1] : c.l0[0];
        const Fp<P> r0 = fp_add<P>(fp_mul<P>(yk, bit ? c.ar_z[1] : c.ar_z[0]), fp_mul<P>(zj, rp_two_pow<P>(i)));
        const Fp<P> r1 = fp_mul<P>(yk, sr);
        t0 = fp_add<P>(t0, fp_mul<P>(l0, r0));
        t1 = fp_add<P>(t1, fp_mul2<P>(l0, r1, l1, r0));
        t2 = fp_add<P>(t2, fp_mul<P>(l1, r1));
        yk = fp_mul<P>(yk, y_step);
        zj = fp_mul<P>(zj, z_step);
    }
    const Fp<P> r2 = fp_const<P>(P::R2);   // every term carries R^-1: closed once per thread
    uint32_t* dst = partial + (size_t)blockIdx.x * 3 * P::W;
    block_sum_store<P>(fp_mul<P>(t0, r2), lds, dst);
    block_sum_store<P>(fp_mul<P>(t1, r2), lds, dst + P::W);
    block_sum_store<P>(fp_mul<P>(t2, r2), lds, dst + 2 * P::W);
}

// ab[k] = l[k] = l0 + x s_L,  ab[N+k] = r[k] = y^k (a_R + z + x s_R) + z^(2+j) 2^i,  h_weight[k] = y_inv^k.
// 7 products per element: x s_L, x s_R, the two of r, y_inv^k into canonical form and the two steps (a third for z^(2+j)).
template <class P>
__global__ __launch_bounds__(MLE_TILE) void rp_eval_kernel(uint64_t n_pos, int log_bits, int seed_bits, RpProverArgs<P> c, RpPowers<P> y_inv,
                                                           Fp<P> x_m, const uint64_t* __restrict__ values, const uint32_t* __restrict__ s,
                                                           uint32_t* __restrict__ ab, uint32_t* __restrict__ h_weight) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    const Fp<P> y_step = c.y.sq[RP_SEED_BITS], yi_step = y_inv.sq[RP_SEED_BITS], z_step = c.z.sq[RP_SEED_BITS - log_bits];
    const Fp<P> one = fp_raw_one<P>();
    uint64_t k = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x;
    Fp<P> yk = rp_power<P>(c.y, k, seed_bits, fp_one<P>());
    Fp<P> yik = rp_power<P>(y_inv, k, seed_bits, fp_one<P>());
    Fp<P> zj = rp_power<P>(c.z, k >> log_bits, seed_bits - log_bits, c.z2_m);
    for (; k < n_pos; k += stride) {
        const bool bit = rp_bit(values, k, log_bits);
        const unsigned i = (unsigned)(k & ((1u << log_bits) - 1));
        const Fp<P> sl = load_fr<P>(s + k * P::W), sr = load_fr<P>(s + (n_pos + k) * P::W);
        const Fp<P> l = fp_add<P>(bit ? c.l0[1] : c.l0[0], fp_mul<P>(sl, x_m));
        const Fp<P> inner = fp_add<P>(bit ? c.ar_z[1] : c.ar_z[0], fp_mul<P>(sr, x_m));
        const Fp<P> r = fp_add<P>(fp_mul<P>(yk, inner), fp_mul<P>(zj, rp_two_pow<P>(i)));
        store_fr<P>(ab + k * P::W, fp_reduce_full<P>(l));
        store_fr<P>(ab + (n_pos + k) * P::W, fp_reduce_full<P>(r));
        store_fr<P>(h_weight + k * P::W, fp_reduce_full<P>(fp_mul<P>(yik, one)));
        yk = fp_mul<P>(yk, y_step);
        yik = fp_mul<P>(yik, yi_step);
        zj = fp_mul<P>(zj, z_step);
    }
}

template <class P>
struct RpVerifyArgs {
    IpaChain<P> c;              // first: the layout of the argument block is the flat one's
    RpPowers<P> y_inv, z;
    Fp<P> a, b;                 // the proof's scalars, below 2r
    Fp<P> z2_m, z_c, neg_z;     // z^2 R; z and -z, canonical, below 2r
};

// out[k] = -z - a s_k,  out[N+k] = z + y_inv^k (z^(2+j) 2^i - b s_k^-1): the challenge chain of ipa_chain.hip.h (2 log N products)
// and 4 more per element
template <class P>
__global__ __launch_bounds__(MLE_TILE) void rp_verify_scalars_kernel(uint64_t n_pos, int log_n, int log_bits, int seed_bits, RpVerifyArgs<P> v,
                                                                     uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    const Fp<P> yi_step = v.y_inv.sq[RP_SEED_BITS], z_step = v.z.sq[RP_SEED_BITS - log_bits];
    uint64_t k = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x;
    Fp<P> yik = rp_power<P>(v.y_inv, k, seed_bits, fp_one<P>());
    Fp<P> zj = rp_power<P>(v.z, k >> log_bits, seed_bits - log_bits, v.z2_m);
    for (; k < n_pos; k += stride) {
        const unsigned i = (unsigned)(k & ((1u << log_bits) - 1));
        Fp<P> sa = v.a, sb = v.b;
        ipa_chain_run<P>(v.c, log_n, k, sa, sb);
        const Fp<P> h = fp_mul<P>(yik, fp_sub<P>(fp_mul<P>(zj, rp_two_pow<P>(i)), sb));
        store_fr<P>(out + k * P::W, fp_reduce_full<P>(fp_sub<P>(v.neg_z, sa)));
        store_fr<P>(out + (n_pos + k) * P::W, fp_reduce_full<P>(fp_add<P>(v.z_c, h)));
        yik = fp_mul<P>(yik, yi_step);
        zj = fp_mul<P>(zj, z_step);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------

static int rp_check_sizes(const char* who, int log_bits, int log_n) {
    if (log_bits < 0 || log_bits > RP_MAX_BITS_LOG || log_n < log_bits || log_n > ZK_IPA_MAX_LOG)
        return fail(ZK_ERR_ARG, std::string(who) + ": need 0 <= log_bits <= 7 and log_bits <= log_N <= 22");
    return ZK_OK;
}

template <class P>
static RpProverArgs<P> rp_prover_args(const uint64_t* y, const uint64_t* z) {
    RpProverArgs<P> c;
    c.y = rp_squarings<P>(y);
    c.z = rp_squarings<P>(z);
    c.z2_m = c.z.sq[1];
    const Fp<P> one = fp_raw_one<P>(), zc = fr_canon<P>(z);
    c.l0[0] = fp_neg<P>(zc);
    c.l0[1] = fp_sub<P>(one, zc);
    c.ar_z[0] = fp_sub<P>(zc, one);
    c.ar_z[1] = zc;
    return c;
}

static int rp_seed_bits(int log_n) { return std::min(log_n, RP_SEED_BITS); }

template <class P>
static int rp_bits_impl(int log_bits, int log_n, const void* d_values, void* d_out, hipStream_t st) {
    ZK_HIP_RC(rp_check_sizes("rp_bits", log_bits, log_n));
    if (!d_values || !d_out) return fail(ZK_ERR_ARG, "rp_bits: null pointer");
    const uint64_t n_pos = 1ull << log_n, m = n_pos >> log_bits;
    if (ranges_overlap(d_values, m * 16, d_out, 2 * n_pos * P::W * 4)) return fail(ZK_ERR_ARG, "rp_bits: two buffers overlap");
    hipLaunchKernelGGL(rp_bits_kernel<P>, dim3(fr_blocks(n_pos)), dim3(MLE_TILE), 0, st, n_pos, log_bits, (const uint64_t*)d_values,
                       (uint32_t*)d_out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int rp_poly_impl(int log_bits, int log_n, const void* d_values, const void* d_s, const uint64_t* y, const uint64_t* z, uint64_t* t_out,
                        hipStream_t st) {
    ZK_HIP_RC(rp_check_sizes("rp_poly", log_bits, log_n));
    if (!d_values || !d_s || !y || !z || !t_out) return fail(ZK_ERR_ARG, "rp_poly: null pointer");
    const uint64_t n_pos = 1ull << log_n;
    FrSum<P> sum;
    ZK_HIP_RC(sum.alloc(fr_blocks(n_pos), 3));
    hipLaunchKernelGGL(rp_poly_kernel<P>, dim3(sum.blocks), dim3(MLE_TILE), 0, st, n_pos, log_bits, rp_seed_bits(log_n), rp_prover_args<P>(y, z),
                       (const uint64_t*)d_values, (const uint32_t*)d_s, sum.part());
    return sum.finish(t_out, st);
}

template <class P>
static int rp_eval_impl(int log_bits, int log_n, const void* d_values, const void* d_s, const uint64_t* y, const uint64_t* y_inv, const uint64_t* z,
                        const uint64_t* x, void* d_ab, void* d_h_weight, hipStream_t st) {
    ZK_HIP_RC(rp_check_sizes("rp_eval", log_bits, log_n));
    if (!d_values || !d_s || !y || !y_inv || !z || !x || !d_ab || !d_h_weight) return fail(ZK_ERR_ARG, "rp_eval: null pointer");
    const uint64_t n_pos = 1ull << log_n, eb = P::W * 4;
    const void* buf[4] = {d_ab, d_h_weight, d_s, d_values};
    const uint64_t len[4] = {2 * n_pos * eb, n_pos * eb, 2 * n_pos * eb, (n_pos >> log_bits) * 16};
    for (int o = 0; o < 2; ++o)       // an output against everything after it
        if (overlaps_any(buf[o], len[o], buf + o + 1, len + o + 1, 3 - o)) return fail(ZK_ERR_ARG, "rp_eval: two buffers overlap");
    hipLaunchKernelGGL(rp_eval_kernel<P>, dim3(fr_blocks(n_pos)), dim3(MLE_TILE), 0, st, n_pos, log_bits, rp_seed_bits(log_n),
                       rp_prover_args<P>(y, z), rp_squarings<P>(y_inv), fr_mont<P>(x), (const uint64_t*)d_values, (const uint32_t*)d_s,
                       (uint32_t*)d_ab, (uint32_t*)d_h_weight);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int rp_verify_scalars_impl(int log_bits, int log_n, const uint64_t* u, const uint64_t* u_inv, const uint64_t* a, const uint64_t* b,
                                  const uint64_t* y_inv, const uint64_t* z, void* d_out, hipStream_t st) {
    ZK_HIP_RC(rp_check_sizes("rp_verify_scalars", log_bits, log_n));
    if (!a || !b || !y_inv || !z || !d_out || (log_n && (!u || !u_inv))) return fail(ZK_ERR_ARG, "rp_verify_scalars: null argument");
    RpVerifyArgs<P> v;
    v.c = ipa_chain_fill<P>(log_n, u, u_inv);
    v.y_inv = rp_squarings<P>(y_inv);
    v.z = rp_squarings<P>(z);
    v.a = fr_canon<P>(a);
    v.b = fr_canon<P>(b);
    v.z2_m = v.z.sq[1];
    v.z_c = fr_canon<P>(z);
    v.neg_z = fp_neg<P>(v.z_c);
    const uint64_t n_pos = 1ull << log_n;
    hipLaunchKernelGGL(rp_verify_scalars_kernel<P>, dim3(fr_blocks(n_pos)), dim3(MLE_TILE), 0, st, n_pos, log_n, log_bits, rp_seed_bits(log_n), v,
                       (uint32_t*)d_out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_rp_bits_dev(int curve, int log_bits, int log_N, const void* d_values, void* d_out, void* stream) {
#define CALL(P) return rp_bits_impl<P>(log_bits, log_N, d_values, d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_rp_poly_dev(int curve, int log_bits, int log_N, const void* d_values, const void* d_s, const uint64_t* y, const uint64_t* z,
                   uint64_t* t_out, void* stream) {
#define CALL(P) return rp_poly_impl<P>(log_bits, log_N, d_values, d_s, y, z, t_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_rp_eval_dev(int curve, int log_bits, int log_N, const void* d_values, const void* d_s, const uint64_t* y, const uint64_t* y_inv,
                   const uint64_t* z, const uint64_t* x, void* d_ab, void* d_h_weight, void* stream) {
#define CALL(P) return rp_eval_impl<P>(log_bits, log_N, d_values, d_s, y, y_inv, z, x, d_ab, d_h_weight, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_rp_verify_scalars_dev(int curve, int log_bits, int log_N, const uint64_t* u, const uint64_t* u_inv, const uint64_t* a, const uint64_t* b,
                             const uint64_t* y_inv, const uint64_t* z, void* d_out, void* stream) {
#define CALL(P) return rp_verify_scalars_impl<P>(log_bits, log_N, u, u_inv, a, b, y_inv, z, d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

}  // extern "C"
