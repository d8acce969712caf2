// frvec.hip -- element-wise vector operations over BN254 Fr / BLS12-381 Fr on gfx950: everything behind zk_vec_* and
// zk_poly_div_vanishing.  Groth16, PlonK, the inner-product argument and GKR all call them.
//
// Stands in for add/mul_over_evaluation_domain and Polynomial.divide_by_vanishing_poly of the reference
// (src/bn254/polynomial.rs:466-489, 535-634 and the bls12_381 twin) and for the Polynomial scalar multiply-adds of Plonk.prove
// (python/zksnake/plonk/protocol.py:213-460).
//
// All vectors are canonical Fr elements (32 B) in HBM; scalars cross the ABI as canonical 4-limb integers.  Products use the
// Montgomery multiplier directly on canonical data: mont(x, s*R) = x*s, so no vector is ever converted to Montgomery form.
#include "fr_sum.hip.h"

namespace zkmi {
using mem::DevBuf;

// op: 0 mul, 1 add, 2 sub on canonical data.  mul: mont(mont(a,b), R^2) = a*b
template <class P>
__global__ void vec_op_kernel(int op, uint64_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp<P> x = load_fr<P>(a + i * P::W), y = load_fr<P>(b + i * P::W), z;
    if (op == 0) z = fp_mul<P>(fp_mul<P>(x, y), fp_const<P>(P::R2));
    else if (op == 1) z = fp_add<P>(x, y);
    else z = fp_sub<P>(x, y);
    store_fr<P>(out + i * P::W, fp_reduce_full<P>(z));
}

// reduce every element below the modulus (inputs of the host API may be >= r)
template <class P>
__global__ void canon_kernel(uint64_t n, uint32_t* a) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t x[P::W];
    uint4* q = reinterpret_cast<uint4*>(a + i * P::W);
#pragma unroll
    for (int k = 0; k < P::W / 4; ++k) {
        uint4 t = q[k];
        x[4 * k] = t.x; x[4 * k + 1] = t.y; x[4 * k + 2] = t.z; x[4 * k + 3] = t.w;
    }
    for (int k = 0; k < 10; ++k) {
        uint32_t t[P::W];
        if (fp_sub_mod_raw<P>(t, x)) break;
#pragma unroll
        for (int l = 0; l < P::W; ++l) x[l] = t[l];
    }
#pragma unroll
    for (int k = 0; k < P::W / 4; ++k) q[k] = make_uint4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
}

// out[k] = g^k as canonical integers (setup: the powers of tau), square-and-multiply per element
template <class P>
__global__ void powers_kernel(uint32_t* out, Fp<P> g, uint32_t count) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    uint32_t e[1] = {k};
    Fp<P> r = fp_pow<P>(g, e, 1);
    uint32_t w[P::W];
    fp_to_canonical<P>(w, r);
    uint4* q = reinterpret_cast<uint4*>(out + (size_t)k * P::W);
#pragma unroll
    for (int i = 0; i < P::W / 4; ++i) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}

// q[j] = sum_{k>=1} c[j + k n],  rem[i] = c[i] + q[i]   (c has len coefficients)
template <class P>
__global__ void div_vanishing_kernel(uint64_t n, uint64_t len, const uint32_t* c, uint32_t* q, uint32_t* rem,
                                     int* nonzero) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t top = len < n ? len : n;
    uint64_t qlen = len > n ? len - n : 0;
    uint64_t lim = qlen > top ? qlen : top;
    if (i >= lim) return;
    // q[i] for i < qlen (may exceed n when len > 2n: then q[i] also folds further blocks)
    Fp<P> acc = fp_zero<P>();
    if (i < qlen) {
        for (uint64_t j = i + n; j < len; j += n) acc = fp_add<P>(acc, load_fr<P>(c + j * P::W));
        store_fr<P>(q + i * P::W, fp_reduce_full<P>(acc));
    }
    if (i < top) {
        Fp<P> r = fp_reduce_full<P>(fp_add<P>(load_fr<P>(c + i * P::W), acc));
        store_fr<P>(rem + i * P::W, r);
        if (!fp_is_zero<P>(r)) atomicOr(nonzero, 1);
    }
}

// out = a*x + b*y + c      (y may be null)
template <class P>
__global__ __launch_bounds__(256) void axpby_kernel(uint64_t n, Fp<P> a_m, const uint32_t* __restrict__ x, Fp<P> b_m,
                                                    const uint32_t* __restrict__ y, Fp<P> c, uint32_t* __restrict__ out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp<P> v = fp_add<P>(fp_mul<P>(load_fr<P>(x + i * P::W), a_m), c);
    if (y) v = fp_add<P>(v, fp_mul<P>(load_fr<P>(y + i * P::W), b_m));
    store_fr<P>(out + i * P::W, fp_reduce_full<P>(v));
}

// acc[i] += sum_k s_k x_k[i] (i < count_k), then acc[at_j] += c_j: a whole chain of scalar multiply-adds and single-coefficient
// updates in ONE launch (the linearisation polynomial of a PlonK proof is ten such terms, a blinding two to three updates; as
// separate launches of a few microseconds each they left the GPU idle between them: launch-bound)
constexpr int LINCOMB_MAX_TERMS = 16, LINCOMB_MAX_AT = 8;
template <class P>
struct LincombArgs {
    const uint32_t* x[LINCOMB_MAX_TERMS];
    uint64_t count[LINCOMB_MAX_TERMS];
    Fp<P> s_m[LINCOMB_MAX_TERMS];      // s R: mont(x, s R) = s x
    uint64_t at[LINCOMB_MAX_AT];
    Fp<P> at_val[LINCOMB_MAX_AT];      // canonical
    int k, n_at;
};
template <class P>
__global__ __launch_bounds__(256) void lincomb_kernel(uint64_t n, uint32_t* __restrict__ acc, LincombArgs<P> a) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp<P> v = load_fr<P>(acc + i * P::W);
    for (int t = 0; t < a.k; ++t)
        if (i < a.count[t]) v = fp_add<P>(v, fp_mul<P>(load_fr<P>(a.x[t] + i * P::W), a.s_m[t]));
    for (int j = 0; j < a.n_at; ++j)
        if (i == a.at[j]) v = fp_add<P>(v, a.at_val[j]);
    store_fr<P>(acc + i * P::W, fp_reduce_full<P>(fp_reduce_full<P>(v)));
}

// out[i] = in[offset + i * stride]: de-interleaves the flat PlonK witness [a0, b0, c0, a1, ..] into its three columns
template <class P>
__global__ __launch_bounds__(256) void gather_kernel(uint64_t n, const uint4* __restrict__ in, uint64_t stride, uint64_t offset, uint4* __restrict__ out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int V = P::W / 4;  // 16-byte vectors per element
    if (i >= n * V) return;
    const uint64_t e = i / V, part = i % V;
    out[i] = in[(offset + e * stride) * V + part];
}

template <class P>
__global__ __launch_bounds__(256) void is_zero_kernel(uint64_t n_vec4, const uint4* __restrict__ x, int* flag) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_vec4) return;
    uint4 t = x[i];
    if (t.x | t.y | t.z | t.w) atomicOr(flag, 1);
}

// ---- host side ------------------------------------------------------------------------------

template <class P>
static int vec_op_dev_impl(int op, uint64_t n, const uint32_t* a, const uint32_t* b, uint32_t* out, hipStream_t stream) {
    if (n == 0) return ZK_OK;
    hipLaunchKernelGGL(vec_op_kernel<P>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, op, n, a, b, out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int canon_impl(uint64_t n, uint32_t* x, hipStream_t stream) {
    hipLaunchKernelGGL(canon_kernel<P>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, x);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int powers_impl(uint64_t n, const uint64_t* g, uint32_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(powers_kernel<P>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, out, fr_mont<P>(g), (uint32_t)n);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int gather_impl(uint64_t n, const void* src, uint64_t stride, uint64_t offset, void* dst, hipStream_t stream) {
    if (n == 0) return ZK_OK;
    const uint64_t nv = n * (P::W / 4);
    hipLaunchKernelGGL(gather_kernel<P>, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, stream, n, (const uint4*)src, stride, offset, (uint4*)dst);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int vec_op_host_impl(int op, uint64_t size, uint64_t n_a, const uint64_t* a, uint64_t n_b, const uint64_t* b, uint64_t* out) {
    if (size == 0) return ZK_OK;
    const size_t eb = P::W * 4;
    DevBuf buf;
    ZK_HIP_RC(buf.alloc(2 * size * eb));
    uint32_t* const d = buf.as();
    ZK_HIP(hipMemset(d, 0, 2 * size * eb));
    uint64_t ca = n_a < size ? n_a : size, cb = n_b < size ? n_b : size;
    if (ca) ZK_HIP(hipMemcpy(d, a, ca * eb, hipMemcpyHostToDevice));
    if (cb) ZK_HIP(hipMemcpy(d + size * P::W, b, cb * eb, hipMemcpyHostToDevice));
    ZK_HIP_RC(canon_impl<P>(2 * size, d, 0));
    ZK_HIP_RC(vec_op_dev_impl<P>(op, size, d, d + size * P::W, d, 0));
    ZK_HIP(hipMemcpy(out, d, size * eb, hipMemcpyDeviceToHost));
    return ZK_OK;
}

template <class P>
static int div_vanishing_host_impl(uint64_t n, uint64_t len, const uint64_t* coeffs, uint64_t* q, uint64_t* rem, int* rem_is_zero) {
    if (n == 0) return fail(ZK_ERR_ARG, "vanishing polynomial of an empty domain");
    *rem_is_zero = 1;
    if (len == 0) return ZK_OK;
    const size_t eb = P::W * 4;
    uint64_t qlen = len > n ? len - n : 0, top = len < n ? len : n;
    DevBuf dc, dq, dr, dflag;
    ZK_HIP_RC(dc.alloc(len * eb));
    ZK_HIP_RC(dq.alloc((qlen ? qlen : 1) * eb));
    ZK_HIP_RC(dr.alloc(top * eb));
    ZK_HIP_RC(dflag.alloc(sizeof(int)));
    ZK_HIP(hipMemcpy(dc.as(), coeffs, len * eb, hipMemcpyHostToDevice));
    (void)hipMemset(dflag.as(), 0, sizeof(int));
    ZK_HIP_RC(canon_impl<P>(len, dc.as(), 0));
    uint64_t lim = qlen > top ? qlen : top;
    hipLaunchKernelGGL(div_vanishing_kernel<P>, dim3((unsigned)((lim + 255) / 256)), dim3(256), 0, 0, n, len, dc.as(), dq.as(), dr.as(), dflag.as<int>());
    int flag = 0;
    ZK_HIP(hipMemcpy(&flag, dflag.as(), sizeof(int), hipMemcpyDeviceToHost));
    if (qlen) ZK_HIP(hipMemcpy(q, dq.as(), qlen * eb, hipMemcpyDeviceToHost));
    ZK_HIP(hipMemcpy(rem, dr.as(), top * eb, hipMemcpyDeviceToHost));
    *rem_is_zero = flag ? 0 : 1;
    return ZK_OK;
}

template <class P>
static int axpby_impl(uint64_t n, const uint64_t* a, const void* x, const uint64_t* b, const void* y, const uint64_t* c, void* out, hipStream_t st) {
    if (n == 0) return ZK_OK;
    if (!a || !x || !out) return fail(ZK_ERR_ARG, "axpby: null argument");
    if ((b == nullptr) != (y == nullptr)) return fail(ZK_ERR_ARG, "axpby: b and y go together");
    Fp<P> am = scalar_times_r<P>(a, 1), bm = b ? scalar_times_r<P>(b, 1) : fp_zero<P>(), cc = c ? scalar_in<P>(c) : fp_zero<P>();
    hipLaunchKernelGGL(axpby_kernel<P>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, am, (const uint32_t*)x, bm,
                       (const uint32_t*)y, cc, (uint32_t*)out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int lincomb_impl(uint64_t n_acc, void* acc, int k, const uint64_t* counts, const void* const* xs, const uint64_t* scalars, int n_at,
                        const uint64_t* at_index, const uint64_t* at_vals, hipStream_t st) {
    if (k < 0 || k > LINCOMB_MAX_TERMS || n_at < 0 || n_at > LINCOMB_MAX_AT) return fail(ZK_ERR_ARG, "lincomb: at most 16 terms and 8 single updates");
    if (n_acc == 0 || (k == 0 && n_at == 0)) return ZK_OK;
    if (!acc || (k && (!counts || !xs || !scalars)) || (n_at && (!at_index || !at_vals))) return fail(ZK_ERR_ARG, "lincomb: null argument");
    LincombArgs<P> a;
    a.k = k;
    a.n_at = n_at;
    uint64_t reach = 0;   // the launch only covers what some term or update touches
    for (int t = 0; t < k; ++t) {
        if (counts[t] > n_acc) return fail(ZK_ERR_ARG, "lincomb: a term is longer than the accumulator");
        if (counts[t] && !xs[t]) return fail(ZK_ERR_ARG, "lincomb: null term");
        a.x[t] = (const uint32_t*)xs[t];
        a.count[t] = counts[t];
        a.s_m[t] = scalar_times_r<P>(scalars + 4 * t, 1);
        reach = std::max<uint64_t>(reach, counts[t]);
    }
    for (int j = 0; j < n_at; ++j) {
        if (at_index[j] >= n_acc) return fail(ZK_ERR_ARG, "lincomb: update index beyond the accumulator");
        a.at[j] = at_index[j];
        a.at_val[j] = scalar_in<P>(at_vals + 4 * j);
        reach = std::max<uint64_t>(reach, at_index[j] + 1);
    }
    hipLaunchKernelGGL(lincomb_kernel<P>, dim3((unsigned)((reach + 255) / 256)), dim3(256), 0, st, reach, (uint32_t*)acc, a);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int is_zero_impl(uint64_t n, const void* x, int* is_zero, hipStream_t st) {
    *is_zero = 1;
    if (n == 0) return ZK_OK;
    DevBuf dflag;
    ZK_HIP_RC(dflag.alloc(sizeof(int)));
    int flag = 0;
    ZK_HIP(hipMemsetAsync(dflag.as(), 0, sizeof(int), st));
    uint64_t nv = n * (P::W / 4);
    hipLaunchKernelGGL(is_zero_kernel<P>, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, nv, (const uint4*)x, dflag.as<int>());
    ZK_HIP(hipMemcpyAsync(&flag, dflag.as(), sizeof(int), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    *is_zero = flag ? 0 : 1;
    return ZK_OK;
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_vec_op(int curve, int op, uint64_t size, uint64_t n_a, const uint64_t* a, uint64_t n_b, const uint64_t* b, uint64_t* out) {
    if (op < 0 || op > 2) return fail(ZK_ERR_ARG, "unknown vector op");
#define CALL(P) return vec_op_host_impl<P>(op, size, n_a, a, n_b, b, out)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_poly_div_vanishing(int curve, uint64_t n, uint64_t len, const uint64_t* coeffs, uint64_t* q, uint64_t* rem, int* rem_is_zero) {
#define CALL(P) return div_vanishing_host_impl<P>(n, len, coeffs, q, rem, rem_is_zero)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_vec_op_dev(int curve, int op, uint64_t n, const void* d_a, const void* d_b, void* d_out, void* stream) {
    if (op < 0 || op > 2) return fail(ZK_ERR_ARG, "unknown vector op");
#define CALL(P) return vec_op_dev_impl<P>(op, n, (const uint32_t*)d_a, (const uint32_t*)d_b, (uint32_t*)d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_vec_powers_dev(int curve, uint64_t n, const uint64_t* g, void* d_out, void* stream) {
    if (n == 0) return ZK_OK;
    if (n > (1ull << 32)) return fail(ZK_ERR_ARG, "too many powers");
#define CALL(P) return powers_impl<P>(n, g, (uint32_t*)d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_vec_canon_dev(int curve, uint64_t n, void* d_x, void* stream) {
    if (n == 0) return ZK_OK;
#define CALL(P) return canon_impl<P>(n, (uint32_t*)d_x, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_vec_axpby_dev(int curve, uint64_t n, const uint64_t* a, const void* d_x, const uint64_t* b, const void* d_y, const uint64_t* c,
                     void* d_out, void* stream) {
#define CALL(P) return axpby_impl<P>(n, a, d_x, b, d_y, c, d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_vec_lincomb_dev(int curve, uint64_t n_acc, void* d_acc, int k, const uint64_t* counts, const void* const* d_x, const uint64_t* scalars,
                       int n_at, const uint64_t* at_index, const uint64_t* at_vals, void* stream) {
#define CALL(P) return lincomb_impl<P>(n_acc, d_acc, k, counts, d_x, scalars, n_at, at_index, at_vals, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_vec_gather_dev(int curve, uint64_t n, const void* d_src, uint64_t stride, uint64_t offset, void* d_dst, void* stream) {
#define CALL(P) return gather_impl<P>(n, d_src, stride, offset, d_dst, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_vec_is_zero_dev(int curve, uint64_t n, const void* d_x, int* is_zero, void* stream) {
#define CALL(P) return is_zero_impl<P>(n, d_x, is_zero, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

}  // extern "C"
