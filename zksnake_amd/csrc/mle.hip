// mle.hip -- dense multilinear polynomials over BN254 Fr / BLS12-381 Fr and the sumcheck prover's round (gfx950).
//
// Stands in for ark-poly's SparseMultilinearExtension behind the reference's MultilinearPolynomial pyclass
// (src/bn254/mle.rs:25-143, src/bls12_381/mle.rs) and for the per-round work of Sumcheck.prove / prove_arbitrary
// (python/zksnake/subprotocol/sumcheck.py:49-131, subprotocol/gkr.py:60-80).
//
// A polynomial in log_n variables is its table of 2^log_n evaluations over {0,1}^log_n, canonical Fr elements (32 B) in
// HBM.  Variable 0 is the LEAST significant bit of the table index (ark-poly's order), so fixing variable 0 to r is
//     out[j] = in[2j] + r (in[2j+1] - in[2j]).
// Like plonk.hip the kernels multiply canonical data directly: mont(x, s R) = x s, and a product of d canonical values is
// closed by a scalar carrying R^d, so no table is ever converted to Montgomery form.
//
// One workgroup of MLE_TILE threads owns a tile of MLE_TILE contiguous elements in LDS and folds up to MLE_TILE_LOG
// variables there, so fixing k variables reads the table once per MLE_TILE_LOG variables instead of k times.
#include <algorithm>
#include <vector>
#include "mle_fold.hip.h"

namespace zkmi {
using mem::DevBuf;

// MLE_TILE_LOG and MLE_TILE (elements per tile == threads per workgroup), the grid's cap and the two-level sums come from fr_sum.hip.h
constexpr int MLE_MAX_LOG = 40;
// the cap under the name tests/test_gpu_fr_large.py reads from this file to place its sizes; the launches use FR_MAX_BLOCKS
constexpr unsigned MLE_MAX_PARTIALS = 1024;
static_assert(MLE_MAX_PARTIALS == FR_MAX_BLOCKS, "the sizes of tests/test_gpu_fr_large.py sit on the shared cap");
constexpr int SC_MAX_TABLES = 8, SC_MAX_TERMS = 8, SC_MAX_DEG = 3;

// ---- fix_variables (FixArgs, fold_step and fix_work_elems: mle_fold.hip.h, shared with mlpcs.hip) -------------
// n input elements (a power of two), f >= 1 variables folded per tile of min(n, MLE_TILE) elements; (tile >> f) survivors per tile
template <class P>
__global__ __launch_bounds__(MLE_TILE) void mle_fix_kernel(uint64_t n, int f, FixArgs<P> a, const uint32_t* __restrict__ in,
                                                           uint32_t* __restrict__ out) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    const int t = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + t;
    lds_put<P>(lds, t, i < n ? load_fr<P>(in + i * P::W) : fp_zero<P>());
    __syncthreads();
    Fp<P> res = fp_zero<P>();
    for (int s = 0; s < f; ++s) {
        const int half = MLE_TILE >> (s + 1);
        if (t < half) {
            const Fp<P> lo = lds_get<P>(lds, 2 * t), hi = lds_get<P>(lds, 2 * t + 1);
            res = fold_step<P>(lo, fp_sub<P>(hi, lo), a.r_m[s]);
        }
        if (s + 1 == f) break;  // the last level goes straight to memory
        __syncthreads();
        if (t < half) lds_put<P>(lds, t, res);
        __syncthreads();
    }
    const uint64_t tile = n < MLE_TILE ? n : MLE_TILE;
    const uint64_t keep = tile >> f;
    if ((uint64_t)t < keep) store_fr<P>(out + ((uint64_t)blockIdx.x * keep + t) * P::W, fp_reduce_full<P>(res));
}

// ---- sums ------------------------------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(MLE_TILE) void mle_sum_kernel(uint64_t n, const uint32_t* __restrict__ x, uint32_t* __restrict__ partial) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    Fp<P> acc = fp_zero<P>();
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; i < n; i += stride) acc = fp_add<P>(acc, load_fr<P>(x + i * P::W));
    block_sum_store<P>(acc, lds, partial + (size_t)blockIdx.x * P::W);
}

// ---- evaluations -> monomial coefficients ----------------------------------------------------------------------
// For every bit b: x[i | 1 << b] -= x[i] (mle.rs:9-23, whose recursion does the same from the top bit down; the steps commute).
// One launch does bits s .. s + nb - 1 in LDS.  A tile is 2^lc consecutive elements (one 32 * 2^lc byte segment) for each of the
// 2^nb settings of those bits: the first pass (s = 0, lc = 0) takes MLE_TILE contiguous elements, later passes 4 x 64.
template <class P>
__global__ __launch_bounds__(MLE_TILE) void mle_coeffs_kernel(int s, int nb, int lc, const uint32_t* in, uint32_t* out) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    const int t = threadIdx.x;
    const bool active = t < (1 << (nb + lc));
    const uint64_t q = blockIdx.x;
    const int bitpart = t >> lc;
    const uint64_t lowpart = t & ((1 << lc) - 1);
    const uint64_t lowhigh = q & ((1ull << (s - lc)) - 1), high = q >> (s - lc);
    const uint64_t i = (high << (s + nb)) | ((uint64_t)bitpart << s) | (lowhigh << lc) | lowpart;
    Fp<P> v = active ? load_fr<P>(in + i * P::W) : fp_zero<P>();
    for (int b = 0; b < nb; ++b) {
        lds_put<P>(lds, t, v);
        __syncthreads();
        if (active && ((bitpart >> b) & 1)) v = fp_sub<P>(v, lds_get<P>(lds, t ^ (1 << (b + lc))));
        __syncthreads();
    }
    if (active) store_fr<P>(out + i * P::W, fp_reduce_full<P>(v));
}

// ---- bit permutation of the index ------------------------------------------------------------------------------
struct PermArgs {
    uint8_t p[64];
};
template <class P>
__global__ __launch_bounds__(MLE_TILE) void mle_permute_kernel(uint64_t n, int log_n, PermArgs a, const uint4* __restrict__ in, uint4* __restrict__ out) {
    constexpr int V = P::W / 4;  // 16-byte vectors per element
    const uint64_t g = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x;
    if (g >= n * V) return;
    const uint64_t j = g / V, part = g % V;
    uint64_t i = 0;
    for (int t = 0; t < log_n; ++t) i |= ((j >> t) & 1) << a.p[t];
    out[g] = in[i * V + part];
}

// ---- the sumcheck prover's round ---------------------------------------------------------------------------------
template <class P>
struct RoundArgs {
    const uint32_t* in[SC_MAX_TABLES];
    uint32_t* out[SC_MAX_TABLES];       // folded tables (fused form)
    Fp<P> coeff_m[SC_MAX_TERMS];        // c_t R^deg_t: closes the chain of deg_t products of canonical values
    Fp<P> r_m;                          // r R (fused form)
    int deg[SC_MAX_TERMS];
    int tbl[SC_MAX_TERMS][SC_MAX_DEG];
    int n_tables, n_terms, fused;
};

// s(X) = sum over pairs of sum_t c_t prod_j M_tj(X), M(X) = lo + X (hi - lo), at X = 0, 1, 2, 3: additions only per factor, one
// product per factor and point.  `pairs` pairs (lo, hi) = (T[2j], T[2j+1]) per table; `single`: the tables have ONE element (no
// variable left) and M(X) = lo.  Fused form: pair j of the folded tables is made here from elements 4j .. 4j+3 of the inputs,
// stored (canonical) and then used for s(.), so a sumcheck round reads each table once.  The stored values are read back by
// the thread that wrote them.
template <class P>
__global__ __launch_bounds__(MLE_TILE) void sumcheck_round_kernel(uint64_t pairs, int single, RoundArgs<P> a, uint32_t* __restrict__ partial) {
    __shared__ uint32_t lds[P::N][MLE_TILE];
    Fp<P> s0 = fp_zero<P>(), s1 = s0, s2 = s0, s3 = s0;
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    const int per = single ? 1 : 2;   // elements per pair
    for (uint64_t j = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; j < pairs; j += stride) {
        if (a.fused) {
            for (int tb = 0; tb < a.n_tables; ++tb) {
                const uint32_t* src = a.in[tb] + 2 * per * j * P::W;
                uint32_t* dst = a.out[tb] + per * j * P::W;
                for (int h = 0; h < per; ++h) {
                    const Fp<P> lo = load_fr<P>(src + 2 * h * P::W), hi = load_fr<P>(src + (2 * h + 1) * P::W);
                    store_fr<P>(dst + h * P::W, fp_reduce_full<P>(fp_add<P>(lo, fp_mul<P>(fp_sub<P>(hi, lo), a.r_m))));
                }
            }
        }
        for (int t = 0; t < a.n_terms; ++t) {
            const uint32_t* tab = (a.fused ? a.out[a.tbl[t][0]] : a.in[a.tbl[t][0]]) + per * j * P::W;
            Fp<P> e0 = fp_mul<P>(load_fr<P>(tab), a.coeff_m[t]);
            Fp<P> e1 = single ? e0 : fp_mul<P>(load_fr<P>(tab + P::W), a.coeff_m[t]);
            Fp<P> d = fp_sub<P>(e1, e0);
            Fp<P> e2 = fp_add<P>(e1, d), e3 = fp_add<P>(e2, d);
            for (int q = 1; q < a.deg[t]; ++q) {
                tab = (a.fused ? a.out[a.tbl[t][q]] : a.in[a.tbl[t][q]]) + per * j * P::W;
                const Fp<P> m0 = load_fr<P>(tab), m1 = single ? m0 : load_fr<P>(tab + P::W);
                d = fp_sub<P>(m1, m0);
                const Fp<P> m2 = fp_add<P>(m1, d), m3 = fp_add<P>(m2, d);
                e0 = fp_mul<P>(e0, m0);
                e1 = fp_mul<P>(e1, m1);
                e2 = fp_mul<P>(e2, m2);
                e3 = fp_mul<P>(e3, m3);
            }
            s0 = fp_add<P>(s0, e0);
            s1 = fp_add<P>(s1, e1);
            s2 = fp_add<P>(s2, e2);
            s3 = fp_add<P>(s3, e3);
        }
    }
    uint32_t* dst = partial + (size_t)blockIdx.x * 4 * P::W;
    block_sum_store<P>(s0, lds, dst);
    block_sum_store<P>(s1, lds, dst + P::W);
    block_sum_store<P>(s2, lds, dst + 2 * P::W);
    block_sum_store<P>(s3, lds, dst + 3 * P::W);
}

// ---- host side -----------------------------------------------------------------------------------------------------

// in (2^log_n) -> out (2^(log_n - k)), variables 0 .. k-1 fixed; `work` holds fix_work_elems(log_n, k) elements.  Enqueues only.
template <class P>
static int fix_chain(int log_n, const uint32_t* in, int k, const uint64_t* r, uint32_t* out, uint32_t* work, hipStream_t st) {
    if (k == 0) {
        ZK_HIP(hipMemcpyAsync(out, in, ((size_t)P::W * 4) << log_n, hipMemcpyDeviceToDevice, st));
        return ZK_OK;
    }
    uint32_t* tmp[2] = {work, work ? work + ((size_t)P::W << (log_n - MLE_TILE_LOG)) : nullptr};
    const uint32_t* cur = in;
    int cur_log = log_n, done = 0;
    for (int pass = 0; done < k; ++pass) {
        const int f = std::min(MLE_TILE_LOG, k - done);
        const FixArgs<P> a = fix_args<P>(r + 4 * done, f);
        uint32_t* dst = done + f == k ? out : tmp[pass & 1];
        const uint64_t n = 1ull << cur_log;
        hipLaunchKernelGGL(mle_fix_kernel<P>, dim3((unsigned)((n + MLE_TILE - 1) / MLE_TILE)), dim3(MLE_TILE), 0, st, n, f, a, cur, dst);
        ZK_HIP(hipGetLastError());
        cur = dst;
        cur_log -= f;
        done += f;
    }
    return ZK_OK;
}

template <class P>
static int mle_fix_impl(int log_n, const void* in, int k, const uint64_t* r, void* out, hipStream_t st) {
    if (log_n < 0 || log_n > MLE_MAX_LOG || k < 0 || k > log_n) return fail(ZK_ERR_ARG, "mle_fix: need 0 <= k <= log_n <= 40");
    if (!in || !out || (k && !r)) return fail(ZK_ERR_ARG, "mle_fix: null argument");
    const uint64_t eb = P::W * 4;
    if (ranges_overlap(in, eb << log_n, out, eb << (log_n - k))) return fail(ZK_ERR_ARG, "mle_fix: d_out overlaps d_in");
    const uint64_t need = fix_work_elems(log_n, k);
    DevBuf work;
    if (need) ZK_HIP_RC(work.alloc(need * eb));
    ZK_HIP_RC(fix_chain<P>(log_n, (const uint32_t*)in, k, r, (uint32_t*)out, work.as(), st));
    if (work) ZK_HIP(hipStreamSynchronize(st));  // the intermediate tables go back to the allocator only after the chain has run
    return ZK_OK;
}

template <class P>
static int mle_eval_impl(int log_n, const void* x, const uint64_t* point, uint64_t* out, void* d_work, hipStream_t st) {
    if (log_n < 0 || log_n > MLE_MAX_LOG) return fail(ZK_ERR_ARG, "mle_eval: need 0 <= log_n <= 40");
    if (!x || !out || (log_n && !point)) return fail(ZK_ERR_ARG, "mle_eval: null argument");
    const uint64_t eb = P::W * 4;
    const uint64_t need = fix_work_elems(log_n, log_n) + 1;   // the chain's intermediates, then the one-element result
    if (d_work && ranges_overlap(x, eb << log_n, d_work, need * eb)) return fail(ZK_ERR_ARG, "mle_eval: d_work overlaps d_x");
    DevBuf own;  // the work memory, when the caller passed none
    if (!d_work) ZK_HIP_RC(own.alloc(need * eb));
    uint32_t* work = d_work ? (uint32_t*)d_work : own.as();
    uint32_t* res = work + (need - 1) * P::W;
    ZK_HIP_RC(fix_chain<P>(log_n, (const uint32_t*)x, log_n, point, res, need > 1 ? work : nullptr, st));
    ZK_HIP(hipMemcpyAsync(out, res, eb, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    return ZK_OK;
}

template <class P>
static int mle_sum_impl(uint64_t n, const void* x, uint64_t* out, hipStream_t st) {
    if (!out || (n && !x)) return fail(ZK_ERR_ARG, "mle_sum: null argument");
    if (n > (1ull << MLE_MAX_LOG)) return fail(ZK_ERR_ARG, "mle_sum: at most 2^40 elements");
    for (int k = 0; k < 4; ++k) out[k] = 0;
    if (n == 0) return ZK_OK;
    FrSum<P> sum;
    ZK_HIP_RC(sum.alloc(fr_blocks(n), 1));
    hipLaunchKernelGGL(mle_sum_kernel<P>, dim3(sum.blocks), dim3(MLE_TILE), 0, st, n, (const uint32_t*)x, sum.part());
    return sum.finish(out, st);
}

template <class P>
static int mle_coeffs_impl(int log_n, const void* in, void* out, hipStream_t st) {
    if (log_n < 0 || log_n > MLE_MAX_LOG) return fail(ZK_ERR_ARG, "mle_coeffs: need 0 <= log_n <= 40");
    if (!in || !out) return fail(ZK_ERR_ARG, "mle_coeffs: null argument");
    const uint64_t bytes = ((uint64_t)P::W * 4) << log_n;
    if (in != out && ranges_overlap(in, bytes, out, bytes)) return fail(ZK_ERR_ARG, "mle_coeffs: d_out partly overlaps d_in");
    if (log_n == 0) {
        if (in != out) ZK_HIP(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, st));
        return ZK_OK;
    }
    const uint32_t* src = (const uint32_t*)in;
    for (int done = 0; done < log_n;) {
        const int lc = done ? 2 : 0;                                         // later passes: 128-byte segments
        const int nb = std::min(log_n - done, MLE_TILE_LOG - lc);
        hipLaunchKernelGGL(mle_coeffs_kernel<P>, dim3((unsigned)(1ull << (log_n - nb - lc))), dim3(MLE_TILE), 0, st, done, nb, lc, src,
                           (uint32_t*)out);
        ZK_HIP(hipGetLastError());
        src = (const uint32_t*)out;   // in place from the second pass on: every element belongs to one thread
        done += nb;
    }
    return ZK_OK;
}

template <class P>
static int mle_permute_impl(int log_n, const void* in, const uint8_t* perm, void* out, hipStream_t st) {
    if (log_n < 0 || log_n > MLE_MAX_LOG) return fail(ZK_ERR_ARG, "mle_permute: need 0 <= log_n <= 40");
    if (!in || !out || (log_n && !perm)) return fail(ZK_ERR_ARG, "mle_permute: null argument");
    PermArgs a;
    uint64_t seen = 0;
    for (int t = 0; t < log_n; ++t) {
        if (perm[t] >= log_n || ((seen >> perm[t]) & 1)) return fail(ZK_ERR_ARG, "mle_permute: not a permutation of 0 .. log_n-1");
        seen |= 1ull << perm[t];
        a.p[t] = perm[t];
    }
    const uint64_t bytes = ((uint64_t)P::W * 4) << log_n;
    if (ranges_overlap(in, bytes, out, bytes)) return fail(ZK_ERR_ARG, "mle_permute: d_out overlaps d_in");
    const uint64_t n = 1ull << log_n, nv = n * (P::W / 4);
    hipLaunchKernelGGL(mle_permute_kernel<P>, dim3((unsigned)((nv + MLE_TILE - 1) / MLE_TILE)), dim3(MLE_TILE), 0, st, n, log_n, a,
                       (const uint4*)in, (uint4*)out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int sumcheck_round_impl(int log_n, int n_tables, const void* const* tables, int n_terms, const uint64_t* coeff, const int* deg,
                               const int* term_tables, const uint64_t* r, void* const* tables_out, uint64_t* s_out, hipStream_t st) {
    if (log_n < 0 || log_n > MLE_MAX_LOG || (r && log_n < 1)) return fail(ZK_ERR_ARG, "sumcheck_round: need 0 <= log_n <= 40, and a variable to fix");
    if (n_tables < 1 || n_tables > SC_MAX_TABLES || n_terms < 1 || n_terms > SC_MAX_TERMS)
        return fail(ZK_ERR_ARG, "sumcheck_round: 1 .. 8 tables and 1 .. 8 terms");
    if (!tables || !coeff || !deg || !term_tables || !s_out || (r && !tables_out)) return fail(ZK_ERR_ARG, "sumcheck_round: null argument");
    RoundArgs<P> a;
    const uint64_t eb = P::W * 4;
    a.n_tables = n_tables;
    a.n_terms = n_terms;
    a.fused = r ? 1 : 0;
    a.r_m = r ? fr_mont<P>(r) : fp_zero<P>();
    for (int tb = 0; tb < SC_MAX_TABLES; ++tb) {
        a.in[tb] = nullptr;
        a.out[tb] = nullptr;
    }
    for (int tb = 0; tb < n_tables; ++tb) {
        if (!tables[tb] || (r && !tables_out[tb])) return fail(ZK_ERR_ARG, "sumcheck_round: null table");
        a.in[tb] = (const uint32_t*)tables[tb];
        a.out[tb] = r ? (uint32_t*)tables_out[tb] : nullptr;
    }
    uint64_t in_len[SC_MAX_TABLES], out_len[SC_MAX_TABLES];
    std::fill_n(in_len, SC_MAX_TABLES, eb << log_n);
    std::fill_n(out_len, SC_MAX_TABLES, (eb << log_n) / 2);
    for (int i = 0; r && i < n_tables; ++i) {   // a folded table against every input and every folded table before it
        if (overlaps_any(tables_out[i], out_len[i], tables, in_len, n_tables)) return fail(ZK_ERR_ARG, "sumcheck_round: a folded table overlaps an input table");
        if (overlaps_any(tables_out[i], out_len[i], tables_out, out_len, i)) return fail(ZK_ERR_ARG, "sumcheck_round: two folded tables overlap");
    }
    for (int t = 0; t < SC_MAX_TERMS; ++t) {
        a.deg[t] = 0;
        a.coeff_m[t] = fp_zero<P>();
        for (int q = 0; q < SC_MAX_DEG; ++q) a.tbl[t][q] = 0;
    }
    for (int t = 0; t < n_terms; ++t) {
        if (deg[t] < 1 || deg[t] > SC_MAX_DEG) return fail(ZK_ERR_ARG, "sumcheck_round: a term has 1 .. 3 factors");
        a.deg[t] = deg[t];
        Fp<P> c = fp_unpack<P>(reinterpret_cast<const uint32_t*>(coeff + 4 * t));
        for (int q = 0; q < deg[t]; ++q) {
            const int tb = term_tables[SC_MAX_DEG * t + q];
            if (tb < 0 || tb >= n_tables) return fail(ZK_ERR_ARG, "sumcheck_round: a term names a table that is not there");
            a.tbl[t][q] = tb;
            c = fp_mul<P>(c, fp_const<P>(P::R2));
        }
        a.coeff_m[t] = fp_reduce_full<P>(c);
    }
    const int vars = log_n - (r ? 1 : 0);           // variables of the tables s(.) is taken over
    const int single = vars == 0;
    const uint64_t pairs = single ? 1 : 1ull << (vars - 1);
    FrSum<P> sum;
    ZK_HIP_RC(sum.alloc(fr_blocks(pairs), 4));
    hipLaunchKernelGGL(sumcheck_round_kernel<P>, dim3(sum.blocks), dim3(MLE_TILE), 0, st, pairs, single, a, sum.part());
    return sum.finish(s_out, st);
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_mle_fix_dev(int curve, int log_n, const void* d_in, int k, const uint64_t* r, void* d_out, void* stream) {
#define CALL(P) return mle_fix_impl<P>(log_n, d_in, k, r, d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_mle_sum_dev(int curve, uint64_t n, const void* d_x, uint64_t* out, void* stream) {
#define CALL(P) return mle_sum_impl<P>(n, d_x, out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_mle_eval_dev(int curve, int log_n, const void* d_x, const uint64_t* point, uint64_t* out, void* d_work, void* stream) {
#define CALL(P) return mle_eval_impl<P>(log_n, d_x, point, out, d_work, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_mle_coeffs_dev(int curve, int log_n, const void* d_in, void* d_out, void* stream) {
#define CALL(P) return mle_coeffs_impl<P>(log_n, d_in, d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_mle_permute_dev(int curve, int log_n, const void* d_in, const uint8_t* perm, void* d_out, void* stream) {
#define CALL(P) return mle_permute_impl<P>(log_n, d_in, perm, d_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_sumcheck_round_dev(int curve, int log_n, int n_tables, const void* const* d_tables, int n_terms, const uint64_t* term_coeff,
                          const int* term_deg, const int* term_tables, const uint64_t* r, void* const* d_tables_out, uint64_t* s_out,
                          void* stream) {
#define CALL(P) \
    return sumcheck_round_impl<P>(log_n, n_tables, d_tables, n_terms, term_coeff, term_deg, term_tables, r, d_tables_out, s_out, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

}  // extern "C"
