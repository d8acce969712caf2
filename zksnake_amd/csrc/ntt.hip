// ntt.hip -- scalar-field radix-2 NTT / iNTT and the fused QAP quotient pipeline built on it, for BN254 Fr and
// BLS12-381 Fr on gfx950.  (The element-wise vector operations are in frvec.hip, the sparse products in spmv.hip.)
//
// Stands in for fft/ifft/coset_fft/coset_ifft of the reference (src/bn254/polynomial.rs:535-634 and the bls12_381
// twin), which call ark-poly 0.4.2's Radix2EvaluationDomain.
//
// Layout in HBM: a vector is 2^k elements x 8 u32 (32 B), canonical integers, natural order.
// The transform is linear, so it runs directly on canonical data with twiddles kept in
// Montgomery form: mont_mul(x, w*R) = x*w.  No conversion pass is needed on either side.
//
// Kernel structure: decimation-in-frequency, several butterfly stages per launch on an LDS
// tile (structure-of-arrays: limb-major, so consecutive lanes hit consecutive banks), then one
// bit-reversal pass that also applies 1/N for the inverse transform.  Twiddles w^k (k < N/2)
// are precomputed once per (field, size, direction) and streamed from HBM.
#include <algorithm>
#include <mutex>
#include <map>
#include <vector>
#include "common.hip.h"
#include "fr_mem.hip.h"
#include "ntt_lazy.hip.h"
#include "ntt_plan.h"

namespace zkmi {
using mem::DevBuf;

#ifndef NTT_THREADS_N
#define NTT_THREADS_N 512
#endif
#ifndef NTT_MIN_BLOCKS
#define NTT_MIN_BLOCKS 2
#endif
constexpr int NTT_THREADS = NTT_THREADS_N;
static_assert(NTT_THREADS % 64 == 0, "whole waves: the pass kernel's barrier-free steps count on wave w holding threads [64w, 64w + 64)");

// ---- twiddle generation -------------------------------------------------------------------
// Stage-major table, independent of the transform size: stage s of a DIF transform pairs (i, i + 2^s) and multiplies the
// difference by zeta_{s+1}^(i mod 2^s), zeta_k = primitive 2^k-th root of unity.  Row s holds zeta_{s+1}^j, j < 2^s, at
// offset 2^s - 1: consecutive butterflies read consecutive entries (the former single table w_n^k made every butterfly of
// a low stage fetch its own 64-byte sector: one L2 request each).  twiddle9_kernel below fills it.

// the lazy-range arithmetic of the butterfly passes (lz_add, lz_sub, lz_norm, lz_reduce, lz_canonical) is in ntt_lazy.hip.h

// an element as NINE raw limb words (36 bytes): the twiddle table of the passes and the scratch vectors between two passes
// keep register form, so that neither side pays the 8-word pack / unpack (78 VALU instructions per radix-4 step for the three
// twiddles alone) and values above 2^256 (< 9p between passes) have room
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
template <class P>
__device__ __forceinline__ Fp<P> load_limbs9(const uint32_t* p) {
    static_assert(P::N == 9, "scalar fields of nine 29-bit limbs");
    Fp<P> r;
    const u32x4_a4 a = *reinterpret_cast<const u32x4_a4*>(p), b = *reinterpret_cast<const u32x4_a4*>(p + 4);
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    r.v[8] = p[8];
    return r;
}
template <class P>
__device__ __forceinline__ void store_limbs9(uint32_t* p, const Fp<P>& a) {
    u32x4_a4 x, y;
    x.x = a.v[0]; x.y = a.v[1]; x.z = a.v[2]; x.w = a.v[3];
    y.x = a.v[4]; y.y = a.v[5]; y.z = a.v[6]; y.w = a.v[7];
    *reinterpret_cast<u32x4_a4*>(p) = x;
    *reinterpret_cast<u32x4_a4*>(p + 4) = y;
    p[8] = a.v[8];
}
constexpr int TW_WORDS = 9;   // words per entry of the stage-major twiddle table and of a scratch element

// stage-major twiddle table in 9-word form: canonical Montgomery representatives (< p), see the range notes above
template <class P>
__global__ void twiddle9_kernel(uint32_t* out, Fp<P> zeta, uint32_t count) {
    uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    uint32_t e[1] = {k};
    store_limbs9<P>(out + (size_t)k * TW_WORDS, fp_reduce_full<P>(fp_pow<P>(zeta, e, 1)));
}

// ---- butterfly passes -----------------------------------------------------------------------
// Decimation in frequency with the digit reversal folded into the passes.  Before a pass, `done` low bits of the
// physical index hold finished (bit-reversed) frequency digits and the upper rem = log_n - done bits the remaining
// logical index in natural order.  A pass takes the top m remaining bits D: a workgroup owns all 2^m values of D for a
// run of 2^q consecutive values of the rest of the index (so every global access is a run of 2^q elements), performs
// stages rem-1 .. rem-m on them in LDS and writes element (D, low, fin) to
//        (low << (done + m)) | (bitrev_m(D) << done) | fin,
// i.e. D's frequency digit lands just above the digits already finished.  After the last pass the vector is in natural
// order: no scattered final store, no separate reordering pass.  `in` and `out` must be different vectors unless the
// pass is the only one (a single workgroup that reads everything before it writes).
// Element formats: the first pass reads canonical 8-word elements, the last pass writes them (multiplied by `scale` when
// use_scale != 0: 1/N of the inverse transform); between two passes the elements travel as nine raw limb words with values
// below 9p (in_raw / out_raw), see the range notes above.
// What a pass can take on from the kernels around a transform (the QAP chain, qap_h_dev_impl):
//   first pass   in_v != nullptr: the element is not read but FORMED, in[p] * in_v[p] / R (the point-wise product of two coset
//                evaluation vectors; canonical inputs);
//   last pass    scale_tab != nullptr: the output is multiplied by scale_tab[index] (canonical Montgomery representatives, 8
//                words: g^i / N, or a multiple of g^-i -- the coset shift rides on the product the inverse transform pays for 1/N
//                anyway); with out2 != nullptr that goes to out2 and `out` still receives x * scale (u and u g^i from one pass);
//                with add_tab != nullptr a second vector is added (h = w / 2 + d (-g^-i / 2N), see qap_h_dev_impl).
struct NttFuse {
    const uint32_t* in_v = nullptr;       // first pass: the element is not read but FORMED, mont(in[p], in_v[p]) = in[p] in_v[p] / R
    const uint32_t* scale_tab = nullptr;
    uint32_t* out2 = nullptr;
    const uint32_t* add_tab = nullptr;    // last pass, with scale_tab and without out2: out = x * scale_tab[index] + add_tab[index]
};

template <class P>
__global__ __launch_bounds__(NTT_THREADS, NTT_MIN_BLOCKS) void ntt_pass_kernel(const uint32_t* in, uint32_t* out,
                                                               const uint32_t* __restrict__ tw, int log_n,
                                                               int rem, int m, int q, int in_raw, int final_pass, Fp<P> scale, int use_scale,
                                                               NttFuse fuse) {
    constexpr int N = P::N;  // register limbs (LDS is limb-major)
    constexpr int W = P::W;  // words per canonical element in HBM
    constexpr int T = TW_WORDS;
    extern __shared__ uint32_t lds[];  // [N][tile]
    const int done = log_n - rem;
    const int tile_log = m + q;
    const uint32_t tile = 1u << tile_log;
    const int rest_bits = log_n - m;
    const uint32_t rest0 = blockIdx.x << q;
    const uint32_t qmask = (1u << q) - 1;
    // LDS element index, skewed by one bank per 2^(tile_log - 5) elements: the first pass reads its output along the
    // bit-reversed digit (stride 2^q elements over the TOP five bits of the lane group), which would otherwise hit one bank
    const int pad_shift = tile_log >= 10 ? tile_log - 5 : 31;
    const uint32_t row = tile + 32;
    // ... and bits 3-4 XORed with bits 5-6: a radix-4 step on element bits (3, 4) -- the last step of a pass with q = 3 -- reads
    // and writes 8 consecutive elements per 8 lanes at a stride of 32 elements, four lane groups on the same 8 banks (4-way
    // conflicts: 37.5 % of the LDS-active cycles of the first and last pass of a 2^22 transform,
    // profiles/r04_ntt_lds_counters_baseline.json); with the swizzle the four groups land on four different bank octets, and
    // every other access pattern of the kernel keeps bits 5-6 constant within a 32-lane group
    const uint32_t swz = tile_log >= 7 ? 3u : 0u;
#define LIDX(e) ((((e) ^ ((((e) >> 5) & swz) << 3))) + ((e) >> pad_shift))

    for (uint32_t e = threadIdx.x; e < tile; e += NTT_THREADS) {
        const uint32_t d = e >> q, r = e & qmask;
        const uint32_t p = (d << rest_bits) | rest0 | r;
        Fp<P> x;
        if (in_raw) {
            x = load_limbs9<P>(in + (size_t)p * T);
        } else if (fuse.in_v) {
            // the point-wise product of two canonical vectors, u v / R (the R travels with the linear transform and is undone by the
            // last pass's table)
            x = fp_mul<P>(load_fr<P>(in + (size_t)p * W), load_fr<P>(fuse.in_v + (size_t)p * W));   // < 2p, normalised
        } else {
            x = load_fr<P>(in + (size_t)p * W);
        }
        const uint32_t le = LIDX(e);
#pragma unroll
        for (int l = 0; l < N; ++l) lds[l * row + le] = x.v[l];
    }
    __syncthreads();

    // Stages in pairs: a thread takes the four elements that differ in bits (b, b-1) of D, runs both stages on them
    // in registers (four butterflies, three distinct twiddles) and writes them back: half the LDS traffic and half the
    // barriers of one stage per round trip.  An odd stage count starts with a single radix-2 stage.
    int b = m - 1;
    if (m & 1) {
        const int s = rem - m + b;
        const int pos = b + q;
        const uint32_t* tws = tw + ((size_t)(1u << s) - 1) * T;
        for (uint32_t u = threadIdx.x; u < (tile >> 1); u += NTT_THREADS) {
            const uint32_t e0 = ((u >> pos) << (pos + 1)) | (u & ((1u << pos) - 1));
            const uint32_t e1 = e0 | (1u << pos);
            const uint32_t d0 = e0 >> q, r = e0 & qmask;
            const uint32_t low = (rest0 | r) >> done;                              // remaining logical bits below D
            const uint32_t j = ((d0 & ((1u << b) - 1)) << (rem - m)) | low;        // i mod 2^s
            Fp<P> x, y;
            const uint32_t l0 = LIDX(e0), l1 = LIDX(e1);
#pragma unroll
            for (int l = 0; l < N; ++l) { x.v[l] = lds[l * row + l0]; y.v[l] = lds[l * row + l1]; }
            Fp<P> w = load_limbs9<P>(tws + (size_t)j * T);
            Fp<P> sum = lz_reduce<P, 8>(lz_add<P>(x, y));              // < 18p -> < 8.7p
            Fp<P> dif = fp_mul<P>(w, lz_sub<P, 18, 29>(x, y));         // operand < 27p
#pragma unroll
            for (int l = 0; l < N; ++l) { lds[l * row + l0] = sum.v[l]; lds[l * row + l1] = dif.v[l]; }
        }
        __syncthreads();
        --b;
    }
    for (; b >= 1; b -= 2) {
        const int s = rem - m + b;          // upper stage of the pair; the lower one is s - 1
        const int pos_lo = b - 1 + q;
        const uint32_t* tw_hi = tw + ((size_t)(1u << s) - 1) * T;
        const uint32_t* tw_lo = tw + ((size_t)(1u << (s - 1)) - 1) * T;
        for (uint32_t u = threadIdx.x; u < (tile >> 2); u += NTT_THREADS) {
            const uint32_t e00 = ((u >> pos_lo) << (pos_lo + 2)) | (u & ((1u << pos_lo) - 1));
            const uint32_t e01 = e00 | (1u << pos_lo), e10 = e00 | (2u << pos_lo), e11 = e00 | (3u << pos_lo);
            const uint32_t d0 = e00 >> q, r = e00 & qmask;
            const uint32_t low = (rest0 | r) >> done;
            const uint32_t j0 = ((d0 & ((1u << b) - 1)) << (rem - m)) | low;            // stage s, bit b-1 of D clear
            const uint32_t j1 = j0 + ((1u << (b - 1)) << (rem - m));                    // stage s, bit b-1 set
            const uint32_t j2 = ((d0 & ((1u << (b - 1)) - 1)) << (rem - m)) | low;      // stage s-1 (both pairs)
            const uint32_t l00 = LIDX(e00), l01 = LIDX(e01), l10 = LIDX(e10), l11 = LIDX(e11);
            // the three twiddles first: their loads travel while the tile elements come out of LDS (left where they were used,
            // each load sat directly in front of its product with a full memory latency exposed, three times per step)
            const Fp<P> w0 = load_limbs9<P>(tw_hi + (size_t)j0 * T);
            const Fp<P> w1 = load_limbs9<P>(tw_hi + (size_t)j1 * T);
            const Fp<P> w2 = load_limbs9<P>(tw_lo + (size_t)j2 * T);
            Fp<P> x00, x01, x10, x11;
#pragma unroll
            for (int l = 0; l < N; ++l) {
                x00.v[l] = lds[l * row + l00]; x01.v[l] = lds[l * row + l01];
                x10.v[l] = lds[l * row + l10]; x11.v[l] = lds[l * row + l11];
            }
            // stage s: (x00, x10) and (x01, x11); every input normalised and < 9p (range notes above)
            Fp<P> a0 = lz_add<P>(x00, x10);
            Fp<P> a1 = fp_mul<P>(w0, lz_sub<P, 18, 29>(x00, x10));
            Fp<P> b0 = lz_add<P>(x01, x11);
            Fp<P> b1 = fp_mul<P>(w1, lz_sub<P, 18, 29>(x01, x11));
            // stage s-1: (a0, b0) and (a1, b1), one twiddle
            x00 = lz_reduce<P, 8>(lz_add<P>(a0, b0));
            x01 = fp_mul<P>(w2, lz_sub<P, 36, 30>(a0, b0));
            x10 = lz_norm<P>(lz_add<P>(a1, b1));
            x11 = fp_mul<P>(w2, fp_sub_lazy<P>(a1, b1));
#pragma unroll
            for (int l = 0; l < N; ++l) {
                lds[l * row + l00] = x00.v[l]; lds[l * row + l01] = x01.v[l];
                lds[l * row + l10] = x10.v[l]; lds[l * row + l11] = x11.v[l];
            }
        }
        // A step on element bits (pos_lo, pos_lo + 1) with pos_lo <= 6 stays inside blocks of 256 consecutive elements, and with
        // one element quad per lane (tile / 4 == NTT_THREADS) wave w holds exactly block w: when this step and the next are both of
        // that kind the next one reads only what this wave wrote, and the LDS serves one wave's accesses in order -- no workgroup
        // barrier, the waves drift apart for two steps (the last two steps of a pass with q = 3).
        // The branch relies on three things: wave64, one element quad per lane, and wave w owning elements [256w, 256w + 256).
        const bool wave_private = (tile >> 2) == NTT_THREADS && pos_lo <= 6 && b >= 3;
        if (wave_private) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        else __syncthreads();
    }

    const uint32_t fin_mask = done >= 32 ? 0xFFFFFFFFu : ((1u << done) - 1);
    for (uint32_t e = threadIdx.x; e < tile; e += NTT_THREADS) {
        // walk the OUTPUT in its run order: with done >= q the run (low q bits) stays in place and D' is next
        uint32_t d, r;
        if (done >= q) { r = e & qmask; d = e >> q; }
        else { d = e & ((1u << m) - 1); r = e >> m; }      // first pass: D' is the fastest output digit
        const uint32_t src = (__brev(d) >> (32 - m)) << q | r;  // element whose D equals bitrev(d)
        const uint32_t rest = rest0 | r;
        const uint32_t po = ((rest >> done) << (done + m)) | (d << done) | (rest & fin_mask);
        Fp<P> x;
        const uint32_t ls = LIDX(src);
#pragma unroll
        for (int l = 0; l < N; ++l) x.v[l] = lds[l * row + ls];
        if (final_pass) {
            // 1/N of the inverse transform rides on a product (9 * 1 <= R/p: the result is below 2p); a forward transform
            // comes down from < 9p by an estimated multiple of 2p
            if (fuse.scale_tab) {
                // x < 9p times a canonical constant: 9 * 1 <= R/p, the product is below 2p
                const Fp<P> t = load_fr<P>(fuse.scale_tab + (size_t)po * W);
                if (fuse.out2) {
                    store_fr<P>(fuse.out2 + (size_t)po * W, fp_reduce_full<P>(fp_mul<P>(x, t)));
                    store_fr<P>(out + (size_t)po * W, fp_reduce_full<P>(fp_mul<P>(x, scale)));
                } else if (fuse.add_tab) {
                    const Fp<P> y = fp_add<P>(fp_mul<P>(x, t), load_fr<P>(fuse.add_tab + (size_t)po * W));   // < 2p + canonical -> below 2p
                    store_fr<P>(out + (size_t)po * W, fp_reduce_full<P>(y));
                } else {
                    store_fr<P>(out + (size_t)po * W, fp_reduce_full<P>(fp_mul<P>(x, t)));
                }
            } else {
                x = use_scale ? fp_reduce_full<P>(fp_mul<P>(x, scale)) : lz_canonical<P>(x);
                store_fr<P>(out + (size_t)po * W, x);
            }
        } else {
            store_limbs9<P>(out + (size_t)po * T, x);
        }
    }
#undef LIDX
}

// x[i] *= g^(+-i) with g = w_n: row log_n - 1 of the stage-major table holds w_n^k for k < n/2; w_n^(n/2) = -1
template <class P>
__global__ void coset_scale_kernel(uint32_t* data, const uint32_t* tw, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (n == 1) return;
    uint32_t half = n >> 1;
    Fp<P> w = load_limbs9<P>(tw + ((size_t)(half - 1) + (i & (half - 1))) * TW_WORDS);
    if (i >= half) w = fp_neg<P>(w);
    Fp<P> a = load_fr<P>(data + (size_t)i * P::W);
    store_fr<P>(data + (size_t)i * P::W, fp_reduce_full<P>(fp_mul<P>(a, w)));
}

// ---- host side: what the transforms keep between calls has ONE owner and ONE mutex -----------------------------------------------
struct TwiddleSet {
    uint32_t* fwd = nullptr;
    uint32_t* inv = nullptr;
    int stages = 0;  // rows 0 .. stages-1 are built (enough for transforms up to 2^stages)
};
struct QapTabs {
    uint32_t *fwd = nullptr, *inv = nullptr;   // g^i / N and -g^-i R / (2N) as canonical Montgomery representatives, g = w_2n
};
// Scratch vectors of the transform, one set per stream (work on a stream is ordered, so reuse is safe), grow-only; and the one
// "u and v are final" event per stream (zk_qap_h_dev_begin, zk_qap_uv_dev)
struct PerStream {
    uint32_t* scratch = nullptr;
    size_t bytes = 0;
    hipEvent_t uv_ready = nullptr;
};

// Two equal tables from plain hipMalloc (not the caching allocator: they stay until shutdown).  Both go back unless the builder
// got as far as publishing them and called release(): a failing allocation, launch or synchronise leaks neither.
struct TablePair {
    uint32_t *a = nullptr, *b = nullptr;
    TablePair() = default;
    TablePair(const TablePair&) = delete;
    TablePair& operator=(const TablePair&) = delete;
    ~TablePair() { (void)hipFree(a); (void)hipFree(b); }
    int alloc(size_t bytes) {
        ZK_HIP(hipMalloc(&a, bytes));
        ZK_HIP(hipMalloc(&b, bytes));
        return ZK_OK;
    }
    void release() { a = b = nullptr; }
};

// Every member is read and written under `mutex`, and no function here takes it twice: get_qap_tabs calls get_twiddles FIRST and
// locks afterwards.
struct NttCaches {
    std::mutex mutex;
    std::map<int, TwiddleSet> twiddles;                    // per curve
    std::vector<void*> retired;                            // smaller tables replaced by a bigger one: other streams may still read them, so they stay until shutdown
    std::map<std::pair<int, int>, QapTabs> qap_tabs;       // (curve, log_n)
    std::map<hipStream_t, PerStream> streams;

    int scratch(hipStream_t stream, size_t bytes, uint32_t** out) {
        std::lock_guard<std::mutex> lock(mutex);
        PerStream& ps = streams[stream];
        if (ps.bytes < bytes) {
            if (ps.scratch) {
                ZK_HIP(hipStreamSynchronize(stream));   // queued passes may still read the vectors that go
                (void)hipFree(ps.scratch);
                ps.scratch = nullptr;
                ps.bytes = 0;
            }
            ZK_HIP(hipMalloc(&ps.scratch, bytes));
            ps.bytes = bytes;
        }
        *out = ps.scratch;
        return ZK_OK;
    }

    int uv_event(hipStream_t stream, hipEvent_t* out) {
        std::lock_guard<std::mutex> lock(mutex);
        PerStream& ps = streams[stream];
        if (!ps.uv_ready) ZK_HIP(hipEventCreateWithFlags(&ps.uv_ready, hipEventDisableTiming));
        *out = ps.uv_ready;
        return ZK_OK;
    }

    // zk_shutdown
    void free_all() {
        std::lock_guard<std::mutex> lock(mutex);
        for (auto& kv : twiddles) { (void)hipFree(kv.second.fwd); (void)hipFree(kv.second.inv); }
        for (void* p : retired) (void)hipFree(p);
        for (auto& kv : qap_tabs) { (void)hipFree(kv.second.fwd); (void)hipFree(kv.second.inv); }
        for (auto& kv : streams) {
            (void)hipFree(kv.second.scratch);
            if (kv.second.uv_ready) (void)hipEventDestroy(kv.second.uv_ready);
        }
        twiddles.clear();
        retired.clear();
        qap_tabs.clear();
        streams.clear();
    }

    // zk_stream_destroy: what is kept for this stream goes with it (it used to stay until zk_shutdown, and the next stream that was
    // handed the same handle value inherited it).  The caller has synchronised the stream: nothing queued on it reads the scratch.
    void release_stream(hipStream_t stream) {
        PerStream ps;
        {
            std::lock_guard<std::mutex> lock(mutex);
            auto it = streams.find(stream);
            if (it == streams.end()) return;
            ps = it->second;
            streams.erase(it);
        }
        (void)hipFree(ps.scratch);
        if (ps.uv_ready) (void)hipEventDestroy(ps.uv_ready);
    }
};
static NttCaches g_ntt;

template <class P>
static Fp<P> host_root(int log_order, bool inverse) {
    // primitive 2^log_order-th root of unity (or its inverse)
    Fp<P> w = fp_const<P>(inverse ? P::ROOT_INV : P::ROOT);
    for (int k = 0; k < P::TWO_ADICITY - log_order; ++k) w = fp_sqr<P>(w);
    return w;
}

template <class P>
static int get_twiddles(int curve, int log_n, TwiddleSet* out, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g_ntt.mutex);
    TwiddleSet& cur = g_ntt.twiddles[curve];
    if (cur.stages >= log_n) { *out = cur; return ZK_OK; }
    TwiddleSet ts;
    ts.stages = log_n < 16 ? 16 : log_n;  // small transforms share one 2 MiB table
    if (ts.stages > P::TWO_ADICITY) ts.stages = P::TWO_ADICITY;
    TablePair tabs;
    ZK_HIP_RC(tabs.alloc((((size_t)1 << ts.stages) - 1) * TW_WORDS * 4));
    for (int s = 0; s < ts.stages; ++s) {
        const uint32_t count = 1u << s;
        const size_t off = ((size_t)count - 1) * TW_WORDS;
        hipLaunchKernelGGL(twiddle9_kernel<P>, dim3((count + 255) / 256), dim3(256), 0, stream, tabs.a + off, host_root<P>(s + 1, false), count);
        hipLaunchKernelGGL(twiddle9_kernel<P>, dim3((count + 255) / 256), dim3(256), 0, stream, tabs.b + off, host_root<P>(s + 1, true), count);
    }
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(stream));
    if (cur.fwd) { g_ntt.retired.push_back(cur.fwd); g_ntt.retired.push_back(cur.inv); }
    ts.fwd = tabs.a;
    ts.inv = tabs.b;
    tabs.release();
    cur = ts;
    *out = ts;
    return ZK_OK;
}

// the pass kernel asks for more dynamic LDS than a kernel gets by default: once per field, under the owner's lock
template <class P>
static int allow_pass_lds() {
    static bool set = false;   // one per field; a property of the loaded kernel, so it outlives free_all()
    std::lock_guard<std::mutex> lock(g_ntt.mutex);
    if (set) return ZK_OK;
    ZK_HIP(hipFuncSetAttribute((const void*)ntt_pass_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(P::N * ((1u << NTT_TILE_LOG) + 32) * 4)));
    set = true;
    return ZK_OK;
}

// what qap_h_dev_impl folds into a transform: NttFuse for the kernel, plus the vectors the first pass reads from (src, instead
// of d) and the last pass writes to (dst, instead of d)
template <class P>
struct NttPlanFuse {
    const uint32_t* src = nullptr;
    uint32_t* dst = nullptr;
    NttFuse k;
    bool own_scale = false;   // an inverse transform multiplies by `scale` (canonical Montgomery form) instead of 1/N
    Fp<P> scale;
};

// One launch per pass of ntt_plan (ntt_plan.h).  Data flow: d -> scratch A -> scratch B -> ... -> d (a single pass runs in place:
// one workgroup holds the whole vector).
template <class P>
static int ntt_dev_impl(int curve, int inverse, int log_n, uint32_t* d, hipStream_t stream, const NttPlanFuse<P>* fuse = nullptr) {
    if (log_n < 0 || log_n > P::TWO_ADICITY || log_n > 30) return fail(ZK_ERR_DOMAIN, "Domain size is too large");
    if (log_n == 0) return ZK_OK;
    int rc = allow_pass_lds<P>();
    if (rc) return rc;
    TwiddleSet ts;
    if ((rc = get_twiddles<P>(curve, log_n, &ts, stream))) return rc;
    const uint32_t* tw = inverse ? ts.inv : ts.fwd;
    const size_t bytes = ((size_t)1 << log_n) * TW_WORDS * 4;   // a scratch vector: nine raw limb words per element
    Fp<P> scale = fp_one<P>();
    if (inverse) {
        uint32_t nn[P::W] = {0};
        nn[0] = 1u << log_n;
        scale = fp_reduce_full<P>(fp_inv<P>(fp_from_canonical<P>(nn)));   // canonical: the last pass multiplies values < 9p by it
        if (fuse && fuse->own_scale) scale = fuse->scale;
    }
    NttPass plan[8];
    const int passes = ntt_plan(log_n, plan);
    uint32_t* scratch = nullptr;
    if (passes > 1 && (rc = g_ntt.scratch(stream, bytes * (passes > 2 ? 2 : 1), &scratch))) return rc;
    uint32_t* bufs[2] = {scratch, scratch ? scratch + (bytes / 4) : nullptr};
    const uint32_t* src = fuse && fuse->src ? fuse->src : d;
    uint32_t* final_dst = fuse && fuse->dst ? fuse->dst : d;
    int rem = log_n, which = 0;
    for (int i = 0; i < passes; ++i) {
        const int m = plan[i].m, q = plan[i].q;
        const bool last = i == passes - 1;
        uint32_t* dst = last ? final_dst : bufs[which];
        const uint32_t tile = 1u << (m + q);
        const size_t lds_bytes = (size_t)P::N * (tile + 32) * 4;
        NttFuse kf;
        if (fuse && i == 0) kf.in_v = fuse->k.in_v;
        if (fuse && last) { kf.scale_tab = fuse->k.scale_tab; kf.out2 = fuse->k.out2; kf.add_tab = fuse->k.add_tab; }
        hipLaunchKernelGGL(ntt_pass_kernel<P>, dim3(1u << (log_n - m - q)), dim3(NTT_THREADS), lds_bytes, stream, src, dst, tw, log_n, rem, m, q,
                           i > 0 ? 1 : 0, last ? 1 : 0, scale, (last && inverse) ? 1 : 0, kf);
        src = dst;
        which ^= 1;
        rem -= m;
    }
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int coset_scale_impl(int curve, int inverse, int log_n, uint32_t* d, hipStream_t stream) {
    if (log_n == 0) return ZK_OK;
    TwiddleSet ts;
    int rc = get_twiddles<P>(curve, log_n, &ts, stream);
    if (rc) return rc;
    uint32_t n = 1u << log_n;
    hipLaunchKernelGGL(coset_scale_kernel<P>, dim3((n + 255) / 256), dim3(256), 0, stream, d, inverse ? ts.inv : ts.fwd, n);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int ntt_host_impl(int curve, int inverse, int coset, uint64_t n_in, const uint64_t* in, uint64_t size, uint64_t* out) {
    uint64_t n = next_pow2_u64(size == 0 ? 1 : size);
    int log_n = log2_u64(n);
    if (log_n > P::TWO_ADICITY || log_n > 30) return fail(ZK_ERR_DOMAIN, "Domain size is too large");
    const size_t eb = P::W * 4;
    // An input longer than the domain is TRUNCATED to the domain size: the reference hands the raw slice to
    // EvaluationDomain::fft / ifft (polynomial.rs:541-542,567-568), whose radix-2 fft_in_place / ifft_in_place start with
    // `coeffs.resize(self.size(), zero)` [ark-poly 0.4.2, not vendored: parity unpinned, see DESIGN.md section 2]; only
    // DensePolynomial::evaluate_over_domain folds modulo X^n - 1, and the reference does not call it on this path.
    if (n_in > n) n_in = n;
    const uint64_t alloc = n;
    DevBuf buf;
    ZK_HIP_RC(buf.alloc(alloc * eb));
    uint32_t* const d = buf.as();
    ZK_HIP(hipMemset(d, 0, alloc * eb));
    if (n_in) ZK_HIP(hipMemcpy(d, in, n_in * eb, hipMemcpyHostToDevice));
    ZK_HIP_RC(zk_vec_canon_dev(curve, alloc, d, nullptr));   // inputs of the host API may be >= r (frvec.hip)
    if (coset && !inverse) ZK_HIP_RC(coset_scale_impl<P>(curve, 0, log_n, d, 0));
    ZK_HIP_RC(ntt_dev_impl<P>(curve, inverse, log_n, d, 0));
    if (coset && inverse) ZK_HIP_RC(coset_scale_impl<P>(curve, 1, log_n, d, 0));
    ZK_HIP(hipMemcpy(out, d, n * eb, hipMemcpyDeviceToHost));
    return ZK_OK;
}

// ---- QAP quotient on a coset ------------------------------------------------------------------------------------
// h = (u v - w) / (X^n - 1).  The reference multiplies u and v over the doubled domain and divides the 2n coefficients
// (qap.py:51-67 -> mul_over_fft, divide_by_vanishing_poly).  Write u v = P_lo + X^n P_hi (both parts of degree < n): modulo X^n - 1
// that is w = P_lo + P_hi, and the quotient is h = P_hi.  On the coset g H with g = the primitive 2n-th root of unity (g^n = -1)
// the n values u(g w^i) v(g w^i) interpolate u v mod (X^n + 1) = P_lo - P_hi =: d, so
//                                  h = (w - d) / 2
// -- SIX size-n transforms (round 4; seven until then, on the coset 5 H with a point-wise division by the constant g^n - 1): the
// three inverse transforms of a, b, c, two forward transforms of the g^i-shifted u and v, and one inverse transform of their
// point-wise product.  And nothing between them (NttFuse): the shift g^i rides on the 1/N product of the inverse transforms'
// last pass (u and v leave it twice: plain, for their MSMs, and shifted), w is read from c and written as w / 2, the product
// u v is formed by the FIRST pass of the last inverse transform as it loads, and its LAST pass multiplies by -g^-i / (2N) and adds
// w / 2: it writes h.  The quotient is exact iff a_i b_i = c_i on the domain itself, which is checked directly on the evaluation
// vectors (the reference's "remainder must be zero", qap.py:68-69).
// row log_n of the stage-major twiddle tables holds w_2n^(+-i), i < n, as nine-word Montgomery representatives
template <class P>
__global__ void qap_tabs_kernel(uint32_t* __restrict__ fwd, uint32_t* __restrict__ inv, uint64_t n, const uint32_t* __restrict__ row_f,
                                const uint32_t* __restrict__ row_i, Fp<P> inv_n, Fp<P> c_inv) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_fr<P>(fwd + i * P::W, fp_reduce_full<P>(fp_mul<P>(load_limbs9<P>(row_f + i * TW_WORDS), inv_n)));   // (g^i R)(R / N) / R
    store_fr<P>(inv + i * P::W, fp_reduce_full<P>(fp_mul<P>(load_limbs9<P>(row_i + i * TW_WORDS), c_inv)));   // (g^-i R)(-R^2 / 2N) / R
}

template <class P>
static int get_qap_tabs(int curve, int log_n, QapTabs* out, hipStream_t stream) {
    TwiddleSet ts;
    int rc = get_twiddles<P>(curve, log_n + 1, &ts, stream);   // takes the owner's mutex itself: first this, then the lock
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(g_ntt.mutex);
    auto it = g_ntt.qap_tabs.find({curve, log_n});
    if (it != g_ntt.qap_tabs.end()) { *out = it->second; return ZK_OK; }
    const uint64_t n = 1ull << log_n;
    TablePair tabs;
    ZK_HIP_RC(tabs.alloc(n * P::W * 4));
    uint32_t nn[P::W] = {0};
    nn[0] = (uint32_t)n;
    const Fp<P> inv_n = fp_inv<P>(fp_from_canonical<P>(nn));                            // R / N
    const Fp<P> half = fp_inv<P>(fp_add<P>(fp_one<P>(), fp_one<P>()));                  // R / 2
    const Fp<P> c_inv = fp_mul<P>(fp_neg<P>(fp_mul<P>(inv_n, half)), fp_const<P>(P::R2));   // -(R / 2N) R^2 / R = -R^2 / (2N)
    const size_t row = (((size_t)1 << log_n) - 1) * TW_WORDS;
    hipLaunchKernelGGL(qap_tabs_kernel<P>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, tabs.a, tabs.b, n, ts.fwd + row, ts.inv + row, inv_n, c_inv);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipStreamSynchronize(stream));
    QapTabs t;
    t.fwd = tabs.a;
    t.inv = tabs.b;
    tabs.release();
    g_ntt.qap_tabs[{curve, log_n}] = t;
    *out = t;
    return ZK_OK;
}

// flag |= (a[i] * b[i] != c[i]) on the domain: the witness satisfies the constraints iff this never fires
template <class P>
__global__ void qap_eval_check_kernel(uint64_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                      const uint32_t* __restrict__ c, int* nonzero) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // mont(a, b) = a b / R against mont(c, 1) = c / R
    Fp<P> one = fp_zero<P>();
    one.v[0] = 1;
    Fp<P> r = fp_sub<P>(fp_mul<P>(load_fr<P>(a + i * P::W), load_fr<P>(b + i * P::W)), fp_mul<P>(load_fr<P>(c + i * P::W), one));
    if (!fp_is_zero<P>(r)) atomicOr(nonzero, 1);
}

// divisible == nullptr: enqueue only (zk_qap_h_dev_begin); uv_ready (optional) is recorded once u and v are final
template <class P>
static int qap_h_dev_impl(int curve, int log_n, uint32_t* a_u, uint32_t* b_v, const uint32_t* c, uint32_t* h,
                          uint32_t* work, int* divisible, hipStream_t stream, hipEvent_t uv_ready = nullptr) {
    if (log_n < 0) return fail(ZK_ERR_DOMAIN, "Domain size is negative");
    // the coset generator is the primitive 2n-th root of unity: one level of two-adicity above the domain
    if (log_n + 1 > P::TWO_ADICITY || log_n > 30) return fail(ZK_ERR_DOMAIN, "Domain size is too large");
    const uint64_t n = 1ull << log_n;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    uint32_t* W0 = work;                     // w / 2 (coefficients)
    uint32_t* U1 = work + n * P::W;          // u g^i, then u on the coset
    uint32_t* V1 = work + 2 * n * P::W;      // v g^i, then v on the coset
    int* dflag = reinterpret_cast<int*>(work + 3 * n * P::W);
    auto finish = [&]() -> int {
        ZK_HIP(hipGetLastError());
        if (!divisible) return ZK_OK;
        int flag = 0;
        ZK_HIP(hipMemcpyAsync(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost, stream));
        ZK_HIP(hipStreamSynchronize(stream));
        *divisible = flag ? 0 : 1;
        return ZK_OK;
    };
    QapTabs qt;
    int rc;
    if (log_n > 0 && (rc = get_qap_tabs<P>(curve, log_n, &qt, stream))) return rc;
    ZK_HIP(hipMemsetAsync(dflag, 0, sizeof(int), stream));
    hipLaunchKernelGGL(qap_eval_check_kernel<P>, dim3(blocks), dim3(256), 0, stream, n, a_u, b_v, c, dflag);
    if (log_n == 0) {
        // one point: u = a and v = b (a size-1 transform is the identity) and u v - w is a constant, so h = 0; the check
        // above sets the flag when a b != c
        ZK_HIP(hipMemsetAsync(h, 0, P::W * sizeof(uint32_t), stream));
        if (uv_ready) ZK_HIP(hipEventRecord(uv_ready, stream));
        return finish();
    }
    NttPlanFuse<P> f;
    f.k.scale_tab = qt.fwd;
    f.k.out2 = U1;
    if ((rc = ntt_dev_impl<P>(curve, 1, log_n, a_u, stream, &f))) return rc;  // u, and u g^i into U1
    f.k.out2 = V1;
    if ((rc = ntt_dev_impl<P>(curve, 1, log_n, b_v, stream, &f))) return rc;  // v, and v g^i into V1
    if (uv_ready) ZK_HIP(hipEventRecord(uv_ready, stream));
    NttPlanFuse<P> fw;   // w / 2 straight from c: the inverse transform's scale is 1 / (2N)
    fw.src = c;
    fw.own_scale = true;
    {
        uint32_t nn[P::W] = {0};
        nn[0] = (uint32_t)n;
        const Fp<P> two_n = fp_add<P>(fp_from_canonical<P>(nn), fp_from_canonical<P>(nn));
        fw.scale = fp_reduce_full<P>(fp_inv<P>(two_n));
    }
    if ((rc = ntt_dev_impl<P>(curve, 1, log_n, W0, stream, &fw))) return rc;
    if ((rc = ntt_dev_impl<P>(curve, 0, log_n, U1, stream))) return rc;       // u on g H
    if ((rc = ntt_dev_impl<P>(curve, 0, log_n, V1, stream))) return rc;       // v on g H
    NttPlanFuse<P> fq;   // h = w / 2 + iNTT_unscaled(u v / R) * (-g^-i R / 2N)
    fq.k.in_v = V1;
    fq.k.scale_tab = qt.inv;
    fq.k.add_tab = W0;
    fq.dst = h;
    if ((rc = ntt_dev_impl<P>(curve, 1, log_n, U1, stream, &fq))) return rc;
    return finish();
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_ntt(int curve, int inverse, int coset, uint64_t n_in, const uint64_t* in, uint64_t size, uint64_t* out) {
#define CALL(P) return ntt_host_impl<P>(curve, inverse, coset, n_in, in, size, out)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_ntt_dev(int curve, int inverse, int log_n, void* d_data, void* stream) {
#define CALL(P) return ntt_dev_impl<P>(curve, inverse, log_n, (uint32_t*)d_data, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_qap_h_dev(int curve, int log_n, void* d_a_u, void* d_b_v, const void* d_c, void* d_h, void* d_work, int* divisible, void* stream) {
#define CALL(P) return qap_h_dev_impl<P>(curve, log_n, (uint32_t*)d_a_u, (uint32_t*)d_b_v, (const uint32_t*)d_c, (uint32_t*)d_h, (uint32_t*)d_work, divisible, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_qap_h_dev_begin(int curve, int log_n, void* d_a_u, void* d_b_v, const void* d_c, void* d_h, void* d_work, void* stream, void** uv_ready) {
    hipEvent_t ev = nullptr;
    if (uv_ready) {
        int rc = g_ntt.uv_event((hipStream_t)stream, &ev);
        if (rc) return rc;
        *uv_ready = (void*)ev;
    }
#define CALL(P) return qap_h_dev_impl<P>(curve, log_n, (uint32_t*)d_a_u, (uint32_t*)d_b_v, (const uint32_t*)d_c, (uint32_t*)d_h, (uint32_t*)d_work, nullptr, (hipStream_t)stream, ev)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_qap_uv_dev(int curve, int log_n, void* d_a_u, void* d_b_v, void* stream, void** uv_ready) {
    hipEvent_t ev = nullptr;
    if (uv_ready) {
        int rc = g_ntt.uv_event((hipStream_t)stream, &ev);
        if (rc) return rc;
        *uv_ready = (void*)ev;
    }
    int rc = ZK_OK;
    if (d_a_u && (rc = zk_ntt_dev(curve, 1, log_n, d_a_u, stream))) return rc;
    if (d_b_v && (rc = zk_ntt_dev(curve, 1, log_n, d_b_v, stream))) return rc;
    if (ev) ZK_HIP(hipEventRecord(ev, (hipStream_t)stream));
    return ZK_OK;
}

int zk_qap_h_dev_end(int curve, int log_n, const void* d_work, int* divisible, void* stream) {
    if (curve != ZK_CURVE_BN254 && curve != ZK_CURVE_BLS12_381) return fail(ZK_ERR_ARG, "unknown curve");
    if (log_n < 0 || log_n > 32) return fail(ZK_ERR_DOMAIN, "Domain size is too large");
    const int* dflag = reinterpret_cast<const int*>(reinterpret_cast<const uint32_t*>(d_work) + ((size_t)3 << log_n) * 8);  // both scalar fields: 8 words
    int flag = 0;
    ZK_HIP(hipMemcpyAsync(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    ZK_HIP(hipStreamSynchronize((hipStream_t)stream));
    *divisible = flag ? 0 : 1;
    return ZK_OK;
}

// the two hooks of host.hip (zk_shutdown, zk_stream_destroy)
void zk_ntt_free_cache(void) { g_ntt.free_all(); }
void zk_ntt_stream_released(void* stream) { g_ntt.release_stream((hipStream_t)stream); }

}  // extern "C"
