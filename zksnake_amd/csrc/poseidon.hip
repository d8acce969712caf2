// poseidon.hip -- the Poseidon permutation over BN254 Fr / BLS12-381 Fr, the fixed-length hash, a sponge over rows and Merkle
// trees of 32-byte nodes (gfx950).  DESIGN.md section 4.15 fixes the definitions; the tree apart from its hash (layout, build
// schedule, opening paths) is merkle_tree.hip.h.
//
// The reference has no algebraic hash: its only Poseidon is the circom fixture its Groth16 test proves (tests/stub/test_poseidon.*),
// and that fixture is what pins width 4 here.  Poseidon (Grassi et al., USENIX Security 2021) with S-box x^5, R_F = 8 and circomlib's
// partial-round table; round constants and the Cauchy matrix come from the paper's Grain LFSR, generated on the host at first use
// and kept, already in Montgomery form and as 29-bit limbs, in one device table per (curve, t).
//
// A permutation is ONE LANE's work: the t state elements stay in registers as 29-bit limbs in Montgomery form, the table is read
// through a const __restrict__ kernel argument with an index every lane of a wave shares (scalar loads), and a round holds no
// conversion.  The round loop is rolled over the rounds and unrolled over t; a row of the matrix product is t products summed in the
// column accumulators of ONE Montgomery reduction (t N^2 + N^2 + N multiply-adds in place of t (2 N^2 + N)).  Workgroups of MLE_TILE
// threads on the capped strided grid of fr_sum.hip.h; plain C++, no atomics, no LDS.
#include <mutex>
#include <vector>
#include "merkle_tree.hip.h"

namespace zkmi {

constexpr uint64_t POSEIDON_MAX_ROW = ZK_POSEIDON_MAX_ROW;
constexpr uint64_t NODE = 32;       // bytes per tree node: one canonical Fr element
constexpr int POSEIDON_RF = 8;
constexpr int poseidon_rp(int t) { return t == 3 ? 57 : t == 4 ? 56 : 60; }   // circomlib's table, used on both curves
constexpr int poseidon_consts(int t) { return (POSEIDON_RF + poseidon_rp(t)) * t + t * t; }   // round constants, then the matrix

// ---- the permutation (host and device: the host runs it in tests/native/poseidon_args_check.cpp) -------------------------------

// sum_j s[j] * m[j] / R in one Montgomery reduction, m: T elements of N limbs below p.  Column room: (T + 1) N products below 2^58,
// 54 * 2^58 < 2^64 for T = 5, N = 9.  Value: T * 2p * p / R + p < 2p as long as 2 T < R / p (>= 70 for both fields).
template <class P, int T>
ZK_HD Fp<P> poseidon_dot(const Fp<P>* s, const uint32_t* __restrict__ m) {
    constexpr int N = P::N;
    static_assert((T + 1) * N < 64 && 2 * T < 70, "the column accumulators and the 2p bound hold up to t = 5 on 9 limbs");
    uint64_t acc = 0;
    uint32_t q[N];
    Fp<P> r;
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int i = 0; i <= k; ++i) acc += (uint64_t)s[j].v[i] * m[j * N + k - i];
#pragma unroll
        for (int i = 0; i < k; ++i) acc += (uint64_t)q[i] * P::M[k - i];
        q[k] = ((uint32_t)acc * P::INV) & LIMB_MASK;
        acc += (uint64_t)q[k] * P::M[0];
        acc >>= LIMB_BITS;
    }
#pragma unroll
    for (int k = N; k < 2 * N - 1; ++k) {
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int i = k - N + 1; i < N; ++i) acc += (uint64_t)s[j].v[i] * m[j * N + k - i];
#pragma unroll
        for (int i = k - N + 1; i < N; ++i) acc += (uint64_t)q[i] * P::M[k - i];
        r.v[k - N] = (uint32_t)acc & LIMB_MASK;
        acc >>= LIMB_BITS;
    }
    r.v[N - 1] = (uint32_t)acc;
    return r;
}

template <class P>
ZK_HD Fp<P> poseidon_sbox(const Fp<P>& x) {
    return fp_mul<P>(fp_sqr<P>(fp_sqr<P>(x)), x);
}

// the loops over t around an S-box or a matrix row are written as recursions over the index: the optimizer leaves such a loop
// rolled at t = 4 and 5 ("loop not unrolled") and the state goes to scratch memory
template <class P, int T, int I = 1>
ZK_HD void poseidon_sbox_rest(Fp<P> (&s)[T]) {
    if constexpr (I < T) {
        s[I] = poseidon_sbox<P>(s[I]);
        poseidon_sbox_rest<P, T, I + 1>(s);
    }
}
template <class P, int T, int I = 0>
ZK_HD void poseidon_mix(const Fp<P> (&s)[T], Fp<P> (&o)[T], const uint32_t* __restrict__ mds) {
    if constexpr (I < T) {
        o[I] = poseidon_dot<P, T>(s, mds + I * T * P::N);
        poseidon_mix<P, T, I + 1>(s, o, mds);
    }
}

// s <- perm_T(s), s in Montgomery form below 2p before and after.  tab: (R_F + R_P) T round constants, then the T x T matrix
// row-major, N limbs each, Montgomery form below p.  A round: add constants, S-box (every element in the first and last R_F / 2
// rounds, element 0 in between), matrix.
template <class P, int T>
ZK_HD void poseidon_perm(Fp<P> (&s)[T], const uint32_t* __restrict__ tab) {
    constexpr int N = P::N, RP = poseidon_rp(T), ROUNDS = POSEIDON_RF + RP;
    const uint32_t* __restrict__ mds = tab + ROUNDS * T * N;
#pragma unroll 1
    for (int r = 0; r < ROUNDS; ++r) {
        const uint32_t* __restrict__ c = tab + r * T * N;
#pragma unroll
        for (int i = 0; i < T; ++i) {
            Fp<P> ci;
#pragma unroll
            for (int l = 0; l < N; ++l) ci.v[l] = c[i * N + l];
            s[i] = fp_add<P>(s[i], ci);
        }
        s[0] = poseidon_sbox<P>(s[0]);
        if (r < POSEIDON_RF / 2 || r >= POSEIDON_RF / 2 + RP) poseidon_sbox_rest<P, T>(s);
        Fp<P> o[T];
        poseidon_mix<P, T>(s, o, mds);
#pragma unroll
        for (int i = 0; i < T; ++i) s[i] = o[i];
    }
}

// canonical element in memory <-> Montgomery form in registers
template <class P>
ZK_D Fp<P> poseidon_in(const uint32_t* p) {
    return fp_mul<P>(load_fr<P>(p), fp_const<P>(P::R2));
}
template <class P>
ZK_D void poseidon_out(uint32_t* p, const Fp<P>& a) {
    store_fr<P>(p, fp_reduce_full<P>(fp_mul<P>(a, fp_raw_one<P>())));
}

// ---- kernels ------------------------------------------------------------------------------------------------------------

// state i = perm_T(state i): T elements at in + i T, to out + i T.  out == in is allowed: a lane reads its state before it writes it.
template <class P, int T>
__global__ __launch_bounds__(MLE_TILE) void poseidon_perm_kernel(uint64_t n, const uint32_t* __restrict__ tab, const uint32_t* in, uint32_t* out) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; i < n; i += stride) {
        Fp<P> s[T];
#pragma unroll
        for (int j = 0; j < T; ++j) s[j] = poseidon_in<P>(in + (i * T + j) * P::W);
        poseidon_perm<P, T>(s, tab);
#pragma unroll
        for (int j = 0; j < T; ++j) poseidon_out<P>(out + (i * T + j) * P::W, s[j]);
    }
}

// out[i] = perm_T([0, row i])[0], a row is T - 1 elements
template <class P, int T>
__global__ __launch_bounds__(MLE_TILE) void poseidon_hash_kernel(uint64_t n, const uint32_t* __restrict__ tab, const uint32_t* __restrict__ rows,
                                                                 uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; i < n; i += stride) {
        Fp<P> s[T];
        s[0] = fp_zero<P>();
#pragma unroll
        for (int j = 1; j < T; ++j) s[j] = poseidon_in<P>(rows + (i * (T - 1) + j - 1) * P::W);
        poseidon_perm<P, T>(s, tab);
        poseidon_out<P>(out + i * P::W, s[0]);
    }
}

// digest i = sponge(row i), a row is `len` elements: width 3, rate 2, the state starts as [len, 0, 0], every block adds its one or
// two elements to state[1], state[2] and runs perm_3; the digest is state[1].  len_m: len in Montgomery form.
template <class P>
__global__ __launch_bounds__(MLE_TILE) void poseidon_sponge_kernel(uint64_t n, const uint32_t* __restrict__ tab, const uint32_t* __restrict__ rows,
                                                                   uint64_t len, Fp<P> len_m, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; i < n; i += stride) {
        const uint32_t* row = rows + i * len * P::W;
        Fp<P> s[3] = {len_m, fp_zero<P>(), fp_zero<P>()};
        for (uint64_t e = 0; e < len; e += 2) {
            s[1] = fp_add<P>(s[1], poseidon_in<P>(row + e * P::W));
            if (e + 1 < len) s[2] = fp_add<P>(s[2], poseidon_in<P>(row + (e + 1) * P::W));
            poseidon_perm<P, 3>(s, tab);
        }
        poseidon_out<P>(out + i * P::W, s[1]);
    }
}

// parent i of a level of n_child nodes: hash(child[2i], child[2i+1]), child[2i] twice where 2i+1 is past the level
template <class P>
__global__ __launch_bounds__(MLE_TILE) void poseidon_level_kernel(uint64_t n_child, const uint32_t* __restrict__ tab, const uint32_t* __restrict__ child,
                                                                  uint32_t* __restrict__ parent) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE, n_parent = (n_child + 1) / 2;
    for (uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; i < n_parent; i += stride) {
        const uint64_t l = 2 * i, r = l + 1 < n_child ? l + 1 : l;
        Fp<P> s[3] = {fp_zero<P>(), poseidon_in<P>(child + l * P::W), poseidon_in<P>(child + r * P::W)};
        poseidon_perm<P, 3>(s, tab);
        poseidon_out<P>(parent + i * P::W, s[0]);
    }
}

// ---- parameters: the paper's Grain LFSR on the host ---------------------------------------------------------------------------

// 80 bits, b[0] the oldest; update: new = b62 ^ b51 ^ b38 ^ b23 ^ b13 ^ b0, shift, append
struct PoseidonGrain {
    uint8_t b[80];
    int head = 0;   // position of b[0] in the ring

    // field = 1 (2 bits), S-box = 0 (4), n (12), t (12), R_F (10), R_P (10), thirty ones; each most significant bit first
    PoseidonGrain(int n, int t, int rf, int rp) {
        const int value[7] = {1, 0, n, t, rf, rp, (1 << 30) - 1}, width[7] = {2, 4, 12, 12, 10, 10, 30};
        int at = 0;
        for (int f = 0; f < 7; ++f)
            for (int i = width[f] - 1; i >= 0; --i) b[at++] = (uint8_t)((value[f] >> i) & 1);
        for (int i = 0; i < 160; ++i) (void)step();
    }
    int step() {
        auto bit = [&](int i) { return b[(head + i) % 80]; };
        const uint8_t fresh = bit(62) ^ bit(51) ^ bit(38) ^ bit(23) ^ bit(13) ^ bit(0);
        b[head] = fresh;
        head = (head + 1) % 80;
        return fresh;
    }
    // bits are read in pairs: the second one counts when the first is 1
    int emitted() {
        for (;;) {
            const int first = step(), second = step();
            if (first) return second;
        }
    }
    // n emitted bits, the first one the most significant, as W words
    template <class P>
    void draw(uint32_t* w) {
        for (int i = 0; i < P::W; ++i) w[i] = 0;
        for (int i = P::BITS - 1; i >= 0; --i) w[i >> 5] |= (uint32_t)emitted() << (i & 31);
    }
};

// canonical words of the (R_F + R_P) t round constants in round order, then of the t x t matrix M[i][j] = 1 / (x_i + y_j) row-major.
// Round constants are redrawn while >= r.  x_0.., y_0.. are the 2 t draws that follow, reduced mod r (a draw is below 2^BITS <= 2r),
// all of them drawn again while two are equal or some x_i + y_j is zero: the generator circomlib's constants came from.
template <class P>
static std::vector<uint32_t> poseidon_generate(int t) {
    const int rp = poseidon_rp(t), rounds = POSEIDON_RF + rp;
    PoseidonGrain grain(P::BITS, t, POSEIDON_RF, rp);
    std::vector<uint32_t> out((size_t)poseidon_consts(t) * P::W);
    uint32_t w[P::W], d[P::W];
    for (int c = 0; c < rounds * t;) {
        grain.draw<P>(w);
        if (!fp_sub_mod_raw<P>(d, w)) continue;   // no borrow: the draw is >= r
        memcpy(&out[(size_t)c * P::W], w, sizeof(w));
        ++c;
    }
    uint32_t xy[10][P::W];
    for (;;) {
        for (int i = 0; i < 2 * t; ++i) {
            grain.draw<P>(w);
            memcpy(xy[i], fp_sub_mod_raw<P>(d, w) ? w : d, sizeof(w));
        }
        bool ok = true;
        for (int i = 0; i < 2 * t; ++i)
            for (int j = 0; j < i; ++j) ok = ok && memcmp(xy[i], xy[j], sizeof(w)) != 0;
        for (int i = 0; i < t && ok; ++i)
            for (int j = 0; j < t; ++j) {
                const Fp<P> sum = fp_add<P>(fp_from_canonical<P>(xy[i]), fp_from_canonical<P>(xy[t + j]));
                ok = ok && !fp_is_zero<P>(sum);
                if (ok) fp_to_canonical<P>(&out[(size_t)(rounds * t + i * t + j) * P::W], fp_inv<P>(sum));
            }
        if (ok) return out;
    }
}

// the kernels' form of the same: N limbs per constant, Montgomery form below p
template <class P>
static std::vector<uint32_t> poseidon_table_host(int t) {
    const std::vector<uint32_t> canon = poseidon_generate<P>(t);
    std::vector<uint32_t> tab((size_t)poseidon_consts(t) * P::N);
    for (int c = 0; c < poseidon_consts(t); ++c) {
        const Fp<P> m = fp_reduce_full<P>(fp_from_canonical<P>(&canon[(size_t)c * P::W]));
        memcpy(&tab[(size_t)c * P::N], m.v, sizeof(m.v));
    }
    return tab;
}

// one device table per (curve, t), made at first use; the one owner, emptied by zk_shutdown
struct PoseidonTables {
    std::mutex mutex;
    uint32_t* tab[2][3] = {};

    template <class P>
    int get(int curve, int t, const uint32_t** out) {
        std::lock_guard<std::mutex> lock(mutex);
        uint32_t*& slot = tab[curve][t - 3];
        if (!slot) {
            const std::vector<uint32_t> host = poseidon_table_host<P>(t);
            uint32_t* d = nullptr;
            ZK_HIP(hipMalloc(&d, host.size() * 4));
            const hipError_t e = hipMemcpy(d, host.data(), host.size() * 4, hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipFree(d);
                ZK_HIP(e);
            }
            slot = d;
        }
        *out = slot;
        return ZK_OK;
    }
    void free_all() {
        std::lock_guard<std::mutex> lock(mutex);
        for (auto& per_curve : tab)
            for (uint32_t*& p : per_curve) {
                (void)hipFree(p);
                p = nullptr;
            }
    }
};
static PoseidonTables g_poseidon;

// ---- host side ----------------------------------------------------------------------------------------------------------

static int poseidon_curve_ok(int curve, const char* who) {
    if (curve != ZK_CURVE_BN254 && curve != ZK_CURVE_BLS12_381) return fail(ZK_ERR_ARG, std::string(who) + ": unknown curve");
    return ZK_OK;
}
static_assert(ZK_CURVE_BN254 == 0 && ZK_CURVE_BLS12_381 == 1, "PoseidonTables is indexed by the curve id");

// `n_in` elements at d_in and `n_out` at d_out, both present and at multiples of 16; they overlap only as d_out == d_in where that is allowed
static int poseidon_spans_ok(const void* d_in, uint64_t n_in, const void* d_out, uint64_t n_out, bool in_place, const char* who) {
    if (!d_in || !d_out) return fail(ZK_ERR_ARG, std::string(who) + ": null pointer");
    if (!aligned16(d_in) || !aligned16(d_out)) return fail(ZK_ERR_ARG, std::string(who) + ": vectors start at a multiple of 16");
    if (in_place && d_in == d_out) return ZK_OK;
    if (ranges_overlap(d_out, n_out * NODE, d_in, n_in * NODE)) return fail(ZK_ERR_ARG, std::string(who) + ": the output overlaps the input");
    return ZK_OK;
}

template <class P, int T>
static int poseidon_perm_impl(int curve, uint64_t n, const void* d_in, void* d_out, hipStream_t st) {
    const uint32_t* tab = nullptr;
    ZK_HIP_RC(g_poseidon.get<P>(curve, T, &tab));
    hipLaunchKernelGGL((poseidon_perm_kernel<P, T>), dim3(fr_blocks(n)), dim3(MLE_TILE), 0, st, n, tab, (const uint32_t*)d_in, (uint32_t*)d_out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P, int T>
static int poseidon_hash_impl(int curve, uint64_t n, const void* d_rows, void* d_out, hipStream_t st) {
    const uint32_t* tab = nullptr;
    ZK_HIP_RC(g_poseidon.get<P>(curve, T, &tab));
    hipLaunchKernelGGL((poseidon_hash_kernel<P, T>), dim3(fr_blocks(n)), dim3(MLE_TILE), 0, st, n, tab, (const uint32_t*)d_rows, (uint32_t*)d_out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int poseidon_sponge_impl(int curve, uint64_t n, const void* d_rows, uint64_t len, void* d_out, hipStream_t st) {
    const uint32_t* tab = nullptr;
    ZK_HIP_RC(g_poseidon.get<P>(curve, 3, &tab));
    const uint64_t len_limbs[4] = {len, 0, 0, 0};
    hipLaunchKernelGGL(poseidon_sponge_kernel<P>, dim3(fr_blocks(n)), dim3(MLE_TILE), 0, st, n, tab, (const uint32_t*)d_rows, len, fr_mont<P>(len_limbs),
                       (uint32_t*)d_out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

template <class P>
static int poseidon_build_impl(int curve, uint64_t n, void* d_tree, hipStream_t st) {
    if (n == 1) return ZK_OK;   // one leaf is its own root
    const uint32_t* tab = nullptr;
    ZK_HIP_RC(g_poseidon.get<P>(curve, 3, &tab));
    return tree_build<NODE>(n, d_tree, [=](uint64_t width, const uint8_t* child, uint8_t* parent) {
        hipLaunchKernelGGL(poseidon_level_kernel<P>, dim3(fr_blocks((width + 1) / 2)), dim3(MLE_TILE), 0, st, width, tab, (const uint32_t*)child,
                           (uint32_t*)parent);
    });
}

// CALL(P, T) for the (curve, t) pair; both have been checked
#define ZK_DISPATCH_POSEIDON(curve, t, CALL)                                       \
    do {                                                                           \
        if ((curve) == ZK_CURVE_BN254) {                                           \
            if ((t) == 3) { CALL(::zkmi::BnFrParams, 3); }                         \
            else if ((t) == 4) { CALL(::zkmi::BnFrParams, 4); }                    \
            else { CALL(::zkmi::BnFrParams, 5); }                                  \
        } else {                                                                   \
            if ((t) == 3) { CALL(::zkmi::BlsFrParams, 3); }                        \
            else if ((t) == 4) { CALL(::zkmi::BlsFrParams, 4); }                   \
            else { CALL(::zkmi::BlsFrParams, 5); }                                 \
        }                                                                          \
    } while (0)

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_poseidon_params(int curve, int t, int* rf, int* rp, uint64_t* out) {
    ZK_HIP_RC(poseidon_curve_ok(curve, "poseidon_params"));
    if (t < 3 || t > 5) return fail(ZK_ERR_ARG, "poseidon_params: the state has 3, 4 or 5 elements");
    if (rf) *rf = POSEIDON_RF;
    if (rp) *rp = poseidon_rp(t);
    if (!out) return ZK_OK;
    const std::vector<uint32_t> canon = curve == ZK_CURVE_BN254 ? poseidon_generate<BnFrParams>(t) : poseidon_generate<BlsFrParams>(t);
    memcpy(out, canon.data(), canon.size() * 4);   // 8 words are 4 little-endian limbs
    return ZK_OK;
}

int zk_poseidon_perm_dev(int curve, int t, uint64_t n, const void* d_in, void* d_out, void* stream) {
    ZK_HIP_RC(poseidon_curve_ok(curve, "poseidon_perm"));
    if (t < 3 || t > 5) return fail(ZK_ERR_ARG, "poseidon_perm: the state has 3, 4 or 5 elements");
    ZK_HIP_RC(leaves_in_range(n, "poseidon_perm"));
    ZK_HIP_RC(poseidon_spans_ok(d_in, n * t, d_out, n * t, true, "poseidon_perm"));
#define CALL(P, T) return poseidon_perm_impl<P, T>(curve, n, d_in, d_out, (hipStream_t)stream)
    ZK_DISPATCH_POSEIDON(curve, t, CALL);
#undef CALL
}

int zk_poseidon_hash_dev(int curve, int k, uint64_t n, const void* d_rows, void* d_out, void* stream) {
    ZK_HIP_RC(poseidon_curve_ok(curve, "poseidon_hash"));
    if (k < 2 || k > 4) return fail(ZK_ERR_ARG, "poseidon_hash: a row has 2, 3 or 4 elements");
    ZK_HIP_RC(leaves_in_range(n, "poseidon_hash"));
    ZK_HIP_RC(poseidon_spans_ok(d_rows, n * k, d_out, n, false, "poseidon_hash"));
#define CALL(P, T) return poseidon_hash_impl<P, T>(curve, n, d_rows, d_out, (hipStream_t)stream)
    ZK_DISPATCH_POSEIDON(curve, k + 1, CALL);
#undef CALL
}

int zk_poseidon_sponge_rows_dev(int curve, uint64_t n, const void* d_rows, uint64_t row_elems, void* d_digests, void* stream) {
    ZK_HIP_RC(poseidon_curve_ok(curve, "poseidon_sponge_rows"));
    ZK_HIP_RC(leaves_in_range(n, "poseidon_sponge_rows"));
    if (row_elems == 0 || row_elems > POSEIDON_MAX_ROW) return fail(ZK_ERR_ARG, "poseidon_sponge_rows: a row has 1 to 2^20 elements");
    ZK_HIP_RC(poseidon_spans_ok(d_rows, n * row_elems, d_digests, n, false, "poseidon_sponge_rows"));
#define CALL(P) return poseidon_sponge_impl<P>(curve, n, d_rows, row_elems, d_digests, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_poseidon_merkle_build_dev(int curve, uint64_t n, void* d_tree, void* stream) {
    ZK_HIP_RC(poseidon_curve_ok(curve, "poseidon_merkle_build"));
    ZK_HIP_RC(tree_build_args("poseidon_merkle_build", n, d_tree));
#define CALL(P) return poseidon_build_impl<P>(curve, n, d_tree, (hipStream_t)stream)
    ZK_DISPATCH_FR(curve, CALL);
#undef CALL
}

int zk_poseidon_merkle_paths_dev(uint64_t n, const void* d_tree, uint64_t k, const void* d_indices, void* d_paths, void* stream) {
    return tree_paths<NODE>("poseidon_merkle_paths", n, d_tree, k, d_indices, d_paths, (hipStream_t)stream);
}

// the hook of host.hip (zk_shutdown)
void zk_poseidon_free_cache(void) { g_poseidon.free_all(); }

}  // extern "C"
