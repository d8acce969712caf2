// ntt_lazy.hip.h -- the lazy-range limb steps of the NTT butterfly passes (ntt.hip), host + device so that the host build of
// tests/native/field_edges.hip runs the same code as the kernels.
#pragma once
#include "field.hip.h"

namespace zkmi {

#if !defined(__HIP_DEVICE_COMPILE__)
// host side of the one multiply-high of lz_reduce
inline uint32_t lz_umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
#else
__device__ __forceinline__ uint32_t lz_umulhi(uint32_t a, uint32_t b) { return __umulhi(a, b); }
#endif

// ---- lazy-range arithmetic of the butterfly passes ---------------------------------------------------------------
// A radix-4 step of the passes (ntt.hip) used to spend a fifth of its VALU instructions on four range-selecting additions
// (fp_add: two candidate results carried through one pass, then a select).  Inside a pass the values now live in a wider
// range instead: every element of the LDS tile is NORMALISED (limbs < 2^29) with value < 9p, sums are formed limb by limb
// without carries, and only the one output per step that is a sum of sums is brought back -- by ONE estimated multiple of
// 8p and a signed carry pass.  For a step on (x00, x01, x10, x11), all < 9p:
//     a0 = x00 + x10, b0 = x01 + x11             limb-wise: limbs < 2^30, value < 18p
//     a1 = w (x00 - x10 + 18p*), b1 = w' (..)    operand limbs < 3 2^29, value < 27p; product < 2p, normalised
//     x00' = reduce8(a0 + b0)                    limbs < 2^31, value < 36p  ->  normalised, < 8.7p
//     x01' = w2 (a0 - b0 + 36p*)                 operand limbs < 5 2^29, value < 54p: columns 9 (5 + 1) 2^58 < 2^64
//     x10' = normalise(a1 + b1)                  < 4p
//     x11' = w2 (a1 - b1 + 4p*)                  as before
// (kp* = k p written with borrow-proof limbs).  A Montgomery product needs (a/p)(b/p) <= R/p = 2^261/p (168 for BN254 Fr,
// 70.7 for BLS12-381 Fr): the twiddles of the 9-word table are canonical (< p), so 54 * 1 fits both fields.
// tools/model_lazy_ntt.py replays these steps on integers with the limb and column bounds asserted.

// k p as normalised 29-bit limbs, at compile time
template <class P>
struct LimbConst { uint32_t v[P::N]; };
template <class P>
constexpr LimbConst<P> times_p(uint32_t k) {
    LimbConst<P> r{};
    uint64_t carry = 0;
    for (int i = 0; i < P::N; ++i) {
        const uint64_t t = (uint64_t)P::M[i] * k + carry;
        r.v[i] = i < P::N - 1 ? (uint32_t)(t & LIMB_MASK) : (uint32_t)t;
        carry = t >> LIMB_BITS;
    }
    return r;
}

// a + b, limb by limb (no carries): the caller accounts for the limb width
template <class P>
ZK_HD Fp<P> lz_add(const Fp<P>& a, const Fp<P>& b) {
    Fp<P> r;
#pragma unroll
    for (int i = 0; i < P::N; ++i) r.v[i] = a.v[i] + b.v[i];
    return r;
}

// a - b + K p with borrow-proof limbs: every limb of K p but the top one borrows 2^BITS from the limb above, so no limb goes
// negative for b with limbs < 2^BITS and value <= K p / 2.  One operand of a product only.
template <class P, int K, int BITS>
ZK_HD Fp<P> lz_sub(const Fp<P>& a, const Fp<P>& b) {
    constexpr LimbConst<P> kp = times_p<P>(K);
    Fp<P> r;
#pragma unroll
    for (int i = 0; i < P::N; ++i) {
        const uint32_t c = kp.v[i] + (i < P::N - 1 ? (1u << BITS) : 0u) - (i > 0 ? (1u << (BITS - LIMB_BITS)) : 0u);
        r.v[i] = a.v[i] + c - b.v[i];
    }
    return r;
}

// carry pass: limbs < 2^31 in, normalised limbs out, same value
template <class P>
ZK_HD Fp<P> lz_norm(const Fp<P>& a) {
    Fp<P> r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < P::N; ++i) {
        const uint32_t t = a.v[i] + c;
        if (i < P::N - 1) {
            r.v[i] = t & LIMB_MASK;
            c = t >> LIMB_BITS;
        } else {
            r.v[i] = t;
        }
    }
    return r;
}

// a - k U p for the estimate k = floor(top(a) / (top(U p) + 1)) (one multiply-high), then a signed carry pass: limbs < 2^31 and
// value < 4.5 U p in, normalised limbs and value < 1.09 U p out (k <= 4, so k * limb(U p) < 2^31 and every limb difference
// fits a signed 32-bit register).  U = 8 inside a pass, U = 2 on the way to a canonical result.
template <class P, int U>
ZK_HD Fp<P> lz_reduce(const Fp<P>& a) {
    constexpr int N = P::N;
    constexpr LimbConst<P> up = times_p<P>(U);
    constexpr uint32_t MAGIC = (uint32_t)((1ull << 32) / ((uint64_t)up.v[N - 1] + 1));
    const uint32_t t = a.v[N - 1] + (a.v[N - 2] >> LIMB_BITS);
    const uint32_t k = lz_umulhi(t, MAGIC);
    Fp<P> r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int32_t d = (int32_t)(a.v[i] - k * up.v[i]) + c;
        if (i < N - 1) {
            r.v[i] = (uint32_t)d & LIMB_MASK;
            c = d >> LIMB_BITS;
        } else {
            r.v[i] = (uint32_t)d;
        }
    }
    return r;
}

// normalised, value < 9p  ->  canonical: one estimated multiple of 2p, then two conditional subtractions of p
template <class P>
ZK_HD Fp<P> lz_canonical(const Fp<P>& a) {
    return fp_reduce_full<P>(fp_reduce_full<P>(lz_reduce<P, 2>(a)));
}

}  // namespace zkmi
