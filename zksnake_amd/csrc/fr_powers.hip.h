// fr_powers.hip.h -- powers g^e of a host scalar inside a kernel over Fr WITHOUT a table (rangeproof.hip: y^k, y^-k, z^(2+j);
// pcs.hip: the opening point's z^j).  The squarings g^(2^t), t <= RP_SEED_BITS, travel as kernel arguments; a thread builds the power
// of its first index from them (one product per set bit; bits 6 and up are the same across a wave, so those branches are uniform)
// and steps by g^(2^18) per grid-stride item: the stride is 2^18 whenever a thread takes a second item.
#pragma once
#include "fr_sum.hip.h"

namespace zkmi {

constexpr int RP_SEED_BITS = 18;             // log2(FR_MAX_BLOCKS * MLE_TILE): a thread's first index has at most this many bits
static_assert((1u << RP_SEED_BITS) == FR_MAX_BLOCKS * MLE_TILE, "the step of a power is the stride of the capped grid");

// g^(2^t) R for t <= RP_SEED_BITS; the last one is the step of a grid-stride loop
template <class P>
struct RpPowers {
    Fp<P> sq[RP_SEED_BITS + 1];
};

// acc g^e for e < 2^bits
template <class P>
__device__ __forceinline__ Fp<P> rp_power(const RpPowers<P>& g, uint64_t e, int bits, Fp<P> acc) {
    for (int t = 0; t < bits; ++t)
        if ((e >> t) & 1) acc = fp_mul<P>(acc, g.sq[t]);
    return acc;
}

template <class P>
static RpPowers<P> rp_squarings(const uint64_t* g) {
    RpPowers<P> out;
    out.sq[0] = fr_mont<P>(g);
    for (int t = 1; t <= RP_SEED_BITS; ++t) out.sq[t] = fp_mul<P>(out.sq[t - 1], out.sq[t - 1]);
    return out;
}

}  // namespace zkmi
