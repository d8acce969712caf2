// ipa_chain.hip.h -- the challenge chain of the inner-product argument's verifier, s_i = prod_{t < log_n} (bit (log_n-1-t) of i ?
// u_t : u_t^-1) and its inverse, as both verify-scalars kernels run it (ipa.hip, rangeproof.hip).
#pragma once
#include "fr_sum.hip.h"

namespace zkmi {

template <class P>
struct IpaChain {
    Fp<P> u_m[ZK_IPA_MAX_LOG], ui_m[ZK_IPA_MAX_LOG];  // u_t R, u_t^-1 R
};

// the first log_n challenges from the host's u, u_inv (4 limbs each); the rest zero
template <class P>
static IpaChain<P> ipa_chain_fill(int log_n, const uint64_t* u, const uint64_t* u_inv) {
    IpaChain<P> c;
    for (int t = 0; t < ZK_IPA_MAX_LOG; ++t) {
        c.u_m[t] = t < log_n ? fr_mont<P>(u + 4 * t) : fp_zero<P>();
        c.ui_m[t] = t < log_n ? fr_mont<P>(u_inv + 4 * t) : fp_zero<P>();
    }
    return c;
}

// sa *= s_i, sb *= s_i^-1: log_n products each
template <class P>
__device__ __forceinline__ void ipa_chain_run(const IpaChain<P>& c, int log_n, uint64_t i, Fp<P>& sa, Fp<P>& sb) {
    for (int t = 0; t < log_n; ++t) {
        const bool bit = (i >> (log_n - 1 - t)) & 1;
        sa = fp_mul<P>(sa, bit ? c.u_m[t] : c.ui_m[t]);
        sb = fp_mul<P>(sb, bit ? c.ui_m[t] : c.u_m[t]);
    }
}

}  // namespace zkmi
