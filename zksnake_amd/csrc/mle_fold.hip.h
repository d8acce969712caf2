// mle_fold.hip.h -- what the LDS-tiled variable folds share (mle.hip: fix / evaluate; mlpcs.hip: the quotient chain of a
// multilinear opening): the per-launch challenges, one fold step, and the size of a chain's intermediate tables.
//
// A launch folds f <= MLE_TILE_LOG variables of a table of n elements: one workgroup of MLE_TILE threads per tile of
// min(n, MLE_TILE) contiguous elements, (tile >> f) survivors per tile.  In every in-tile level thread t reads elements 2t and 2t+1
// of the tile and the level's result goes back to element t, so the tile stays compact: the stride between neighbouring lanes is
// two elements for the reads and one for the write at EVERY level, the deep ones included.
#pragma once
#include "fr_sum.hip.h"

namespace zkmi {

template <class P>
struct FixArgs {
    Fp<P> r_m[MLE_TILE_LOG];  // r R: mont(d, r R) = r d
};

// the challenges r[0 .. f-1] (4 limbs each, any value) of one launch; zero past f
template <class P>
static FixArgs<P> fix_args(const uint64_t* r, int f) {
    FixArgs<P> a;
    for (int s = 0; s < MLE_TILE_LOG; ++s) a.r_m[s] = s < f ? fr_mont<P>(r + 4 * s) : fp_zero<P>();
    return a;
}

// lo + r d for d = hi - lo, below 2r
template <class P>
__device__ __forceinline__ Fp<P> fold_step(const Fp<P>& lo, const Fp<P>& d, const Fp<P>& r_m) {
    return fp_add<P>(lo, fp_mul<P>(d, r_m));
}

// device elements a chain of fold passes over k variables needs between its first and its last pass
static uint64_t fix_work_elems(int log_n, int k) {
    const int passes = (k + MLE_TILE_LOG - 1) / MLE_TILE_LOG;
    if (passes < 2) return 0;
    return (1ull << (log_n - MLE_TILE_LOG)) + (passes > 2 ? 1ull << (log_n - 2 * MLE_TILE_LOG) : 0);
}

}  // namespace zkmi
