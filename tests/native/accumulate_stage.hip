// Stage harness for stage 5 of the MSM pipeline: the PRODUCTION kernels of csrc/msm_accumulate.hip.h (accumulate_kernel,
// accumulate_split_kernel, bases_to_mont_kernel) through the launchers of that header (launch_accumulate, launch_bases_to_mont),
// the same calls MsmPlan (msm_impl.hip.h) makes, on layouts built by tests/test_gpu_msm_accumulate_stage.py.  Device build only
// (the library's own hipcc pipeline, gfx950), driven through ctypes.  A second compilation of the header, with the default scheduling strategy for every
// group (the library compiles three of the groups' accumulate kernels with max-ilp scheduling): what is tested is the source.
//   group: 0 BN254 G1, 1 BN254 G2, 2 BLS12-381 G1, 3 BLS12-381 G2
// Returns 0, 1 for a refused argument, 3 for a HIP error, 4 for a layout under which the kernel would form an index outside one
// of its arrays: as_accumulate walks the layout on the host first and refuses instead of launching.
#include <cstdint>
#include <cstring>
#include <algorithm>
#include <hip/hip_runtime.h>
#include "../../zksnake_amd/csrc/msm_accumulate.hip.h"

using namespace zkmi;

constexpr uint64_t AS_MAX_COUNT = 1ull << 22;

struct DevBuf {
    uint32_t* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

static int as_words(int group) {   // F::LIMBS
    switch (group) {
    case 0: return Bn254G1::F::LIMBS;
    case 1: return Bn254G2::F::LIMBS;
    case 2: return Bls381G1::F::LIMBS;
    default: return Bls381G2::F::LIMBS;
    }
}
static bool as_group_ok(int group) { return group >= 0 && group <= 3; }

static int as_upload(DevBuf& d, const uint32_t* host, size_t words) {
    if (hipMalloc(&d.p, std::max<size_t>(words, 4) * 4) != hipSuccess) return 3;
    if (hipMemset(d.p, 0, std::max<size_t>(words, 4) * 4) != hipSuccess) return 3;
    if (words && hipMemcpy(d.p, host, words * 4, hipMemcpyHostToDevice) != hipSuccess) return 3;
    return 0;
}
static int as_download(DevBuf& d, uint32_t* host, size_t words) {
    if (words && hipMemcpy(host, d.p, words * 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    return 0;
}

// Every index the kernels form, from their own expressions:
//   bucket_start[0 .. n_keys]   monotone from 0 to `total` (the binary search and the skip loop stay below n_keys + 1 because
//                               every segment starts below bucket_start[n_keys])
//   sorted[e], e < total        its reference below n_rows
//   run_start[key], [key + 1]   run_slot: one run -> buckets[key]; otherwise partials[r0 + t - bucket_start[key] / seg_len], which
//                               is inside [r0, r0 + runs) exactly when run_start holds the run counts of the layout
static bool as_layout_inside(uint64_t n_rows, const uint32_t* sorted, uint64_t total, const uint32_t* bstart, const uint32_t* sstart,
                             uint32_t n_keys, uint32_t seg_len, uint64_t n_partials) {
    if (bstart[0] != 0 || bstart[n_keys] != total || sstart[0] != 0) return false;
    for (uint32_t k = 0; k < n_keys; ++k) {
        const uint32_t s0 = bstart[k], s1 = bstart[k + 1];
        if (s1 < s0) return false;
        const uint32_t runs = s1 > s0 ? 1 + (s1 - 1) / seg_len - s0 / seg_len : 0;
        if (sstart[k + 1] < sstart[k] || sstart[k + 1] - sstart[k] != runs) return false;
    }
    if (sstart[n_keys] > n_partials) return false;
    for (uint64_t e = 0; e < total; ++e) if ((sorted[e] & 0x7FFFFFFFu) >= n_rows) return false;
    return true;
}

// bases: n_rows affine rows (Montgomery, memory form); sorted: `total` entry words; bstart / sstart: n_keys + 1 words each;
// partials: n_partials XYZZ rows, buckets: n_keys XYZZ rows -- both uploaded as given (the caller's sentinel) and read back.
// split != 0: the lane-pair kernel (groups 1 and 3 only)
extern "C" int as_accumulate(int group, int split, const uint32_t* bases, uint64_t n_rows, const uint32_t* sorted, uint64_t total,
                             const uint32_t* bstart, const uint32_t* sstart, uint32_t n_keys, uint32_t seg_len, uint32_t prio_steps,
                             uint32_t* partials, uint64_t n_partials, uint32_t* buckets) {
    if (!as_group_ok(group) || !bases || !sorted || !bstart || !sstart || !partials || !buckets) return 1;
    if (n_keys == 0 || n_keys > AS_MAX_COUNT || n_rows == 0 || n_rows > AS_MAX_COUNT || total > AS_MAX_COUNT || n_partials > AS_MAX_COUNT) return 1;
    if (seg_len == 0 || seg_len > 1024 || prio_steps > 1) return 1;
    if (split && group != 1 && group != 3) return 1;
    if (!as_layout_inside(n_rows, sorted, total, bstart, sstart, n_keys, seg_len, n_partials)) return 4;
    const size_t L = (size_t)as_words(group), AW = 2 * L, XW = 4 * L;
    DevBuf d_bases, d_sorted, d_bstart, d_sstart, d_part, d_buckets;
    int rc;
    if ((rc = as_upload(d_bases, bases, n_rows * AW)) || (rc = as_upload(d_sorted, sorted, total)) || (rc = as_upload(d_bstart, bstart, (size_t)n_keys + 1)) ||
        (rc = as_upload(d_sstart, sstart, (size_t)n_keys + 1)) || (rc = as_upload(d_part, partials, n_partials * XW)) || (rc = as_upload(d_buckets, buckets, n_keys * XW))) return rc;
    const uint64_t lanes_needed = (total + seg_len - 1) / seg_len;
    if (lanes_needed > 0) {   // stage_accumulate never runs on an empty entry list (a zero-size grid is not a launch)
        switch (group) {
        case 0: launch_accumulate<Bn254G1>(false, lanes_needed, d_bases.p, d_sorted.p, d_bstart.p, d_sstart.p, n_keys, seg_len, prio_steps, d_part.p, d_buckets.p, nullptr); break;
        case 1: launch_accumulate<Bn254G2>(split != 0, lanes_needed, d_bases.p, d_sorted.p, d_bstart.p, d_sstart.p, n_keys, seg_len, prio_steps, d_part.p, d_buckets.p, nullptr); break;
        case 2: launch_accumulate<Bls381G1>(false, lanes_needed, d_bases.p, d_sorted.p, d_bstart.p, d_sstart.p, n_keys, seg_len, prio_steps, d_part.p, d_buckets.p, nullptr); break;
        default: launch_accumulate<Bls381G2>(split != 0, lanes_needed, d_bases.p, d_sorted.p, d_bstart.p, d_sstart.p, n_keys, seg_len, prio_steps, d_part.p, d_buckets.p, nullptr); break;
        }
    }
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 3;
    if ((rc = as_download(d_part, partials, n_partials * XW)) || (rc = as_download(d_buckets, buckets, n_keys * XW))) return rc;
    return 0;
}

// in: n canonical affine rows; out: n rows in Montgomery form, or 2n rows (P_i, phi(P_i)) when glv != 0, read back over the
// caller's sentinel.
extern "C" int as_bases_to_mont(int group, const uint32_t* in, uint64_t n, int glv, uint32_t* out) {
    if (!as_group_ok(group) || !in || !out || n == 0 || n > AS_MAX_COUNT || (glv != 0 && glv != 1)) return 1;
    const size_t AW = 2 * (size_t)as_words(group), n_out = (glv ? 2 : 1) * n;
    DevBuf d_in, d_out;
    int rc;
    if ((rc = as_upload(d_in, in, n * AW)) || (rc = as_upload(d_out, out, n_out * AW))) return rc;
    switch (group) {
    case 0: launch_bases_to_mont<Bn254G1>(d_in.p, n, d_out.p, glv, nullptr); break;
    case 1: launch_bases_to_mont<Bn254G2>(d_in.p, n, d_out.p, glv, nullptr); break;
    case 2: launch_bases_to_mont<Bls381G1>(d_in.p, n, d_out.p, glv, nullptr); break;
    default: launch_bases_to_mont<Bls381G2>(d_in.p, n, d_out.p, glv, nullptr); break;
    }
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 3;
    return as_download(d_out, out, n_out * AW);
}

extern "C" void as_constants(uint32_t* out) {
    out[0] = COMBINE_SMALL_MAX;
    out[1] = COMBINE_WAVE_MAX;
}
