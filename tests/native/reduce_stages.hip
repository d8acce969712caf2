// Stage harness for the lane-pair arithmetic behind the MSM's accumulate kernel: pair_add (csrc/pair.hip.h), the pair-split G2
// bucket step sp_add_affine (csrc/fp2_split.hip.h) and the three PRODUCTION kernels of csrc/msm_reduce.hip.h (combine_kernel,
// strided_sum_kernel, weighted_sum_kernel), launched through the launchers of that header (launch_combine, launch_strided_sum,
// launch_weighted_sum), the same calls MsmPlan (msm_impl.hip.h) makes.  Device build only (the library's own hipcc pipeline,
// gfx950), driven through ctypes by tests/test_gpu_msm_reduce_stages.py.
//   group: 0 BN254 G1, 1 BN254 G2, 2 BLS12-381 G1, 3 BLS12-381 G2
// Register form = the 29-bit limbs of Fp<P>::v as they sit in registers (F::REGS words per coordinate, Fp2 as c0 | c1); memory
// form = packed 32-bit words (F::LIMBS per coordinate), a point as the XYZZ row [X | Y | ZZ | ZZZ].
//   rs_pair_add    record in: P then Q, each X | Y | ZZ | ZZZ in register form (8 F::REGS words); out: the sum (4 F::REGS words).
//                  One lane PAIR per record, 32 records per wave, every record takes its own branch.
//   rs_split_step  the record of field_edges.hip's FE_G2_STEP (16 N words in, 8 N out), sp_add_affine on a lane pair
//   rs_lane_step   the same record through the one-lane xyzz_add_affine_mem (what sp_add_affine must equal)
// Every entry point returns 0, 1 for a refused argument, 3 for a HIP error, 4 for an index that would leave an array: the
// launchers of the production kernels recompute the largest index of each job on the host and refuse instead of launching.
#include <cstdint>
#include <cstring>
#include <algorithm>
#include <hip/hip_runtime.h>
#include "../../zksnake_amd/csrc/msm_reduce.hip.h"
#include "../../zksnake_amd/csrc/fp2_split.hip.h"

using namespace zkmi;

constexpr uint64_t RS_MAX_COUNT = 1ull << 20;

template <class T>
__device__ __forceinline__ T rs_ld(const uint32_t* w) {
    T r;
    memcpy(&r, w, sizeof(T));
    return r;
}
template <class T>
__device__ __forceinline__ void rs_st(uint32_t* w, const T& a) {
    memcpy(w, &a, sizeof(T));
}

template <class F>
__global__ __launch_bounds__(64) void rs_pair_add_kernel(uint32_t count, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    typedef typename F::T T;
    constexpr int R = F::REGS;
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t rec = gid >> 1;
    const bool odd = (gid & 1) != 0;
    if (rec >= count) return;   // both lanes of a pair leave together
    const uint32_t* r = in + (size_t)rec * 8 * R;
    const HalfPt<F> p = {rs_ld<T>(r + (odd ? 1 : 0) * R), rs_ld<T>(r + (odd ? 3 : 2) * R)};
    const HalfPt<F> q = {rs_ld<T>(r + (odd ? 5 : 4) * R), rs_ld<T>(r + (odd ? 7 : 6) * R)};
    const HalfPt<F> s = pair_add<F>(p, q, odd);
    uint32_t* o = out + (size_t)rec * 4 * R;
    rs_st<T>(o + (odd ? 1 : 0) * R, s.a);
    rs_st<T>(o + (odd ? 3 : 2) * R, s.b);
}

template <class P>
__global__ __launch_bounds__(64) void rs_split_step_kernel(uint32_t count, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    constexpr int N = P::N, W = P::W;
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t rec = gid >> 1;
    const bool odd = (gid & 1) != 0;
    if (rec >= count) return;
    const uint32_t* r = in + (size_t)rec * 16 * N;
    const int c = odd ? 1 : 0;
    const uint32_t* a = r + 4 * N;   // X.c0 X.c1 Y.c0 Y.c1 ZZ.c0 ZZ.c1 ZZZ.c0 ZZZ.c1
    SplitXYZZ<P> acc = {rs_ld<Fp<P>>(a + (0 + c) * N), rs_ld<Fp<P>>(a + (2 + c) * N), rs_ld<Fp<P>>(a + (4 + c) * N), rs_ld<Fp<P>>(a + (6 + c) * N)};
    const Fp<P> qx = fp_load<P>(r + c * W), qy = fp_load<P>(r + 2 * W + c * W);
    sp_add_affine<P>(acc, qx, qy, r[12 * N] != 0, odd);
    uint32_t* o = out + (size_t)rec * 8 * N;
    rs_st<Fp<P>>(o + (0 + c) * N, acc.X);
    rs_st<Fp<P>>(o + (2 + c) * N, acc.Y);
    rs_st<Fp<P>>(o + (4 + c) * N, acc.ZZ);
    rs_st<Fp<P>>(o + (6 + c) * N, acc.ZZZ);
}

template <class P>
__global__ __launch_bounds__(64) void rs_lane_step_kernel(uint32_t count, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    typedef Fp2Ops<P> F;
    constexpr int N = P::N;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t* r = in + (size_t)i * 16 * N;
    XYZZ<F> acc = rs_ld<XYZZ<F>>(r + 4 * N);
    xyzz_add_affine_mem<F>(acc, r, r[12 * N] != 0);
    rs_st<XYZZ<F>>(out + (size_t)i * 8 * N, acc);
}

#define RS_HIP(expr)                                     \
    do {                                                 \
        if ((expr) != hipSuccess) { rc = 3; goto done; } \
    } while (0)

struct DevBuf {
    uint32_t* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

static int rs_words(int group) {   // F::LIMBS
    switch (group) {
    case 0: return Bn254G1::F::LIMBS;
    case 1: return Bn254G2::F::LIMBS;
    case 2: return Bls381G1::F::LIMBS;
    default: return Bls381G2::F::LIMBS;
    }
}
static int rs_regs(int group) {   // F::REGS
    switch (group) {
    case 0: return Bn254G1::F::REGS;
    case 1: return Bn254G2::F::REGS;
    case 2: return Bls381G1::F::REGS;
    default: return Bls381G2::F::REGS;
    }
}
static bool rs_group_ok(int group) { return group >= 0 && group <= 3; }

// copies `words` u32 to a fresh device buffer (at least one word is allocated, so an empty array still has an address)
static int rs_upload(DevBuf& d, const uint32_t* host, size_t words) {
    if (hipMalloc(&d.p, std::max<size_t>(words, 4) * 4) != hipSuccess) return 3;
    if (hipMemset(d.p, 0, std::max<size_t>(words, 4) * 4) != hipSuccess) return 3;
    if (words && hipMemcpy(d.p, host, words * 4, hipMemcpyHostToDevice) != hipSuccess) return 3;
    return 0;
}
static int rs_finish(DevBuf& d, uint32_t* host, size_t words) {
    if (hipGetLastError() != hipSuccess) return 3;
    if (hipDeviceSynchronize() != hipSuccess) return 3;
    if (words && hipMemcpy(host, d.p, words * 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    return 0;
}

extern "C" int rs_pair_add(int group, uint64_t count, const uint32_t* in, uint32_t* out) {
    if (!rs_group_ok(group) || count > RS_MAX_COUNT || (count && (!in || !out))) return 1;
    if (count == 0) return 0;
    const size_t R = rs_regs(group);
    DevBuf d_in, d_out;
    int rc;
    if ((rc = rs_upload(d_in, in, count * 8 * R))) return rc;
    if (hipMalloc(&d_out.p, count * 4 * R * 4) != hipSuccess || hipMemset(d_out.p, 0, count * 4 * R * 4) != hipSuccess) return 3;
    const dim3 grid((unsigned)((2 * count + 63) / 64)), block(64);
    switch (group) {
    case 0: hipLaunchKernelGGL(rs_pair_add_kernel<Bn254G1::F>, grid, block, 0, 0, (uint32_t)count, d_in.p, d_out.p); break;
    case 1: hipLaunchKernelGGL(rs_pair_add_kernel<Bn254G2::F>, grid, block, 0, 0, (uint32_t)count, d_in.p, d_out.p); break;
    case 2: hipLaunchKernelGGL(rs_pair_add_kernel<Bls381G1::F>, grid, block, 0, 0, (uint32_t)count, d_in.p, d_out.p); break;
    default: hipLaunchKernelGGL(rs_pair_add_kernel<Bls381G2::F>, grid, block, 0, 0, (uint32_t)count, d_in.p, d_out.p); break;
    }
    return rs_finish(d_out, out, count * 4 * R);
}

// lanes: 2 = sp_add_affine on a lane pair, 1 = xyzz_add_affine_mem on one lane; G2 groups only
static int rs_step(int group, int lanes, uint64_t count, const uint32_t* in, uint32_t* out) {
    if ((group != 1 && group != 3) || count > RS_MAX_COUNT || (count && (!in || !out))) return 1;
    if (count == 0) return 0;
    const size_t N = group == 1 ? BnFqParams::N : BlsFqParams::N;
    DevBuf d_in, d_out;
    int rc;
    if ((rc = rs_upload(d_in, in, count * 16 * N))) return rc;
    if (hipMalloc(&d_out.p, count * 8 * N * 4) != hipSuccess || hipMemset(d_out.p, 0, count * 8 * N * 4) != hipSuccess) return 3;
    const dim3 grid((unsigned)((lanes * count + 63) / 64)), block(64);
    if (lanes == 2) {
        if (group == 1) hipLaunchKernelGGL(rs_split_step_kernel<BnFqParams>, grid, block, 0, 0, (uint32_t)count, d_in.p, d_out.p);
        else hipLaunchKernelGGL(rs_split_step_kernel<BlsFqParams>, grid, block, 0, 0, (uint32_t)count, d_in.p, d_out.p);
    } else {
        if (group == 1) hipLaunchKernelGGL(rs_lane_step_kernel<BnFqParams>, grid, block, 0, 0, (uint32_t)count, d_in.p, d_out.p);
        else hipLaunchKernelGGL(rs_lane_step_kernel<BlsFqParams>, grid, block, 0, 0, (uint32_t)count, d_in.p, d_out.p);
    }
    return rs_finish(d_out, out, count * 8 * N);
}
extern "C" int rs_split_step(int group, uint64_t count, const uint32_t* in, uint32_t* out) { return rs_step(group, 2, count, in, out); }
extern "C" int rs_lane_step(int group, uint64_t count, const uint32_t* in, uint32_t* out) { return rs_step(group, 1, count, in, out); }

// ---- the production kernels ------------------------------------------------------------------------------------------------

// job words: n_out, per_group, group_stride, outer, inner, count, out_offset, split, outer2, in_offset (SumJob's members in order)
static SumJob rs_job(const uint32_t* w) {
    SumJob j = {w[0], w[1], w[2], w[3], w[4], w[5], w[6]};
    j.split = w[7];
    j.outer2 = w[8];
    j.in_offset = w[9];
    return j;
}
// largest point index a job reads / writes (the kernel's own index expression, enumerated); false when it leaves an array
static bool rs_job_inside(const SumJob& j, uint64_t n_in, uint64_t n_out) {
    if (j.n_out == 0) return true;
    if (j.per_group == 0 || j.split == 0 || j.count == 0) return false;
    for (uint32_t o = 0; o < j.n_out; ++o) {
        const uint32_t x = o % j.per_group;
        const uint64_t base = (uint64_t)j.in_offset + (uint64_t)(o / j.per_group) * j.group_stride + (uint64_t)(x / j.split) * j.outer + (uint64_t)(x % j.split) * j.outer2;
        if (base + (uint64_t)(j.count - 1) * j.inner >= n_in) return false;
    }
    return (uint64_t)j.out_offset + j.n_out <= n_out;
}

extern "C" int rs_strided_sum(int group, const uint32_t* in, uint64_t n_in_points, uint32_t* out, uint64_t n_out_points,
                              const uint32_t* job0, const uint32_t* job1, uint32_t lpo) {
    if (!rs_group_ok(group) || !in || !out || !job0 || !job1 || n_in_points > RS_MAX_COUNT || n_out_points > RS_MAX_COUNT) return 1;
    if (lpo < 2 || lpo > 64 || (lpo & (lpo - 1))) return 1;
    const SumJob j0 = rs_job(job0), j1 = rs_job(job1);
    if ((uint64_t)j0.n_out + j1.n_out == 0 || (uint64_t)j0.n_out + j1.n_out > RS_MAX_COUNT) return 1;
    if (!rs_job_inside(j0, n_in_points, n_out_points) || !rs_job_inside(j1, n_in_points, n_out_points)) return 4;
    const size_t XW = 4 * (size_t)rs_words(group);
    DevBuf d_in, d_out;
    int rc;
    if ((rc = rs_upload(d_in, in, n_in_points * XW)) || (rc = rs_upload(d_out, out, n_out_points * XW))) return rc;
    switch (group) {
    case 0: launch_strided_sum<Bn254G1>(d_in.p, d_out.p, j0, j1, lpo, nullptr); break;
    case 1: launch_strided_sum<Bn254G2>(d_in.p, d_out.p, j0, j1, lpo, nullptr); break;
    case 2: launch_strided_sum<Bls381G1>(d_in.p, d_out.p, j0, j1, lpo, nullptr); break;
    default: launch_strided_sum<Bls381G2>(d_in.p, d_out.p, j0, j1, lpo, nullptr); break;
    }
    return rs_finish(d_out, out, n_out_points * XW);
}

// n0 arrays of m0 points in in0 and n0 arrays of m1 points in in1 (the row sums and the column sums of n0 bucket sets);
// out: (S, T) per block of WS_BLOCK points, n0 * (ceil(m0 / WS_BLOCK) + ceil(m1 / WS_BLOCK)) blocks
extern "C" int rs_weighted_sum(int group, const uint32_t* in0, uint32_t m0, uint32_t n0, const uint32_t* in1, uint32_t m1, uint32_t* out) {
    if (!rs_group_ok(group) || !in0 || !in1 || !out || m0 == 0 || m1 == 0 || n0 == 0 || m0 > 65536 || m1 > 65536 || n0 > 64) return 1;
    const size_t XW = 4 * (size_t)rs_words(group);
    const uint32_t bpa0 = (m0 + WS_BLOCK - 1) / WS_BLOCK, bpa1 = (m1 + WS_BLOCK - 1) / WS_BLOCK;
    const unsigned blocks = n0 * (bpa0 + bpa1);
    DevBuf d0, d1, d_out;
    int rc;
    if ((rc = rs_upload(d0, in0, (size_t)n0 * m0 * XW)) || (rc = rs_upload(d1, in1, (size_t)n0 * m1 * XW)) ||
        (rc = rs_upload(d_out, out, (size_t)blocks * 2 * XW))) return rc;
    switch (group) {
    case 0: launch_weighted_sum<Bn254G1>(d0.p, m0, n0, d1.p, m1, d_out.p, nullptr); break;
    case 1: launch_weighted_sum<Bn254G2>(d0.p, m0, n0, d1.p, m1, d_out.p, nullptr); break;
    case 2: launch_weighted_sum<Bls381G1>(d0.p, m0, n0, d1.p, m1, d_out.p, nullptr); break;
    default: launch_weighted_sum<Bls381G2>(d0.p, m0, n0, d1.p, m1, d_out.p, nullptr); break;
    }
    return rs_finish(d_out, out, (size_t)blocks * 2 * XW);
}

// run_start: n_keys + 1 offsets into partials (n_partials rows); big_list: n_keys entries, wave-tier keys from the front,
// workgroup-tier keys from the back; big_count: the two lengths; buckets: n_keys rows, read back after the launch
extern "C" int rs_combine(int group, const uint32_t* partials, uint64_t n_partials, const uint32_t* run_start, uint32_t n_keys,
                          const uint32_t* big_list, const uint32_t* big_count, uint32_t* buckets) {
    if (!rs_group_ok(group) || !partials || !run_start || !big_list || !big_count || !buckets || n_keys == 0 || n_keys > RS_MAX_COUNT ||
        n_partials > RS_MAX_COUNT) return 1;
    // every index the kernel forms, checked here: monotone run offsets inside partials, listed keys inside [0, n_keys)
    if (run_start[0] != 0 || run_start[n_keys] != n_partials) return 4;
    for (uint32_t k = 0; k < n_keys; ++k) if (run_start[k] > run_start[k + 1]) return 4;
    if ((uint64_t)big_count[0] + big_count[1] > n_keys) return 4;
    for (uint32_t b = 0; b < big_count[0]; ++b) if (big_list[b] >= n_keys) return 4;
    for (uint32_t b = 0; b < big_count[1]; ++b) if (big_list[n_keys - 1 - b] >= n_keys) return 4;
    const size_t XW = 4 * (size_t)rs_words(group);
    DevBuf d_part, d_runs, d_list, d_count, d_buckets;
    int rc;
    if ((rc = rs_upload(d_part, partials, n_partials * XW)) || (rc = rs_upload(d_runs, run_start, (size_t)n_keys + 1)) ||
        (rc = rs_upload(d_list, big_list, n_keys)) || (rc = rs_upload(d_count, big_count, 2)) || (rc = rs_upload(d_buckets, buckets, n_keys * XW))) return rc;
    switch (group) {
    case 0: launch_combine<Bn254G1>(d_part.p, d_runs.p, n_keys, d_list.p, d_count.p, d_buckets.p, nullptr); break;
    case 1: launch_combine<Bn254G2>(d_part.p, d_runs.p, n_keys, d_list.p, d_count.p, d_buckets.p, nullptr); break;
    case 2: launch_combine<Bls381G1>(d_part.p, d_runs.p, n_keys, d_list.p, d_count.p, d_buckets.p, nullptr); break;
    default: launch_combine<Bls381G2>(d_part.p, d_runs.p, n_keys, d_list.p, d_count.p, d_buckets.p, nullptr); break;
    }
    return rs_finish(d_buckets, buckets, n_keys * XW);
}

// the tier constants the expected-value builders of the test must agree with
extern "C" void rs_constants(uint32_t* out) {
    out[0] = COMBINE_SMALL_MAX;
    out[1] = COMBINE_WAVE_MAX;
    out[2] = COMBINE_WAVE_BLOCKS;
    out[3] = COMBINE_BIG_BLOCKS;
    out[4] = COMBINE_THREADS;
    out[5] = WS_BLOCK;
}
