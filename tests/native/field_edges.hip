// Edge-of-range harness for the field primitives of csrc/field.hip.h, the lazy NTT steps of csrc/ntt_lazy.hip.h and the relaxed
// bucket step of csrc/curve.hip.h.  One source, two builds (tests/test_field_edges.py):
//   g++ -x c++      fe_run loops over the records on the CPU (also built with -fsanitize=undefined)
//   hipcc, gfx950   fe_run copies the records to the device and runs one lane per record
// Records hold raw register-form limbs (Fp<P>::v[N], no Montgomery conversion here), so the caller sets exact limb patterns,
// including the non-normalised lazy forms.  Record strides: FE_IN_WORDS(N) = 16 N words in, FE_OUT_WORDS(N) = 8 N words out.
//   field: 0 BN254 Fq, 1 BN254 Fr, 2 BLS12-381 Fq, 3 BLS12-381 Fr
//   op:    the FE_* numbers below (tests/test_field_edges.py mirrors them)
// A bucket-step record (FE_G1_STEP / FE_G2_STEP, fields 0 and 2): the base row (x, y) in memory form (2 F::LIMBS words) at word 0,
// the accumulator X, Y, ZZ, ZZZ in register form (F::REGS words each) at word 4 N, the negate flag at word 12 N.  FE_G1_STEP runs
// the device form xyzz_add_affine_mem only (it does not exist on the host); FE_G2_STEP runs xyzz_add_affine_mem on the device and
// xyzz_add_affine_relaxed2 (what it calls) on the host.
#include <cstdint>
#include <cstring>
#include "../../zksnake_amd/csrc/curve.hip.h"
#include "../../zksnake_amd/csrc/ntt_lazy.hip.h"

using namespace zkmi;

enum {
    FE_ADD = 0, FE_SUB, FE_REDUCE_FULL, FE_REDUCE_2P, FE_IS_ZERO, FE_IS_ZERO_LIMBS, FE_EQ,
    FE_MUL, FE_MUL2, FE_MUL4, FE_SQR, FE_INV,
    FE_SUB_LAZY, FE_SUB_K2, FE_SUB_K4, FE_SUB_K8, FE_SUB_TWICE_SEL4, FE_SUB_LAZY8, FE_NEG_LAZY, FE_NEG_LAZY_K4, FE_NEG_LAZY_K8,
    FE_ADD_NOSEL, FE_DBL_LAZY,
    FE_FROM_CANONICAL, FE_TO_CANONICAL,
    FE_FP2_MUL, FE_FP2_SQR, FE_FP2_INV, FE_FP2_MUL_REL4, FE_FP2_MUL_REL8, FE_FP2_SQR_REL4, FE_FP2_SQR_REL8,
    FE_LZ_SUB_18_29, FE_LZ_SUB_36_30, FE_LZ_NORM, FE_LZ_REDUCE8, FE_LZ_REDUCE2, FE_LZ_CANONICAL,
    FE_G1_STEP, FE_G2_STEP,
    FE_NUM_OPS
};

constexpr uint64_t FE_MAX_COUNT = 1ull << 20;

template <class P>
ZK_HD Fp<P> ld(const uint32_t* in, int k) {
    Fp<P> r;
    for (int i = 0; i < P::N; ++i) r.v[i] = in[k * P::N + i];
    return r;
}
template <class P>
ZK_HD void st(uint32_t* out, int k, const Fp<P>& a) {
    for (int i = 0; i < P::N; ++i) out[k * P::N + i] = a.v[i];
}
template <class P>
ZK_HD Fp2<P> ld2(const uint32_t* in, int k) {
    return {ld<P>(in, 2 * k), ld<P>(in, 2 * k + 1)};
}
template <class P>
ZK_HD void st2(uint32_t* out, int k, const Fp2<P>& a) {
    st<P>(out, 2 * k, a.c0);
    st<P>(out, 2 * k + 1, a.c1);
}

// the field ops: both builds; returns 0, or 1 for an op this field does not have
template <class P>
ZK_HD int fe_field_op(int op, const uint32_t* in, uint32_t* out) {
    const Fp<P> a = ld<P>(in, 0), b = ld<P>(in, 1);
    switch (op) {
    case FE_ADD: st<P>(out, 0, fp_add<P>(a, b)); return 0;
    case FE_SUB: st<P>(out, 0, fp_sub<P>(a, b)); return 0;
    case FE_REDUCE_FULL: st<P>(out, 0, fp_reduce_full<P>(a)); return 0;
    case FE_REDUCE_2P: st<P>(out, 0, fp_reduce_2p<P>(a)); return 0;
    case FE_IS_ZERO: out[0] = fp_is_zero<P>(a) ? 1u : 0u; return 0;
    case FE_IS_ZERO_LIMBS: out[0] = fp_is_zero_limbs<P>(a) ? 1u : 0u; return 0;
    case FE_EQ: out[0] = fp_eq<P>(a, b) ? 1u : 0u; return 0;
    case FE_MUL: st<P>(out, 0, fp_mul<P>(a, b)); return 0;
    case FE_MUL2: st<P>(out, 0, fp_mul2<P>(a, b, ld<P>(in, 2), ld<P>(in, 3))); return 0;
    case FE_MUL4:
        if constexpr (P::N <= 9) {
            st<P>(out, 0, fp_mul4<P>(a, b, ld<P>(in, 2), ld<P>(in, 3), ld<P>(in, 4), ld<P>(in, 5), ld<P>(in, 6), ld<P>(in, 7)));
            return 0;
        }
        return 1;
    case FE_SQR: st<P>(out, 0, fp_sqr<P>(a)); return 0;
    case FE_INV: st<P>(out, 0, fp_inv<P>(a)); return 0;
    case FE_SUB_LAZY: st<P>(out, 0, fp_sub_lazy<P>(a, b)); return 0;
    case FE_SUB_K2: st<P>(out, 0, fp_sub_k<P, 2>(a, b)); return 0;
    case FE_SUB_K4: st<P>(out, 0, fp_sub_k<P, 4>(a, b)); return 0;
    case FE_SUB_K8: st<P>(out, 0, fp_sub_k<P, 8>(a, b)); return 0;
    case FE_SUB_TWICE_SEL4: st<P>(out, 0, fp_sub_twice_sel4<P>(a, b)); return 0;
    case FE_SUB_LAZY8: st<P>(out, 0, fp_sub_lazy8<P>(a, b)); return 0;
    case FE_NEG_LAZY: st<P>(out, 0, fp_neg_lazy<P>(a)); return 0;
    case FE_NEG_LAZY_K4: st<P>(out, 0, fp_neg_lazy_k<P, 4>(a)); return 0;
    case FE_NEG_LAZY_K8: st<P>(out, 0, fp_neg_lazy_k<P, 8>(a)); return 0;
    case FE_ADD_NOSEL: st<P>(out, 0, fp_add_nosel<P>(a, b)); return 0;
    case FE_DBL_LAZY: st<P>(out, 0, fp_dbl_lazy<P>(a)); return 0;
    case FE_FROM_CANONICAL: st<P>(out, 0, fp_from_canonical<P>(in)); return 0;   // W words in
    case FE_TO_CANONICAL: fp_to_canonical<P>(out, a); return 0;                 // W words out
    case FE_FP2_MUL: st2<P>(out, 0, fp2_mul<P>(ld2<P>(in, 0), ld2<P>(in, 1))); return 0;
    case FE_FP2_SQR: st2<P>(out, 0, fp2_sqr<P>(ld2<P>(in, 0))); return 0;
    case FE_FP2_INV: st2<P>(out, 0, fp2_inv<P>(ld2<P>(in, 0))); return 0;
    case FE_FP2_MUL_REL4: st2<P>(out, 0, fp2_mul_relaxed<P, 4>(ld2<P>(in, 0), ld2<P>(in, 1))); return 0;
    case FE_FP2_MUL_REL8: st2<P>(out, 0, fp2_mul_relaxed<P, 8>(ld2<P>(in, 0), ld2<P>(in, 1))); return 0;
    case FE_FP2_SQR_REL4: st2<P>(out, 0, fp2_sqr_relaxed<P, 4>(ld2<P>(in, 0))); return 0;
    case FE_FP2_SQR_REL8: st2<P>(out, 0, fp2_sqr_relaxed<P, 8>(ld2<P>(in, 0))); return 0;
    case FE_LZ_SUB_18_29: st<P>(out, 0, lz_sub<P, 18, 29>(a, b)); return 0;
    case FE_LZ_SUB_36_30: st<P>(out, 0, lz_sub<P, 36, 30>(a, b)); return 0;
    case FE_LZ_NORM: st<P>(out, 0, lz_norm<P>(a)); return 0;
    case FE_LZ_REDUCE8: st<P>(out, 0, lz_reduce<P, 8>(a)); return 0;
    case FE_LZ_REDUCE2: st<P>(out, 0, lz_reduce<P, 2>(a)); return 0;
    case FE_LZ_CANONICAL: st<P>(out, 0, lz_canonical<P>(a)); return 0;
    default: return 1;
    }
}

// the record layout of a bucket step
template <class F>
struct StepRec {
    static constexpr int N = F::Params::N;
    static constexpr int ACC = 4 * N;    // word offset of the accumulator
    static constexpr int NEG = 12 * N;   // word offset of the negate flag
    static_assert(2 * F::LIMBS <= ACC && ACC + 4 * F::REGS <= NEG, "record layout");
};
template <class F>
ZK_HD XYZZ<F> step_load_acc(const uint32_t* in) {
    XYZZ<F> acc;
    memcpy(&acc, in + StepRec<F>::ACC, sizeof(acc));
    return acc;
}

static bool fe_field_ok(int field) { return field >= 0 && field <= 3; }
static int fe_words_n(int field) { return field == 2 ? BlsFqParams::N : BnFqParams::N; }   // N is 9 for the other three

static bool fe_op_ok(int field, int op) {
    if (op < 0 || op >= FE_NUM_OPS) return false;
    if (op == FE_MUL4 && field == 2) return false;                                  // fp_mul4 needs N <= 9
    if (op >= FE_LZ_SUB_18_29 && op <= FE_LZ_CANONICAL && field != 1 && field != 3) return false;   // scalar fields only
    if ((op == FE_G1_STEP || op == FE_G2_STEP) && field != 0 && field != 2) return false;         // base fields only
    return true;
}

#if !defined(__HIPCC__)

// ---- host build ------------------------------------------------------------------------------------------------------
template <class P>
static int host_run(int op, uint64_t count, const uint32_t* in, uint32_t* out) {
    const size_t iw = 16 * P::N, ow = 8 * P::N;
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t* r = in + i * iw;
        uint32_t* o = out + i * ow;
        if (op == FE_G1_STEP) return 2;   // device form only
        if (op == FE_G2_STEP) {
            typedef Fp2Ops<P> F;
            XYZZ<F> acc = step_load_acc<F>(r);
            const Affine<F> q = {F::load(r), F::load(r + F::LIMBS)};
            xyzz_add_affine_relaxed2<F>(acc, q, r[StepRec<F>::NEG] != 0);
            memcpy(o, &acc, sizeof(acc));
            continue;
        }
        if (fe_field_op<P>(op, r, o)) return 2;
    }
    return 0;
}

extern "C" int fe_run(int field, int op, uint64_t count, const uint32_t* in, uint32_t* out) {
    if (!fe_field_ok(field) || !fe_op_ok(field, op) || count > FE_MAX_COUNT || (count && (!in || !out))) return 1;
    switch (field) {
    case 0: return host_run<BnFqParams>(op, count, in, out);
    case 1: return host_run<BnFrParams>(op, count, in, out);
    case 2: return host_run<BlsFqParams>(op, count, in, out);
    default: return host_run<BlsFrParams>(op, count, in, out);
    }
}

#else

// ---- device build: one lane per record -------------------------------------------------------------------------------
template <class P>
__global__ void fe_field_kernel(int op, uint64_t count, const uint32_t* in, uint32_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    fe_field_op<P>(op, in + i * 16 * P::N, out + i * 8 * P::N);
}

template <class F>
__global__ void fe_step_kernel(uint64_t count, const uint32_t* in, uint32_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    constexpr int N = F::Params::N;
    const uint32_t* r = in + i * 16 * N;
    XYZZ<F> acc = step_load_acc<F>(r);
    xyzz_add_affine_mem<F>(acc, r, r[StepRec<F>::NEG] != 0);
    memcpy(out + i * 8 * N, &acc, sizeof(acc));
}

#define FE_HIP(expr)                                  \
    do {                                              \
        if ((expr) != hipSuccess) { rc = 3; goto done; } \
    } while (0)

extern "C" int fe_run(int field, int op, uint64_t count, const uint32_t* in, uint32_t* out) {
    if (!fe_field_ok(field) || !fe_op_ok(field, op) || count > FE_MAX_COUNT || (count && (!in || !out))) return 1;
    if (count == 0) return 0;
    const int n = fe_words_n(field);
    const size_t in_bytes = count * 16 * n * 4, out_bytes = count * 8 * n * 4;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    int rc = 0;
    const dim3 grid((unsigned)((count + 63) / 64)), block(64);
    FE_HIP(hipMalloc(&d_in, in_bytes));
    FE_HIP(hipMalloc(&d_out, out_bytes));
    FE_HIP(hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice));
    FE_HIP(hipMemset(d_out, 0, out_bytes));
    if (op == FE_G1_STEP || op == FE_G2_STEP) {
        if (field == 0 && op == FE_G1_STEP) hipLaunchKernelGGL(fe_step_kernel<FpOps<BnFqParams>>, grid, block, 0, 0, count, d_in, d_out);
        if (field == 2 && op == FE_G1_STEP) hipLaunchKernelGGL(fe_step_kernel<FpOps<BlsFqParams>>, grid, block, 0, 0, count, d_in, d_out);
        if (field == 0 && op == FE_G2_STEP) hipLaunchKernelGGL(fe_step_kernel<Fp2Ops<BnFqParams>>, grid, block, 0, 0, count, d_in, d_out);
        if (field == 2 && op == FE_G2_STEP) hipLaunchKernelGGL(fe_step_kernel<Fp2Ops<BlsFqParams>>, grid, block, 0, 0, count, d_in, d_out);
    } else {
        switch (field) {
        case 0: hipLaunchKernelGGL(fe_field_kernel<BnFqParams>, grid, block, 0, 0, op, count, d_in, d_out); break;
        case 1: hipLaunchKernelGGL(fe_field_kernel<BnFrParams>, grid, block, 0, 0, op, count, d_in, d_out); break;
        case 2: hipLaunchKernelGGL(fe_field_kernel<BlsFqParams>, grid, block, 0, 0, op, count, d_in, d_out); break;
        default: hipLaunchKernelGGL(fe_field_kernel<BlsFrParams>, grid, block, 0, 0, op, count, d_in, d_out); break;
        }
    }
    FE_HIP(hipGetLastError());
    FE_HIP(hipDeviceSynchronize());
    FE_HIP(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
done:
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    return rc;
}

#endif
