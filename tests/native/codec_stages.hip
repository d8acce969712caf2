// Stage harness for the point codec (csrc/codec.hip.h): its pieces called directly, one record per call.  One source, two
// builds (tests/test_codec_stages.py):
//   g++ -x c++      cs_run loops over the records on the CPU
//   hipcc, gfx950   cs_run copies the records to the device and runs one lane per record, 128 lanes per workgroup as
//                   points_decode_kernel / points_encode_kernel do
// Every record is CS_IN_WORDS words in and CS_OUT_WORDS words out; the output records arrive filled by the caller and only the
// words named below are written.  Field elements cross as canonical 32-bit words (W = 8 or 12 per element).
//   sel  for the field ops: 0 BN254 Fq, 1 BLS12-381 Fq;  for CS_DECODE / CS_ENCODE: 0 BN254 G1, 1 BN254 G2, 2 BLS12-381 G1,
//        3 BLS12-381 G2
//   CS_POW          in: a (W), the exponent (W words), nwords <= W at word 2 W          out: a^e (W)
//   CS_SQRT         in: a (W)                                                           out: found, the root (W)
//   CS_FP2_SQRT     in: c0, c1                                                          out: found, the root c0, c1
//   CS_LARGER       in: y (W)                                                           out: coord_is_larger
//   CS_LARGER_FP2   in: c0, c1                                                          out: coord_is_larger
//   CS_LT_MOD       in: W raw words                                                     out: canonical_lt_mod
//   CS_DECODE       in: the encoding, one byte per word                                 out: the status, the point (2 F::LIMBS)
//   CS_ENCODE       in: the point (2 F::LIMBS)                                          out: the status, one byte per word (the
//                                                                                            low byte; point_encode is handed the
//                                                                                            caller's low bytes to write over)
// cs_run returns 0, 1 for a refused argument, 3 for a HIP error.
#include <cstdint>
#include "../../zksnake_amd/csrc/codec.hip.h"

using namespace zkmi;

enum { CS_POW = 0, CS_SQRT, CS_FP2_SQRT, CS_LARGER, CS_LARGER_FP2, CS_LT_MOD, CS_DECODE, CS_ENCODE, CS_NUM_OPS };

constexpr int CS_IN_WORDS = 128, CS_OUT_WORDS = 128;
constexpr uint64_t CS_MAX_COUNT = 1ull << 16;

template <class P>
ZK_HD void cs_field_op(int op, const uint32_t* in, uint32_t* out) {
    constexpr int W = P::W;
    static_assert(2 * W + 1 <= CS_IN_WORDS && 1 + 2 * W <= CS_OUT_WORDS, "record layout");
    const Fp<P> a = fp_from_canonical<P>(in);
    const Fp2<P> a2 = {a, fp_from_canonical<P>(in + W)};
    switch (op) {
    case CS_POW: {
        const int nwords = in[2 * W] <= (uint32_t)W ? (int)in[2 * W] : W;
        fp_to_canonical<P>(out, fp_pow<P>(a, in + W, nwords));
        return;
    }
    case CS_SQRT: {
        Fp<P> s = fp_zero<P>();
        out[0] = fp_sqrt<P>(a, &s) ? 1u : 0u;
        fp_to_canonical<P>(out + 1, s);
        return;
    }
    case CS_FP2_SQRT: {
        Fp2<P> s = fp2_zero<P>();
        out[0] = fp2_sqrt<P>(a2, &s) ? 1u : 0u;
        fp_to_canonical<P>(out + 1, s.c0);
        fp_to_canonical<P>(out + 1 + W, s.c1);
        return;
    }
    case CS_LARGER: out[0] = coord_is_larger<P>(a) ? 1u : 0u; return;
    case CS_LARGER_FP2: out[0] = coord_is_larger<P>(a2) ? 1u : 0u; return;
    case CS_LT_MOD: out[0] = canonical_lt_mod<P>(in) ? 1u : 0u; return;
    }
}

template <class G>
ZK_HD void cs_point_op(int op, const uint32_t* in, uint32_t* out) {
    constexpr int TOTAL = CodecLayout<G>::TOTAL, ROW = 2 * G::F::LIMBS;
    static_assert(TOTAL <= CS_IN_WORDS && 1 + TOTAL <= CS_OUT_WORDS && 1 + ROW <= CS_OUT_WORDS, "record layout");
    uint8_t bytes[TOTAL];
    if (op == CS_DECODE) {
        for (int i = 0; i < TOTAL; ++i) bytes[i] = (uint8_t)in[i];
        out[0] = (uint32_t)point_decode<G>(bytes, out + 1);
    } else {
        for (int i = 0; i < TOTAL; ++i) bytes[i] = (uint8_t)out[1 + i];   // the caller's fill, so that a refusal that writes shows
        out[0] = (uint32_t)point_encode<G>(in, bytes);
        for (int i = 0; i < TOTAL; ++i) out[1 + i] = (out[1 + i] & ~0xFFu) | bytes[i];
    }
}

static bool cs_args_ok(int op, int sel, uint64_t count, const uint32_t* in, uint32_t* out) {
    if (op < 0 || op >= CS_NUM_OPS || count > CS_MAX_COUNT || (count && (!in || !out))) return false;
    return sel >= 0 && sel <= (op >= CS_DECODE ? 3 : 1);
}

#if !defined(__HIPCC__)

// ---- host build ------------------------------------------------------------------------------------------------------
extern "C" int cs_run(int op, int sel, uint64_t count, const uint32_t* in, uint32_t* out) {
    if (!cs_args_ok(op, sel, count, in, out)) return 1;
    for (uint64_t i = 0; i < count; ++i) {
        const uint32_t* r = in + i * CS_IN_WORDS;
        uint32_t* o = out + i * CS_OUT_WORDS;
        if (op < CS_DECODE) {
            if (sel == 0) cs_field_op<BnFqParams>(op, r, o);
            else cs_field_op<BlsFqParams>(op, r, o);
        } else if (sel == 0) cs_point_op<Bn254G1>(op, r, o);
        else if (sel == 1) cs_point_op<Bn254G2>(op, r, o);
        else if (sel == 2) cs_point_op<Bls381G1>(op, r, o);
        else cs_point_op<Bls381G2>(op, r, o);
    }
    return 0;
}

#else

// ---- device build: one lane per record -------------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(128) void cs_field_kernel(int op, uint64_t count, const uint32_t* in, uint32_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    cs_field_op<P>(op, in + i * CS_IN_WORDS, out + i * CS_OUT_WORDS);
}

template <class G>
__global__ __launch_bounds__(128) void cs_point_kernel(int op, uint64_t count, const uint32_t* in, uint32_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    cs_point_op<G>(op, in + i * CS_IN_WORDS, out + i * CS_OUT_WORDS);
}

#define CS_HIP(expr)                                  \
    do {                                              \
        if ((expr) != hipSuccess) { rc = 3; goto done; } \
    } while (0)

extern "C" int cs_run(int op, int sel, uint64_t count, const uint32_t* in, uint32_t* out) {
    if (!cs_args_ok(op, sel, count, in, out)) return 1;
    if (count == 0) return 0;
    const size_t in_bytes = count * CS_IN_WORDS * 4, out_bytes = count * CS_OUT_WORDS * 4;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    int rc = 0;
    const dim3 grid((unsigned)((count + 127) / 128)), block(128);
    CS_HIP(hipMalloc(&d_in, in_bytes));
    CS_HIP(hipMalloc(&d_out, out_bytes));
    CS_HIP(hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice));
    CS_HIP(hipMemcpy(d_out, out, out_bytes, hipMemcpyHostToDevice));
    if (op < CS_DECODE) {
        if (sel == 0) hipLaunchKernelGGL(cs_field_kernel<BnFqParams>, grid, block, 0, 0, op, count, d_in, d_out);
        else hipLaunchKernelGGL(cs_field_kernel<BlsFqParams>, grid, block, 0, 0, op, count, d_in, d_out);
    } else if (sel == 0) hipLaunchKernelGGL(cs_point_kernel<Bn254G1>, grid, block, 0, 0, op, count, d_in, d_out);
    else if (sel == 1) hipLaunchKernelGGL(cs_point_kernel<Bn254G2>, grid, block, 0, 0, op, count, d_in, d_out);
    else if (sel == 2) hipLaunchKernelGGL(cs_point_kernel<Bls381G1>, grid, block, 0, 0, op, count, d_in, d_out);
    else hipLaunchKernelGGL(cs_point_kernel<Bls381G2>, grid, block, 0, 0, op, count, d_in, d_out);
    CS_HIP(hipGetLastError());
    CS_HIP(hipDeviceSynchronize());
    CS_HIP(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
done:
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    return rc;
}

#endif
