// rangeproof_args_check.cpp -- the host side of csrc/rangeproof.hip (size and pointer rules, overlap checks, the squarings and
// the conversion of the challenges) as a stand-alone host program for a sanitizer run; no device code is built and no kernel
// can be launched.  Built and linked like ipa_args_check.cpp beside it (host-only compile, an EMPTY offload bundle for the
// __hip_fatbin_<hash> symbol the object refers to, -fsanitize=address,undefined).
// Every refused call must come back with ZK_ERR_ARG before anything is written; the last ones pass the checks, build their
// kernel arguments on the host and then fail in the launch (ZK_ERR_HIP: the empty device image holds no kernel).
#include <cstdio>
#include <cstdlib>
#include "../../zksnake_amd/csrc/rangeproof.hip"

namespace zkmi {
int dev_alloc_cached(void** p, size_t bytes) { *p = malloc(bytes ? bytes : 1); return *p ? ZK_OK : ZK_ERR_HIP; }
void dev_free_cached(void* p) { free(p); }
}  // namespace zkmi

static int g_errors = 0;
#define EXPECT(call, want)                                                                       \
    do {                                                                                         \
        int got_ = (call);                                                                       \
        if (got_ != (want)) { printf("  FAILED line %d: %s = %d\n", __LINE__, #call, got_); ++g_errors; } \
    } while (0)

int main() {
    const int lb = 2, ln = 4, size = 16, m = 4;
    static uint64_t mem[(2 * size + 2 * size + size) * 4 + 2 * m];   // s (2N) | out (2N) | weights (N) | values: never dereferenced
    uint64_t *s = mem, *out = mem + 8 * size, *w = mem + 16 * size, *v = mem + 20 * size;
    uint64_t y[4] = {5, 0, 0, 0}, big[4] = {~0ull, ~0ull, ~0ull, ~0ull}, one[4] = {1, 0, 0, 0}, t[12] = {0};
    uint64_t us[ZK_IPA_MAX_LOG * 4];
    for (int i = 0; i < ZK_IPA_MAX_LOG * 4; ++i) us[i] = ~0ull - i;
    for (int curve = 0; curve < 2; ++curve) {
        EXPECT(zk_rp_bits_dev(curve, lb, ln, nullptr, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_bits_dev(curve, lb, ln, v, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_bits_dev(curve, -1, ln, v, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_bits_dev(curve, 8, 8, v, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_bits_dev(curve, 3, 2, v, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_bits_dev(curve, lb, ZK_IPA_MAX_LOG + 1, v, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_bits_dev(curve, lb, 63, v, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_bits_dev(curve, lb, ln, out + 4, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_poly_dev(curve, lb, ln, nullptr, s, y, y, t, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_poly_dev(curve, lb, ln, v, nullptr, y, y, t, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_poly_dev(curve, lb, ln, v, s, nullptr, y, t, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_poly_dev(curve, lb, ln, v, s, y, nullptr, t, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_poly_dev(curve, lb, ln, v, s, y, y, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_poly_dev(curve, 8, 8, v, s, y, y, t, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_poly_dev(curve, 3, 2, v, s, y, y, t, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_eval_dev(curve, lb, ln, nullptr, s, y, y, y, y, out, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_eval_dev(curve, lb, ln, v, nullptr, y, y, y, y, out, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_eval_dev(curve, lb, ln, v, s, nullptr, y, y, y, out, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_eval_dev(curve, lb, ln, v, s, y, nullptr, y, y, out, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_eval_dev(curve, lb, ln, v, s, y, y, nullptr, y, out, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_eval_dev(curve, lb, ln, v, s, y, y, y, nullptr, out, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_eval_dev(curve, lb, ln, v, s, y, y, y, y, nullptr, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_eval_dev(curve, lb, ln, v, s, y, y, y, y, out, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_eval_dev(curve, lb, ZK_IPA_MAX_LOG + 1, v, s, y, y, y, y, out, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_eval_dev(curve, lb, ln, v, s, y, y, y, y, s + 4, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_eval_dev(curve, lb, ln, v, s, y, y, y, y, out, out + 4 * (2 * size - 1), nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_eval_dev(curve, lb, ln, v, s, y, y, y, y, out, s, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_eval_dev(curve, lb, ln, w, s, y, y, y, y, out, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_verify_scalars_dev(curve, lb, ln, nullptr, us, one, one, y, y, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_verify_scalars_dev(curve, lb, ln, us, nullptr, one, one, y, y, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_verify_scalars_dev(curve, lb, ln, us, us, nullptr, one, y, y, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_verify_scalars_dev(curve, lb, ln, us, us, one, nullptr, y, y, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_verify_scalars_dev(curve, lb, ln, us, us, one, one, nullptr, y, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_verify_scalars_dev(curve, lb, ln, us, us, one, one, y, nullptr, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_verify_scalars_dev(curve, lb, ln, us, us, one, one, y, y, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_rp_verify_scalars_dev(curve, -1, ln, us, us, one, one, y, y, out, nullptr), ZK_ERR_ARG);
        // past the checks: squarings and conversions run on the host (values of 256 set bits among them), then the launch fails
        EXPECT(zk_rp_bits_dev(curve, lb, ln, v, out, nullptr), ZK_ERR_HIP);
        EXPECT(zk_rp_poly_dev(curve, lb, ln, v, s, big, y, t, nullptr), ZK_ERR_HIP);
        EXPECT(zk_rp_eval_dev(curve, lb, ln, v, s, y, big, big, one, out, w, nullptr), ZK_ERR_HIP);
        EXPECT(zk_rp_verify_scalars_dev(curve, 7, ZK_IPA_MAX_LOG, us, us, big, big, big, y, out, nullptr), ZK_ERR_HIP);
        EXPECT(zk_rp_verify_scalars_dev(curve, 0, 0, nullptr, nullptr, one, one, y, y, out, nullptr), ZK_ERR_HIP);
    }
    EXPECT(zk_rp_bits_dev(2, lb, ln, v, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_rp_poly_dev(-1, lb, ln, v, s, y, y, t, nullptr), ZK_ERR_ARG);
    EXPECT(zk_rp_eval_dev(7, lb, ln, v, s, y, y, y, y, out, w, nullptr), ZK_ERR_ARG);
    EXPECT(zk_rp_verify_scalars_dev(2, lb, ln, us, us, one, one, y, y, out, nullptr), ZK_ERR_ARG);
    for (unsigned i = 0; i < sizeof(mem) / sizeof(mem[0]); ++i)
        if (mem[i]) { printf("  FAILED: a refused call wrote to its buffers\n"); ++g_errors; break; }
    for (int i = 0; i < 12; ++i)
        if (t[i]) { printf("  FAILED: a failing call wrote t_out\n"); ++g_errors; break; }
    if (g_errors) printf("rangeproof_args_check: %d FAILED\n", g_errors);
    else printf("rangeproof_args_check: all ok\n");
    return g_errors ? 1 : 0;
}
