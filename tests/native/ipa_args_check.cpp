// ipa_args_check.cpp -- the host side of csrc/ipa.hip (argument rules, overlap checks, the challenges' conversion) as a
// stand-alone host program for a sanitizer run; no device code is built and no kernel can be launched:
//   hipcc -x hip --offload-host-only --offload-arch=gfx950 -O1 -g -std=c++17 -mbmi2 -madx -DZK_NOINLINE_MUL
//         -fsanitize=address,undefined -fno-sanitize-recover=undefined -c tests/native/ipa_args_check.cpp -o ipa_args_check.o
// The object refers to its device image (__hip_fatbin_<hash>, see `nm -u`): link it with an EMPTY offload bundle of that
// name, built the way tools/sanitize_cpu.sh builds its fatbin_stub.cpp, and with -fsanitize=address,undefined; then run it.
// Every call below must come back with ZK_ERR_ARG before anything is written; the last ones pass the checks, convert their
// challenges on the host and then fail in the launch (ZK_ERR_HIP: the empty device image holds no kernel).
#include <cstdio>
#include <cstdlib>
#include "../../zksnake_amd/csrc/ipa.hip"

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
    const int n = 8, log_n = 3;
    static uint64_t mem[8 * n * 4];   // a | b | s | s_inv | scal_L (2n) | scal_R (2n): never dereferenced by a call that is refused
    uint64_t *a = mem, *b = mem + 4 * n, *s = mem + 8 * n, *si = mem + 12 * n, *l = mem + 16 * n, *r = mem + 24 * n;
    uint64_t u[4] = {5, 0, 0, 0}, ui[4] = {~0ull, ~0ull, ~0ull, ~0ull}, cross[8] = {0}, one[4] = {1, 0, 0, 0};
    uint64_t us[ZK_IPA_MAX_LOG * 4];
    for (int i = 0; i < ZK_IPA_MAX_LOG * 4; ++i) us[i] = ~0ull - i;
    for (int curve = 0; curve < 2; ++curve) {
        EXPECT(zk_ipa_round_dev(curve, log_n, 1, nullptr, b, s, si, u, ui, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, 1, a, nullptr, s, si, u, ui, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, 1, a, b, nullptr, si, u, ui, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, 1, a, b, s, nullptr, u, ui, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, 1, a, b, s, si, u, ui, nullptr, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, 1, a, b, s, si, u, ui, l, nullptr, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, 1, a, b, s, si, u, ui, l, r, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, -1, a, b, s, si, nullptr, nullptr, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, log_n + 1, a, b, s, si, u, ui, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, -1, 0, a, b, s, si, nullptr, nullptr, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, ZK_IPA_MAX_LOG + 1, 1, a, b, s, si, u, ui, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, 63, 1, a, b, s, si, u, ui, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, 0, a, b, s, si, u, ui, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, 0, a, b, s, si, nullptr, ui, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, 1, a, b, s, si, nullptr, ui, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, log_n, a, b, s, si, u, nullptr, nullptr, nullptr, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, 1, a, a + 4 * (n - 1), s, si, u, ui, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, 1, a, b, s, s, u, ui, l, r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, 1, a, b, s, si, u, ui, l, l + 4 * (2 * n - 1), cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_round_dev(curve, log_n, 0, a, b, s, si, nullptr, nullptr, si + 4 * (n - 1), r, cross, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_verify_scalars_dev(curve, log_n, us, us, nullptr, one, l, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_verify_scalars_dev(curve, log_n, us, us, one, nullptr, l, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_verify_scalars_dev(curve, log_n, us, us, one, one, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_verify_scalars_dev(curve, log_n, nullptr, us, one, one, l, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_verify_scalars_dev(curve, log_n, us, nullptr, one, one, l, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_verify_scalars_dev(curve, -1, us, us, one, one, l, nullptr), ZK_ERR_ARG);
        EXPECT(zk_ipa_verify_scalars_dev(curve, ZK_IPA_MAX_LOG + 1, us, us, one, one, l, nullptr), ZK_ERR_ARG);
        // past the checks: the conversions run on the host (22 challenges of 256 set bits), then the launch fails
        EXPECT(zk_ipa_verify_scalars_dev(curve, ZK_IPA_MAX_LOG, us, us, ui, ui, l, nullptr), ZK_ERR_HIP);
        EXPECT(zk_ipa_round_dev(curve, log_n, 1, a, b, s, si, u, ui, l, r, cross, nullptr), ZK_ERR_HIP);
        EXPECT(zk_ipa_round_dev(curve, log_n, log_n, a, b, s, si, ui, u, nullptr, nullptr, nullptr, nullptr), ZK_ERR_HIP);
    }
    EXPECT(zk_ipa_round_dev(2, log_n, 0, a, b, s, si, nullptr, nullptr, l, r, cross, nullptr), ZK_ERR_ARG);
    EXPECT(zk_ipa_verify_scalars_dev(-1, 0, nullptr, nullptr, one, one, l, nullptr), ZK_ERR_ARG);
    for (unsigned i = 0; i < sizeof(mem) / sizeof(mem[0]); ++i)
        if (mem[i]) { printf("  FAILED: a refused call wrote to its buffers\n"); ++g_errors; break; }
    if (g_errors) printf("ipa_args_check: %d FAILED\n", g_errors);
    else printf("ipa_args_check: all ok\n");
    return g_errors ? 1 : 0;
}
