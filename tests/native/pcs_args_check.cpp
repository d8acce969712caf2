// pcs_args_check.cpp -- the host side of csrc/pcs.hip (argument rules, overlap checks, the conversion of the challenges and the
// squarings of the opening point) as a stand-alone host program for a sanitizer run; no device code is built and no kernel can be
// launched:
//   hipcc -x hip --offload-host-only --offload-arch=gfx950 -O1 -g -std=c++17 -mbmi2 -madx -DZK_NOINLINE_MUL
//         -fsanitize=address,undefined -fno-sanitize-recover=undefined -c tests/native/pcs_args_check.cpp -o pcs_args_check.o
// The object refers to its device image (__hip_fatbin_<hash>, see `nm -u`): link it with an EMPTY offload bundle of that
// name, built the way tools/sanitize_cpu.sh builds its fatbin_stub.cpp, and with -fsanitize=address,undefined; then run it.
// Every call below must come back with ZK_ERR_ARG before anything is written; the last ones pass the checks, convert their
// scalars on the host and then fail in the launch (ZK_ERR_HIP: the empty device image holds no kernel).
#include <cstdio>
#include <cstdlib>
#include "../../zksnake_amd/csrc/pcs.hip"

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
    static uint64_t mem[4 * n * 4];   // c | s | scal_L | scal_R: never dereferenced by a call that is refused
    uint64_t *c = mem, *s = mem + 4 * n, *l = mem + 8 * n, *r = mem + 12 * n;
    uint64_t u[4] = {5, 0, 0, 0}, ui[4] = {~0ull, ~0ull, ~0ull, ~0ull}, z[4] = {~0ull, 7, ~0ull, ~0ull}, evals[8] = {0}, one[4] = {1, 0, 0, 0};
    uint64_t us[ZK_PCS_MAX_LOG * 4];
    for (int i = 0; i < ZK_PCS_MAX_LOG * 4; ++i) us[i] = ~0ull - i;
    for (int curve = 0; curve < 2; ++curve) {
        // a null pointer
        EXPECT(zk_pcs_round_dev(curve, log_n, 1, nullptr, s, u, ui, z, l, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, 1, c, nullptr, u, ui, z, l, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, 1, c, s, u, ui, nullptr, l, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, 1, c, s, u, ui, z, nullptr, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, 1, c, s, u, ui, z, l, nullptr, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, 1, c, s, u, ui, z, l, r, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, 0, c, s, nullptr, nullptr, nullptr, l, r, evals, nullptr), ZK_ERR_ARG);
        // a size out of range
        EXPECT(zk_pcs_round_dev(curve, log_n, -1, c, s, nullptr, nullptr, z, l, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, log_n + 1, c, s, u, ui, z, l, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, -1, 0, c, s, nullptr, nullptr, z, l, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, ZK_PCS_MAX_LOG + 1, 1, c, s, u, ui, z, l, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, 63, 1, c, s, u, ui, z, l, r, evals, nullptr), ZK_ERR_ARG);
        // a challenge present at k = 0, or missing later
        EXPECT(zk_pcs_round_dev(curve, log_n, 0, c, s, u, ui, z, l, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, 0, c, s, u, nullptr, z, l, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, 0, c, s, nullptr, ui, z, l, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, 1, c, s, nullptr, ui, z, l, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, 1, c, s, u, nullptr, z, l, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, log_n, c, s, u, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, 0, 0, c, s, u, ui, nullptr, nullptr, nullptr, nullptr, nullptr), ZK_ERR_ARG);
        // two buffers that overlap
        EXPECT(zk_pcs_round_dev(curve, log_n, 1, c, c + 4 * (n - 1), u, ui, z, l, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, 1, c, s, u, ui, z, s, r, evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, 1, c, s, u, ui, z, l, l + 4 * (n - 1), evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, 0, c, s, nullptr, nullptr, z, l, c + 4 * (n - 1), evals, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_round_dev(curve, log_n, log_n, c, c, u, ui, nullptr, nullptr, nullptr, nullptr, nullptr), ZK_ERR_ARG);
        // the verifier's scalars
        EXPECT(zk_pcs_verify_scalars_dev(curve, log_n, us, nullptr, l, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_verify_scalars_dev(curve, log_n, us, one, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_verify_scalars_dev(curve, log_n, nullptr, one, l, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_verify_scalars_dev(curve, -1, us, one, l, nullptr), ZK_ERR_ARG);
        EXPECT(zk_pcs_verify_scalars_dev(curve, ZK_PCS_MAX_LOG + 1, us, one, l, nullptr), ZK_ERR_ARG);
        // past the checks: the conversions run on the host (21 challenges of 256 set bits, 18 squarings), then the launch fails
        EXPECT(zk_pcs_verify_scalars_dev(curve, ZK_PCS_MAX_LOG, us, ui, l, nullptr), ZK_ERR_HIP);
        EXPECT(zk_pcs_verify_scalars_dev(curve, 0, nullptr, one, l, nullptr), ZK_ERR_HIP);
        EXPECT(zk_pcs_round_dev(curve, log_n, 0, c, s, nullptr, nullptr, z, l, r, evals, nullptr), ZK_ERR_HIP);
        EXPECT(zk_pcs_round_dev(curve, log_n, 1, c, s, u, ui, z, l, r, evals, nullptr), ZK_ERR_HIP);
        EXPECT(zk_pcs_round_dev(curve, log_n, log_n, c, s, ui, u, nullptr, nullptr, nullptr, nullptr, nullptr), ZK_ERR_HIP);
        EXPECT(zk_pcs_round_dev(curve, 0, 0, c, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), ZK_ERR_HIP);
    }
    EXPECT(zk_pcs_round_dev(2, log_n, 0, c, s, nullptr, nullptr, z, l, r, evals, nullptr), ZK_ERR_ARG);
    EXPECT(zk_pcs_verify_scalars_dev(-1, 0, nullptr, one, l, nullptr), ZK_ERR_ARG);
    for (unsigned i = 0; i < sizeof(mem) / sizeof(mem[0]); ++i)
        if (mem[i]) { printf("  FAILED: a refused call wrote to its buffers\n"); ++g_errors; break; }
    for (int i = 0; i < 8; ++i)
        if (evals[i]) { printf("  FAILED: a refused call wrote to evals\n"); ++g_errors; break; }
    if (g_errors) printf("pcs_args_check: %d FAILED\n", g_errors);
    else printf("pcs_args_check: all ok\n");
    return g_errors ? 1 : 0;
}
