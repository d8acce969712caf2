// mlpcs_args_check.cpp -- the host side of csrc/mlpcs.hip (argument rules, overlap checks, the conversion of the point) as a
// stand-alone host program for a sanitizer run; no device code is built and no kernel can be launched.  Built and run by the
// recipe in the header of pcs_args_check.cpp (tests/helpers.py run_host_program).
// Every call in the first part must come back with ZK_ERR_ARG before anything is written; the last ones pass the checks, convert
// their scalars on the host and then fail in the launch or the copy (ZK_ERR_HIP: no device, and the empty image holds no kernel).
#include <cstdio>
#include <cstdlib>
#include "../../zksnake_amd/csrc/mlpcs.hip"

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
    const int log_n = 3, n = 8;
    // f (n) | q (n - 1) | work (2 elements at this size); never dereferenced by a call that is refused
    static uint64_t mem[4 * (n + n + 2)];
    uint64_t *f = mem, *q = mem + 4 * n, *w = mem + 8 * n;
    uint64_t point[ZK_MLPCS_MAX_LOG * 4], eval[4] = {0};
    for (int i = 0; i < ZK_MLPCS_MAX_LOG * 4; ++i) point[i] = ~0ull - i;
    static_assert(ZK_MLPCS_MAX_LOG == 24, "the cap this program walks up to");
    for (int curve = 0; curve < 2; ++curve) {
        // a null pointer
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, nullptr, point, q, eval, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, f, nullptr, q, eval, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, f, point, nullptr, eval, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, f, point, q, nullptr, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, 0, nullptr, nullptr, nullptr, eval, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, 0, f, nullptr, nullptr, nullptr, nullptr, nullptr), ZK_ERR_ARG);
        // log_n out of range
        EXPECT(zk_mlpcs_quotients_dev(curve, -1, f, point, q, eval, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, ZK_MLPCS_MAX_LOG + 1, f, point, q, eval, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, 63, f, point, q, eval, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, 64, f, point, q, eval, nullptr, nullptr), ZK_ERR_ARG);
        // d_q overlaps d_f: the same start, its last element over the first of f, its first over the last of f
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, f, point, f, eval, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, q, point, q - 4 * (n - 2), eval, w, nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, f, point, f + 4 * (n - 1), eval, w, nullptr), ZK_ERR_ARG);
        // d_work (2 elements here) overlaps d_f or d_q
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, f, point, q, eval, f, nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, f, point, q, eval, f + 4 * (n - 1), nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, f, point, q, eval, f + 4, nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, f, point, q, eval, q, nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, f, point, q, eval, q + 4 * (n - 2), nullptr), ZK_ERR_ARG);
        EXPECT(zk_mlpcs_quotients_dev(curve, 0, f, nullptr, nullptr, eval, f, nullptr), ZK_ERR_ARG);
        // past the checks: the point is converted on the host, then the launch (or, without a variable, the copy) fails
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, f, point, q, eval, w, nullptr), ZK_ERR_HIP);
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, f, point, q, eval, nullptr, nullptr), ZK_ERR_HIP);
        EXPECT(zk_mlpcs_quotients_dev(curve, log_n, f, point, q, eval, q + 4 * (n - 1), nullptr), ZK_ERR_HIP);   // adjacent, not overlapping
        EXPECT(zk_mlpcs_quotients_dev(curve, 0, f, nullptr, nullptr, eval, nullptr, nullptr), ZK_ERR_HIP);
        EXPECT(zk_mlpcs_quotients_dev(curve, 1, f, point, q, eval, w, nullptr), ZK_ERR_HIP);
    }
    EXPECT(zk_mlpcs_quotients_dev(2, log_n, f, point, q, eval, w, nullptr), ZK_ERR_ARG);
    EXPECT(zk_mlpcs_quotients_dev(-1, 0, f, nullptr, nullptr, eval, nullptr, nullptr), ZK_ERR_ARG);
    for (unsigned i = 0; i < sizeof(mem) / sizeof(mem[0]); ++i)
        if (mem[i]) { printf("  FAILED: a refused call wrote to its buffers\n"); ++g_errors; break; }
    for (int i = 0; i < 4; ++i)
        if (eval[i]) { printf("  FAILED: a refused call wrote to eval_out\n"); ++g_errors; break; }
    if (g_errors) printf("mlpcs_args_check: %d FAILED\n", g_errors);
    else printf("mlpcs_args_check: all ok\n");
    return g_errors ? 1 : 0;
}
