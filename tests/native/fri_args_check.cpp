// fri_args_check.cpp -- the host side of csrc/fri.hip (argument rules, alignment and overlap checks) as a stand-alone host
// program for a sanitizer run; no device code is built and no kernel can be launched:
//   hipcc -x hip --offload-host-only --offload-arch=gfx950 -O1 -g -std=c++17 -mbmi2 -madx -DZK_NOINLINE_MUL
//         -fsanitize=address,undefined -fno-sanitize-recover=undefined -c tests/native/fri_args_check.cpp -o fri_args_check.o
// The object refers to its device image (__hip_fatbin_<hash>, see `nm -u`): link it with an EMPTY offload bundle of that
// name, built the way tools/sanitize_cpu.sh builds its fatbin_stub.cpp, and with -fsanitize=address,undefined; then run it.
// Every refused call must come back with ZK_ERR_ARG before anything is written; the calls that pass the checks fail in the
// launch (ZK_ERR_HIP: the empty device image holds no kernel), and the one that has nothing to launch returns ZK_OK.
// zk_ntt_dev lives in ntt.hip, which is not part of this program: the stand-in below counts its calls, and there must be none,
// because zk_fri_lde_dev's first launch fails before the transform is reached.
#include <cstdio>
#include <cstdlib>
#include "../../zksnake_amd/csrc/fri.hip"

static int g_ntt_calls = 0;
extern "C" int zk_ntt_dev(int, int, int, void*, void*) {
    ++g_ntt_calls;
    return ZK_ERR_HIP;
}

static int g_errors = 0;
#define EXPECT(call, want)                                                                       \
    do {                                                                                         \
        int got_ = (call);                                                                       \
        if (got_ != (want)) { printf("  FAILED line %d: %s = %d\n", __LINE__, #call, got_); ++g_errors; } \
    } while (0)

int main() {
    // log_n = 2, log_blowup = 1: 4 coefficients, 8 evaluations.  One block holds coeffs | work | out | a spare layer, 32 bytes
    // per element, so that overlaps can be asked for.
    alignas(64) static uint8_t mem[32 * 32];
    alignas(64) static uint64_t idx[4];
    alignas(64) static uint8_t rows_out[4 * 64];
    uint8_t *coeffs = mem, *work = mem + 4 * 32, *out = mem + 12 * 32, *spare = mem + 20 * 32;
    const uint64_t shift[4] = {5, 0, 0, 0}, c[4] = {3, 0, 0, 0}, w[4] = {7, 0, 0, 0};
    for (int curve = 0; curve < 2; ++curve) {
        // ---- zk_fri_lde_dev ----
        EXPECT(zk_fri_lde_dev(curve, -1, 1, 0, coeffs, shift, work, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_lde_dev(curve, 2, 0, 4, coeffs, shift, work, out, nullptr), ZK_ERR_ARG);          // no blowup
        EXPECT(zk_fri_lde_dev(curve, 2, -1, 4, coeffs, shift, work, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_lde_dev(curve, ZK_FRI_MAX_LOG, 1, 4, coeffs, shift, work, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_lde_dev(curve, 1, ZK_FRI_MAX_LOG, 2, coeffs, shift, work, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_lde_dev(curve, 0x7fffffff, 0x7fffffff, 4, coeffs, shift, work, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 5, coeffs, shift, work, out, nullptr), ZK_ERR_ARG);          // more than 2^log_n coefficients
        EXPECT(zk_fri_lde_dev(curve, 2, 1, ~0ull, coeffs, shift, work, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 4, nullptr, shift, work, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 4, coeffs, nullptr, work, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 4, coeffs, shift, nullptr, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 4, coeffs, shift, work, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 4, coeffs + 8, shift, work, out, nullptr), ZK_ERR_ARG);      // misaligned
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 4, coeffs, shift, work + 4, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 4, coeffs, shift, work, out + 1, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 4, coeffs, shift, coeffs, out, nullptr), ZK_ERR_ARG);        // work on the coefficients
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 4, coeffs, shift, work, coeffs + 3 * 32 + 16, nullptr), ZK_ERR_ARG);   // out begins in the last one
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 4, coeffs, shift, work, work, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 4, coeffs, shift, work, work + 7 * 32 + 16, nullptr), ZK_ERR_ARG);     // out begins in work's last element
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 4, coeffs, shift, out + 32, out, nullptr), ZK_ERR_ARG);
        // ---- zk_fri_fold_dev: a layer of 8 (work) into 4 (spare) ----
        EXPECT(zk_fri_fold_dev(curve, 0, work, c, w, spare, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_fold_dev(curve, -3, work, c, w, spare, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_fold_dev(curve, ZK_FRI_MAX_LOG + 1, work, c, w, spare, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_fold_dev(curve, 3, nullptr, c, w, spare, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_fold_dev(curve, 3, work, nullptr, w, spare, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_fold_dev(curve, 3, work, c, nullptr, spare, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_fold_dev(curve, 3, work, c, w, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_fold_dev(curve, 3, work + 8, c, w, spare, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_fold_dev(curve, 3, work, c, w, spare + 4, nullptr), ZK_ERR_ARG);
        EXPECT(zk_fri_fold_dev(curve, 3, work, c, w, work, nullptr), ZK_ERR_ARG);                       // in place
        EXPECT(zk_fri_fold_dev(curve, 3, work, c, w, work + 7 * 32 + 16, nullptr), ZK_ERR_ARG);         // begins in the layer's last element
        EXPECT(zk_fri_fold_dev(curve, 3, work, c, w, work - 4 * 32 + 16, nullptr), ZK_ERR_ARG);         // ends in the layer's first element
        // past the checks: the launch fails, and the transform is not reached
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 4, coeffs, shift, work, out, nullptr), ZK_ERR_HIP);
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 3, coeffs, shift, work, out, nullptr), ZK_ERR_HIP);
        EXPECT(zk_fri_lde_dev(curve, 2, 1, 0, nullptr, shift, work, out, nullptr), ZK_ERR_HIP);          // no coefficients to read
        EXPECT(zk_fri_lde_dev(curve, 0, 1, 1, coeffs, shift, work, work + 2 * 32, nullptr), ZK_ERR_HIP); // out begins where work ends
        EXPECT(zk_fri_fold_dev(curve, 3, work, c, w, spare, nullptr), ZK_ERR_HIP);
        EXPECT(zk_fri_fold_dev(curve, 3, work, c, w, work + 8 * 32, nullptr), ZK_ERR_HIP);               // begins where the layer ends
        EXPECT(zk_fri_fold_dev(curve, 1, work, c, w, spare, nullptr), ZK_ERR_HIP);
    }
    // an unknown curve
    EXPECT(zk_fri_lde_dev(2, 2, 1, 4, coeffs, shift, work, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_lde_dev(-1, 2, 1, 4, coeffs, shift, work, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_fold_dev(2, 3, work, c, w, spare, nullptr), ZK_ERR_ARG);
    // ---- zk_fri_rows_dev: 16 rows of 64 bytes (mem), 4 indices ----
    EXPECT(zk_fri_rows_dev(0, 64, mem, 4, idx, rows_out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev((1ull << 32) + 1, 64, mem, 4, idx, rows_out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev(~0ull, 64, mem, 4, idx, rows_out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev(16, 0, mem, 4, idx, rows_out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev(16, 24, mem, 4, idx, rows_out, nullptr), ZK_ERR_ARG);                        // no multiple of 16
    EXPECT(zk_fri_rows_dev(16, ZK_FRI_MAX_ROW_BYTES + 16, mem, 4, idx, rows_out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev(16, ~0ull & ~15ull, mem, 4, idx, rows_out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev(16, 64, mem, (1ull << 32) + 1, idx, rows_out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev(16, 64, nullptr, 4, idx, rows_out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev(16, 64, nullptr, 0, idx, rows_out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev(16, 64, mem, 4, nullptr, rows_out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev(16, 64, mem, 4, idx, nullptr, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev(16, 64, mem + 8, 4, idx, rows_out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev(16, 64, mem, 4, idx, rows_out + 8, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev(16, 64, mem, 4, (uint8_t*)idx + 4, rows_out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_fri_rows_dev(16, 64, mem, 4, idx, mem + 15 * 64 + 48, nullptr), ZK_ERR_ARG);              // out begins in the last row
    EXPECT(zk_fri_rows_dev(8, 64, mem + 4 * 64, 4, idx, mem + 16, nullptr), ZK_ERR_ARG);                // out ends in the first row
    EXPECT(zk_fri_rows_dev(4, 64, mem, 4, rows_out + 3 * 64 + 32, rows_out, nullptr), ZK_ERR_ARG);      // the indices lie in the last output row
    EXPECT(zk_fri_rows_dev(16, 64, mem, 0, idx, rows_out, nullptr), ZK_OK);                             // nothing to do
    EXPECT(zk_fri_rows_dev(16, 64, mem, 0, nullptr, nullptr, nullptr), ZK_OK);
    EXPECT(zk_fri_rows_dev(16, 64, mem, 4, idx, rows_out, nullptr), ZK_ERR_HIP);
    EXPECT(zk_fri_rows_dev(8, 64, mem, 4, idx, mem + 8 * 64, nullptr), ZK_ERR_HIP);                     // out begins where the rows end
    EXPECT(zk_fri_rows_dev(64, 16, mem, 4, idx, rows_out, nullptr), ZK_ERR_HIP);
    if (g_ntt_calls) { printf("  FAILED: the transform was called %d times\n", g_ntt_calls); ++g_errors; }
    for (unsigned i = 0; i < sizeof(mem); ++i)
        if (mem[i] || rows_out[i % sizeof(rows_out)] || idx[i % 4]) { printf("  FAILED: a call wrote to a buffer\n"); ++g_errors; break; }
    if (g_errors) printf("fri_args_check: %d FAILED\n", g_errors);
    else printf("fri_args_check: all ok\n");
    return g_errors ? 1 : 0;
}
