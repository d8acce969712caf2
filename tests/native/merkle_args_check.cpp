// merkle_args_check.cpp -- the host side of csrc/merkle.hip (argument rules, overlap checks, the layout arithmetic) as a
// stand-alone host program for a sanitizer run; no device code is built and no kernel can be launched:
//   hipcc -x hip --offload-host-only --offload-arch=gfx950 -O1 -g -std=c++17 -mbmi2 -madx -DZK_NOINLINE_MUL
//         -fsanitize=address,undefined -fno-sanitize-recover=undefined -c tests/native/merkle_args_check.cpp -o merkle_args_check.o
// The object refers to its device image (__hip_fatbin_<hash>, see `nm -u`): link it with an EMPTY offload bundle of that
// name, built the way tools/sanitize_cpu.sh builds its fatbin_stub.cpp, and with -fsanitize=address,undefined; then run it.
// Every refused call must come back with ZK_ERR_ARG before anything is written; the calls that pass the checks fail in the
// launch (ZK_ERR_HIP: the empty device image holds no kernel), and the ones that have nothing to launch return ZK_OK.
#include <cstdio>
#include <cstdlib>
#include "../../zksnake_amd/csrc/merkle.hip"

static int g_errors = 0;
#define EXPECT(call, want)                                                                       \
    do {                                                                                         \
        int got_ = (call);                                                                       \
        if (got_ != (want)) { printf("  FAILED line %d: %s = %d\n", __LINE__, #call, got_); ++g_errors; } \
    } while (0)

int main() {
    const uint64_t n = 5, big = (1ull << ZK_MERKLE_MAX_LOG) + 1;
    // rows (5 x 32) | offsets (6) | digests / tree (9 nodes for n = 5: 5 + 3 + 2 + 1 = 11, room for 16) | indices (4) | paths (4 x 3)
    alignas(64) static uint8_t rows[5 * 32], tree[16 * 64], paths[4 * 3 * 64];
    alignas(64) static uint64_t off[6], idx[4];
    // a size out of range
    EXPECT(zk_blake2b_rows_dev(0, rows, 32, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_rows_dev(big, rows, 32, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_rows_dev(~0ull, rows, 32, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_rows_dev(n, rows, 1ull << 32, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_rows_dev(n, rows, ~0ull, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_items_dev(0, rows, sizeof(rows), off, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_items_dev(big, rows, sizeof(rows), off, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_build_dev(0, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_build_dev(big, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_paths_dev(0, tree, 4, idx, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_paths_dev(big, tree, 4, idx, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_paths_dev(n, tree, (1ull << 32) + 1, idx, paths, nullptr), ZK_ERR_ARG);
    // a null pointer
    EXPECT(zk_blake2b_rows_dev(n, nullptr, 32, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_rows_dev(n, rows, 32, nullptr, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_rows_dev(n, nullptr, 0, nullptr, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_items_dev(n, nullptr, sizeof(rows), off, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_items_dev(n, rows, sizeof(rows), nullptr, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_items_dev(n, rows, sizeof(rows), off, nullptr, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_items_dev(n, nullptr, 0, nullptr, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_build_dev(n, nullptr, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_paths_dev(n, nullptr, 4, idx, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_paths_dev(n, nullptr, 0, idx, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_paths_dev(n, tree, 4, nullptr, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_paths_dev(n, tree, 4, idx, nullptr, nullptr), ZK_ERR_ARG);
    // a misaligned digest, tree, path, offset or index pointer
    EXPECT(zk_blake2b_rows_dev(n, rows, 32, tree + 8, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_items_dev(n, rows, sizeof(rows), off, tree + 1, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_items_dev(n, rows, sizeof(rows), (uint8_t*)off + 4, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_build_dev(n, tree + 4, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_paths_dev(n, tree + 8, 4, idx, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_paths_dev(n, tree, 4, idx, paths + 8, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_paths_dev(n, tree, 4, (uint8_t*)idx + 1, paths, nullptr), ZK_ERR_ARG);
    // an output that overlaps an input
    EXPECT(zk_blake2b_rows_dev(n, rows, 32, rows, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_rows_dev(n, tree + 5 * 64 - 16, 32, tree, nullptr), ZK_ERR_ARG);       // the rows begin in the last digest
    EXPECT(zk_blake2b_rows_dev(2, rows, 32, rows + 48, nullptr), ZK_ERR_ARG);                // the digests begin in the last row
    EXPECT(zk_blake2b_items_dev(n, tree + 64, sizeof(rows), off, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_blake2b_items_dev(1, rows, sizeof(rows), tree + 48, tree, nullptr), ZK_ERR_ARG);   // two offsets in the digest
    EXPECT(zk_merkle_paths_dev(n, tree, 4, idx, tree + 10 * 64, nullptr), ZK_ERR_ARG);       // the paths begin in the root
    EXPECT(zk_merkle_paths_dev(n, paths + 64, 1, idx, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_merkle_paths_dev(n, tree, 2, paths + 3 * 64 - 16, paths, nullptr), ZK_ERR_ARG);    // the indices lie in the first path
    // nothing to do
    EXPECT(zk_merkle_paths_dev(n, tree, 0, idx, paths, nullptr), ZK_OK);
    EXPECT(zk_merkle_paths_dev(n, tree, 0, nullptr, nullptr, nullptr), ZK_OK);
    EXPECT(zk_merkle_paths_dev(1, tree, 4, idx, paths, nullptr), ZK_OK);    // depth 0: a path is empty
    EXPECT(zk_merkle_build_dev(1, tree, nullptr), ZK_OK);                   // one leaf is its own root
    // the layout: host arithmetic
    int depth = -1;
    uint64_t nodes = 0, lo[ZK_MERKLE_MAX_LOG + 2];
    for (int i = 0; i < ZK_MERKLE_MAX_LOG + 2; ++i) lo[i] = ~0ull;
    EXPECT(zk_merkle_layout(0, &depth, lo, &nodes), ZK_ERR_ARG);
    EXPECT(zk_merkle_layout(big, &depth, lo, &nodes), ZK_ERR_ARG);
    if (depth != -1 || nodes != 0 || lo[0] != ~0ull) { printf("  FAILED: a refused layout call wrote\n"); ++g_errors; }
    EXPECT(zk_merkle_layout(n, nullptr, nullptr, nullptr), ZK_OK);
    EXPECT(zk_merkle_layout(n, &depth, lo, &nodes), ZK_OK);
    if (depth != 3 || nodes != 11 || lo[0] != 0 || lo[1] != 5 || lo[2] != 8 || lo[3] != 10 || lo[4] != ~0ull) {
        printf("  FAILED: layout of 5 leaves\n"); ++g_errors;
    }
    EXPECT(zk_merkle_layout(1, &depth, lo, &nodes), ZK_OK);
    if (depth != 0 || nodes != 1 || lo[0] != 0) { printf("  FAILED: layout of 1 leaf\n"); ++g_errors; }
    EXPECT(zk_merkle_layout(1ull << ZK_MERKLE_MAX_LOG, &depth, lo, &nodes), ZK_OK);
    if (depth != ZK_MERKLE_MAX_LOG || nodes != (2ull << ZK_MERKLE_MAX_LOG) - 1 || lo[ZK_MERKLE_MAX_LOG] != nodes - 1 || lo[ZK_MERKLE_MAX_LOG + 1] != ~0ull) {
        printf("  FAILED: layout of 2^26 leaves\n"); ++g_errors;
    }
    // past the checks: the launch fails
    EXPECT(zk_blake2b_rows_dev(n, rows, 32, tree, nullptr), ZK_ERR_HIP);
    EXPECT(zk_blake2b_rows_dev(n, rows + 1, 31, tree, nullptr), ZK_ERR_HIP);                 // the byte path
    EXPECT(zk_blake2b_rows_dev(n, nullptr, 0, tree, nullptr), ZK_ERR_HIP);                   // no bytes to read
    EXPECT(zk_blake2b_rows_dev(n, tree + 5 * 64, 32, tree, nullptr), ZK_ERR_HIP);            // the rows begin where the digests end
    EXPECT(zk_blake2b_items_dev(n, rows, sizeof(rows), off, tree, nullptr), ZK_ERR_HIP);
    EXPECT(zk_blake2b_items_dev(n, nullptr, 0, off, tree, nullptr), ZK_ERR_HIP);
    EXPECT(zk_merkle_build_dev(n, tree, nullptr), ZK_ERR_HIP);
    EXPECT(zk_merkle_build_dev(1ull << ZK_MERKLE_MAX_LOG, tree, nullptr), ZK_ERR_HIP);       // refused by the launch, nothing is touched
    EXPECT(zk_merkle_paths_dev(n, tree, 4, idx, paths, nullptr), ZK_ERR_HIP);
    for (unsigned i = 0; i < sizeof(tree); ++i)
        if (tree[i]) { printf("  FAILED: a call wrote to the tree\n"); ++g_errors; break; }
    for (unsigned i = 0; i < sizeof(paths); ++i)
        if (paths[i] || rows[i % sizeof(rows)]) { printf("  FAILED: a call wrote to the paths or the rows\n"); ++g_errors; break; }
    if (g_errors) printf("merkle_args_check: %d FAILED\n", g_errors);
    else printf("merkle_args_check: all ok\n");
    return g_errors ? 1 : 0;
}
