// poseidon_args_check.cpp -- the host side of csrc/poseidon.hip (argument rules, overlap checks, the parameter generator) and the
// permutation's own arithmetic run on the host, as a stand-alone host program for a sanitizer run; no device code is built and no
// kernel can be launched.  Built and run by helpers.run_host_program, by the recipe in the header of merkle_args_check.cpp.
// Every refused call must come back with ZK_ERR_ARG before anything is written; the calls that pass the checks fail with
// ZK_ERR_HIP (the program sees no device: the parameter table cannot be made, and the empty device image holds no kernel), and
// the ones that have nothing to launch return ZK_OK.
#include <cstdio>
#include <cstdlib>
#include "../../zksnake_amd/csrc/poseidon.hip"

static int g_errors = 0;
#define EXPECT(call, want)                                                                       \
    do {                                                                                         \
        int got_ = (call);                                                                       \
        if (got_ != (want)) { printf("  FAILED line %d: %s = %d\n", __LINE__, #call, got_); ++g_errors; } \
    } while (0)

// hash(1, .., T - 1) on BN254 through poseidon_perm, the function the kernels run, on the table the kernels read
template <int T>
static void host_hash(uint32_t* out) {
    typedef BnFrParams P;
    const std::vector<uint32_t> tab = poseidon_table_host<P>(T);
    Fp<P> s[T];
    s[0] = fp_zero<P>();
    for (int j = 1; j < T; ++j) {
        uint32_t w[P::W] = {(uint32_t)j};
        s[j] = fp_from_canonical<P>(w);
    }
    poseidon_perm<P, T>(s, tab.data());
    fp_to_canonical<P>(out, s[0]);
}

int main() {
    const uint64_t n = 5, big = (1ull << ZK_POSEIDON_MAX_LOG) + 1;
    const int BN = ZK_CURVE_BN254, BLS = ZK_CURVE_BLS12_381;
    // in: 5 states of 5 elements | out: the same | tree: 11 nodes for n = 5, room for 16 | indices (4) | paths (4 x 3 nodes)
    alignas(64) static uint8_t in[25 * 32], out[25 * 32], tree[16 * 32], paths[4 * 3 * 32];
    alignas(64) static uint64_t idx[4];
    // a size out of range
    EXPECT(zk_poseidon_perm_dev(BN, 3, 0, in, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_perm_dev(BN, 3, big, in, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_perm_dev(BN, 3, ~0ull, in, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_hash_dev(BN, 2, 0, in, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_hash_dev(BLS, 2, big, in, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_sponge_rows_dev(BN, 0, in, 2, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_sponge_rows_dev(BN, big, in, 2, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_sponge_rows_dev(BN, n, in, 0, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_sponge_rows_dev(BN, n, in, (uint64_t)ZK_POSEIDON_MAX_ROW + 1, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_sponge_rows_dev(BN, n, in, ~0ull, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_build_dev(BN, 0, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_build_dev(BN, big, tree, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_paths_dev(0, tree, 4, idx, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_paths_dev(big, tree, 4, idx, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_paths_dev(n, tree, (1ull << 32) + 1, idx, paths, nullptr), ZK_ERR_ARG);
    // a width, a row length or a curve that does not exist
    for (int t : {-1, 0, 2, 6, 1 << 30}) {
        EXPECT(zk_poseidon_perm_dev(BN, t, n, in, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_poseidon_params(BN, t, nullptr, nullptr, nullptr), ZK_ERR_ARG);
    }
    for (int k : {-1, 0, 1, 5}) EXPECT(zk_poseidon_hash_dev(BN, k, n, in, out, nullptr), ZK_ERR_ARG);
    for (int curve : {-1, 2, 7}) {
        EXPECT(zk_poseidon_params(curve, 3, nullptr, nullptr, nullptr), ZK_ERR_ARG);
        EXPECT(zk_poseidon_perm_dev(curve, 3, n, in, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_poseidon_hash_dev(curve, 2, n, in, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_poseidon_sponge_rows_dev(curve, n, in, 2, out, nullptr), ZK_ERR_ARG);
        EXPECT(zk_poseidon_merkle_build_dev(curve, n, tree, nullptr), ZK_ERR_ARG);
    }
    // a null pointer
    EXPECT(zk_poseidon_perm_dev(BN, 3, n, nullptr, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_perm_dev(BN, 3, n, in, nullptr, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_perm_dev(BN, 3, n, nullptr, nullptr, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_hash_dev(BN, 2, n, nullptr, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_hash_dev(BN, 2, n, in, nullptr, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_sponge_rows_dev(BN, n, nullptr, 2, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_sponge_rows_dev(BN, n, in, 2, nullptr, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_build_dev(BN, n, nullptr, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_build_dev(BN, 1, nullptr, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_paths_dev(n, nullptr, 4, idx, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_paths_dev(n, nullptr, 0, idx, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_paths_dev(n, tree, 4, nullptr, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_paths_dev(n, tree, 4, idx, nullptr, nullptr), ZK_ERR_ARG);
    // a misaligned pointer
    EXPECT(zk_poseidon_perm_dev(BN, 3, n, in + 8, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_perm_dev(BN, 3, n, in, out + 4, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_perm_dev(BN, 3, n, in + 8, in + 8, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_hash_dev(BN, 2, n, in + 1, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_hash_dev(BN, 2, n, in, out + 8, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_sponge_rows_dev(BN, n, in + 8, 2, out, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_sponge_rows_dev(BN, n, in, 2, out + 2, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_build_dev(BN, n, tree + 8, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_paths_dev(n, tree + 8, 4, idx, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_paths_dev(n, tree, 4, idx, paths + 8, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_paths_dev(n, tree, 4, (uint8_t*)idx + 1, paths, nullptr), ZK_ERR_ARG);
    // a forbidden overlap: anything but d_out == d_in for the permutation
    EXPECT(zk_poseidon_perm_dev(BN, 3, n, in, in + 32, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_perm_dev(BN, 3, n, in + 32, in, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_perm_dev(BN, 5, n, in, in + 25 * 32 - 16, nullptr), ZK_ERR_ARG);     // the output begins in the last state
    EXPECT(zk_poseidon_hash_dev(BN, 2, n, in, in, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_hash_dev(BN, 4, n, in, in + 20 * 32 - 16, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_hash_dev(BN, 2, n, in + 5 * 32 - 16, in, nullptr), ZK_ERR_ARG);      // the rows begin in the last digest
    EXPECT(zk_poseidon_sponge_rows_dev(BN, n, in, 1, in, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_sponge_rows_dev(BN, n, in, 5, in + 24 * 32, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_paths_dev(n, tree, 4, idx, tree + 10 * 32, nullptr), ZK_ERR_ARG);      // the paths begin in the root
    EXPECT(zk_poseidon_merkle_paths_dev(n, paths + 32, 1, idx, paths, nullptr), ZK_ERR_ARG);
    EXPECT(zk_poseidon_merkle_paths_dev(n, tree, 2, paths + 3 * 32 - 16, paths, nullptr), ZK_ERR_ARG);   // the indices lie in the first path
    // nothing to do
    EXPECT(zk_poseidon_merkle_paths_dev(n, tree, 0, idx, paths, nullptr), ZK_OK);
    EXPECT(zk_poseidon_merkle_paths_dev(n, tree, 0, nullptr, nullptr, nullptr), ZK_OK);
    EXPECT(zk_poseidon_merkle_paths_dev(1, tree, 4, idx, paths, nullptr), ZK_OK);    // depth 0: a path is empty
    EXPECT(zk_poseidon_merkle_build_dev(BN, 1, tree, nullptr), ZK_OK);               // one leaf is its own root
    EXPECT(zk_poseidon_merkle_build_dev(BLS, 1, tree, nullptr), ZK_OK);
    // the parameters: host arithmetic.  A refused call writes nothing; the counts; every value below r
    int rf = -1, rp = -1;
    static uint64_t par[(68 * 5 + 25 + 1) * 4];
    for (uint64_t& x : par) x = ~0ull;
    EXPECT(zk_poseidon_params(BN, 6, &rf, &rp, par), ZK_ERR_ARG);
    EXPECT(zk_poseidon_params(2, 3, &rf, &rp, par), ZK_ERR_ARG);
    if (rf != -1 || rp != -1 || par[0] != ~0ull) { printf("  FAILED: a refused params call wrote\n"); ++g_errors; }
    const int want_rp[3] = {57, 56, 60};
    for (int curve : {BN, BLS})
        for (int t = 3; t <= 5; ++t) {
            for (uint64_t& x : par) x = ~0ull;
            EXPECT(zk_poseidon_params(curve, t, &rf, &rp, nullptr), ZK_OK);
            EXPECT(zk_poseidon_params(curve, t, nullptr, nullptr, par), ZK_OK);
            const int count = (8 + want_rp[t - 3]) * t + t * t;
            if (rf != 8 || rp != want_rp[t - 3] || par[4 * count] != ~0ull || par[4 * count - 1] == ~0ull) {
                printf("  FAILED: round numbers or constant count, curve %d t %d\n", curve, t); ++g_errors;
            }
            const uint64_t top = curve == BN ? 0x30644e72e131a029ull : 0x73eda753299d7d48ull;   // the top limb of r
            for (int c = 0; c < count; ++c)
                if (par[4 * c + 3] > top) { printf("  FAILED: constant %d of curve %d t %d is not below r\n", c, curve, t); ++g_errors; break; }
        }
    // the permutation as the kernels compute it (poseidon_perm over the register-form table), on the host: circomlib's
    // Poseidon(3) of (1, 2, 3) -- the public output of the circom fixture -- and Poseidon(2) of (1, 2)
    const uint32_t want123[8] = {0xab36d732u, 0xf725df34u, 0x9dc5b968u, 0xf3230e26u, 0x8dab6302u, 0xff03d5e5u, 0x9e6939c0u, 0x0e7732d8u};
    const uint32_t want12[8] = {0x4417189au, 0x9e19607au, 0x74324551u, 0x2a3617f2u, 0x9662e9cfu, 0x3df64c6bu, 0xe7d69041u, 0x115cc0f5u};
    uint32_t got[8];
    host_hash<4>(got);
    if (memcmp(got, want123, sizeof(got))) { printf("  FAILED: host hash(1, 2, 3)\n"); ++g_errors; }
    host_hash<3>(got);
    if (memcmp(got, want12, sizeof(got))) { printf("  FAILED: host hash(1, 2)\n"); ++g_errors; }
    // past the checks: no device, so the parameter table or the launch fails
    EXPECT(zk_poseidon_perm_dev(BN, 3, n, in, out, nullptr), ZK_ERR_HIP);
    EXPECT(zk_poseidon_perm_dev(BLS, 5, n, in, in, nullptr), ZK_ERR_HIP);                    // in place
    EXPECT(zk_poseidon_perm_dev(BN, 4, n, in, in + 20 * 32, nullptr), ZK_ERR_HIP);           // the output begins where the input ends
    EXPECT(zk_poseidon_hash_dev(BN, 2, n, in, out, nullptr), ZK_ERR_HIP);
    EXPECT(zk_poseidon_hash_dev(BLS, 4, n, in, in + 20 * 32, nullptr), ZK_ERR_HIP);
    EXPECT(zk_poseidon_sponge_rows_dev(BN, n, in, 5, out, nullptr), ZK_ERR_HIP);
    EXPECT(zk_poseidon_sponge_rows_dev(BLS, 1, in, 1, out, nullptr), ZK_ERR_HIP);
    EXPECT(zk_poseidon_merkle_build_dev(BN, n, tree, nullptr), ZK_ERR_HIP);
    EXPECT(zk_poseidon_merkle_build_dev(BLS, 1ull << ZK_POSEIDON_MAX_LOG, tree, nullptr), ZK_ERR_HIP);   // refused before a launch, nothing is touched
    EXPECT(zk_poseidon_merkle_paths_dev(n, tree, 4, idx, paths, nullptr), ZK_ERR_HIP);
    zk_poseidon_free_cache();
    for (unsigned i = 0; i < sizeof(in); ++i)
        if (in[i] || out[i]) { printf("  FAILED: a call wrote to the vectors\n"); ++g_errors; break; }
    for (unsigned i = 0; i < sizeof(paths); ++i)
        if (paths[i] || tree[i % sizeof(tree)]) { printf("  FAILED: a call wrote to the paths or the tree\n"); ++g_errors; break; }
    if (g_errors) printf("poseidon_args_check: %d FAILED\n", g_errors);
    else printf("poseidon_args_check: all ok\n");
    return g_errors ? 1 : 0;
}
