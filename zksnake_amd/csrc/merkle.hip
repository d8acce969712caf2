// merkle.hip -- BLAKE2b-512 leaf digests, Merkle trees over them and batched opening paths (gfx950).
//
// Stands in for the hashlib loops of the reference's vector commitment (python/zksnake/commitment/vector/merkle.py): one Python
// hash call per leaf and per node, and the whole tree again for every open.  Here a digest is ONE LANE's work: the 8-word chaining
// value, the 16-word message block and the 16-word working state stay in registers, a compression is 96 G functions of 64-bit
// add / xor / rotate and no multiply.  The rotations by 24, 16 and 63 are pairs of 32-bit funnel shifts (v_alignbit_b32), the one
// by 32 is a swap of halves and costs nothing.  BLAKE2b as hashlib.new("blake2b", data) computes it: RFC 7693, 64-byte digest, no
// key, salt or personalisation, so h[0] starts as IV[0] ^ 0x01010040.
//
// A tree has the shape of merkle_tree.hip.h, 64 bytes per node; a node without a right sibling is hashed with itself (the
// reference's _build_tree).  Layout, build schedule and the gather of opening paths are that header's; this file brings the hash.
// Workgroups of MLE_TILE threads on the capped strided grid of fr_sum.hip.h; plain C++, no atomics.
#include "merkle_tree.hip.h"

namespace zkmi {

constexpr uint64_t DIGEST = ZK_MERKLE_DIGEST;
constexpr int DIGEST_WORDS = 8;
// ---- BLAKE2b ------------------------------------------------------------------------------------------------------------

#define B2B_IV0 0x6a09e667f3bcc908ull
#define B2B_IV1 0xbb67ae8584caa73bull
#define B2B_IV2 0x3c6ef372fe94f82bull
#define B2B_IV3 0xa54ff53a5f1d36f1ull
#define B2B_IV4 0x510e527fade682d1ull
#define B2B_IV5 0x9b05688c2b3e6c1full
#define B2B_IV6 0x1f83d9abfb41bd6bull
#define B2B_IV7 0x5be0cd19137e2179ull

// x rotated right by N, 0 < N < 32, or by 32 + N: two funnel shifts over the halves, taken in swapped order past 32
template <int N, bool SWAP>
__device__ __forceinline__ uint64_t b2b_rotr(uint64_t x) {
    const uint32_t lo = SWAP ? (uint32_t)(x >> 32) : (uint32_t)x, hi = SWAP ? (uint32_t)x : (uint32_t)(x >> 32);
    return ((uint64_t)__builtin_amdgcn_alignbit(lo, hi, N) << 32) | __builtin_amdgcn_alignbit(hi, lo, N);
}
__device__ __forceinline__ uint64_t b2b_swap(uint64_t x) { return (x << 32) | (x >> 32); }   // rotation by 32: a renaming of halves

#define B2B_G(a, b, c, d, x, y)                \
    do {                                       \
        a = a + b + (x);                       \
        d = b2b_swap(d ^ a);                   \
        c = c + d;                             \
        b = b2b_rotr<24, false>(b ^ c);        \
        a = a + b + (y);                       \
        d = b2b_rotr<16, false>(d ^ a);        \
        c = c + d;                             \
        b = b2b_rotr<31, true>(b ^ c);         \
    } while (0)

// one round with the message schedule sigma written out: the indices are literals, so m[] never leaves the registers
#define B2B_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
    do {                                                                                \
        B2B_G(v0, v4, v8, v12, m[s0], m[s1]);                                           \
        B2B_G(v1, v5, v9, v13, m[s2], m[s3]);                                           \
        B2B_G(v2, v6, v10, v14, m[s4], m[s5]);                                          \
        B2B_G(v3, v7, v11, v15, m[s6], m[s7]);                                          \
        B2B_G(v0, v5, v10, v15, m[s8], m[s9]);                                          \
        B2B_G(v1, v6, v11, v12, m[s10], m[s11]);                                        \
        B2B_G(v2, v7, v8, v13, m[s12], m[s13]);                                         \
        B2B_G(v3, v4, v9, v14, m[s14], m[s15]);                                         \
    } while (0)

__device__ __forceinline__ void b2b_init(uint64_t h[DIGEST_WORDS]) {
    h[0] = B2B_IV0 ^ 0x01010040ull;   // digest length 64, key length 0, fanout 1, depth 1
    h[1] = B2B_IV1; h[2] = B2B_IV2; h[3] = B2B_IV3; h[4] = B2B_IV4; h[5] = B2B_IV5; h[6] = B2B_IV6; h[7] = B2B_IV7;
}

// h <- F(h, m, t, last): t = message bytes up to and including this block (below 2^64: the high counter word is zero)
__device__ __forceinline__ void b2b_compress(uint64_t h[DIGEST_WORDS], const uint64_t m[16], uint64_t t, bool last) {
    uint64_t v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3], v4 = h[4], v5 = h[5], v6 = h[6], v7 = h[7];
    uint64_t v8 = B2B_IV0, v9 = B2B_IV1, v10 = B2B_IV2, v11 = B2B_IV3, v12 = B2B_IV4 ^ t, v13 = B2B_IV5;
    uint64_t v14 = last ? ~B2B_IV6 : B2B_IV6, v15 = B2B_IV7;
    B2B_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    B2B_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
    B2B_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4);
    B2B_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8);
    B2B_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13);
    B2B_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9);
    B2B_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11);
    B2B_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10);
    B2B_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5);
    B2B_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0);
    B2B_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    B2B_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
    h[0] ^= v0 ^ v8;  h[1] ^= v1 ^ v9;  h[2] ^= v2 ^ v10; h[3] ^= v3 ^ v11;
    h[4] ^= v4 ^ v12; h[5] ^= v5 ^ v13; h[6] ^= v6 ^ v14; h[7] ^= v7 ^ v15;
}

// the first `avail` <= 128 bytes at p as a message block, zero beyond them.  words: p is a multiple of 8, so whole words are
// 64-bit loads; the bytes of a partial word, and every byte when p is not aligned, are loaded one by one.  Nothing at or past
// p + avail is read.
__device__ __forceinline__ void b2b_load_block(const uint8_t* p, uint32_t avail, bool words, uint64_t m[16]) {
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        uint64_t x = 0;
        if (words && 8u * w + 8 <= avail) {
            x = *reinterpret_cast<const uint64_t*>(p + 8 * w);
        } else if (8u * w < avail) {
#pragma unroll
            for (int b = 0; b < 8; ++b)
                if (8u * w + b < avail) x |= (uint64_t)p[8 * w + b] << (8 * b);
        }
        m[w] = x;
    }
}

// the digest of the len bytes at p (p is not read when len = 0).  The empty message is one zero block with t = 0; a message of
// 128 j bytes ends with its j-th full block, no empty one follows.
__device__ __forceinline__ void b2b_hash(const uint8_t* p, uint64_t len, bool words, uint64_t h[DIGEST_WORDS]) {
    b2b_init(h);
    uint64_t t = 0;
    for (;;) {
        const uint64_t rest = len - t;
        const bool last = rest <= 128;
        const uint32_t avail = last ? (uint32_t)rest : 128u;
        uint64_t m[16];
        b2b_load_block(p + t, avail, words, m);
        t += avail;
        b2b_compress(h, m, t, last);
        if (last) break;
    }
}

// a node is 64 bytes at a multiple of 16 (checked on the host): four 16-byte accesses
__device__ __forceinline__ void node_load(const void* p, uint64_t w[DIGEST_WORDS]) {
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const ulonglong2 t = q[i];
        w[2 * i] = t.x; w[2 * i + 1] = t.y;
    }
}
__device__ __forceinline__ void node_store(void* p, const uint64_t w[DIGEST_WORDS]) {
    ulonglong2* q = reinterpret_cast<ulonglong2*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = make_ulonglong2(w[2 * i], w[2 * i + 1]);
}

// parent i of a level of n_child nodes: H(child[2i] || child[2i+1]), child[2i] twice where 2i+1 is past the level.  The 128 bytes
// are exactly one final block.
__device__ __forceinline__ void merkle_parent(const uint8_t* child, uint64_t n_child, uint64_t i, uint8_t* parent) {
    const uint64_t l = 2 * i, r = l + 1 < n_child ? l + 1 : l;
    uint64_t m[16], h[DIGEST_WORDS];
    node_load(child + l * DIGEST, m);
    node_load(child + r * DIGEST, m + 8);
    b2b_init(h);
    b2b_compress(h, m, 128, true);
    node_store(parent + i * DIGEST, h);
}

__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ---- kernels ------------------------------------------------------------------------------------------------------------

// digest i = BLAKE2b(rows[i * row_bytes .. (i+1) * row_bytes)).  WORDS: rows and row_bytes are multiples of 8.
template <bool WORDS>
__global__ __launch_bounds__(MLE_TILE) void blake2b_rows_kernel(uint64_t n, const uint8_t* __restrict__ rows, uint64_t row_bytes,
                                                                uint8_t* __restrict__ digests) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; i < n; i += stride) {
        uint64_t h[DIGEST_WORDS];
        b2b_hash(rows + i * row_bytes, row_bytes, WORDS, h);
        node_store(digests + i * DIGEST, h);
    }
}

// digest i = BLAKE2b(data[off[i] .. off[i+1])), both ends clamped into [0, data_bytes] and the start to the end: whatever the
// offsets hold, nothing outside data is read.  An item that starts at a multiple of 8 takes the 64-bit loads.
__global__ __launch_bounds__(MLE_TILE) void blake2b_items_kernel(uint64_t n, const uint8_t* __restrict__ data, uint64_t data_bytes,
                                                                 const uint64_t* __restrict__ off, uint8_t* __restrict__ digests) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE;
    for (uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; i < n; i += stride) {
        const uint64_t end = umin64(off[i + 1], data_bytes), start = umin64(off[i], end);
        const uint8_t* p = data + start;
        uint64_t h[DIGEST_WORDS];
        b2b_hash(p, end - start, ((uintptr_t)p & 7) == 0, h);
        node_store(digests + i * DIGEST, h);
    }
}

__global__ __launch_bounds__(MLE_TILE) void merkle_level_kernel(uint64_t n_child, const uint8_t* __restrict__ child,
                                                                uint8_t* __restrict__ parent) {
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE, n_parent = (n_child + 1) / 2;
    for (uint64_t i = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; i < n_parent; i += stride) merkle_parent(child, n_child, i, parent);
}

// ---- host side ----------------------------------------------------------------------------------------------------------

static int blake2b_rows(uint64_t n, const void* d_rows, uint64_t row_bytes, void* d_digests, hipStream_t st) {
    ZK_HIP_RC(leaves_in_range(n, "blake2b_rows"));
    if (row_bytes >> 32) return fail(ZK_ERR_ARG, "blake2b_rows: a row has fewer than 2^32 bytes");
    if (!d_digests || (!d_rows && row_bytes)) return fail(ZK_ERR_ARG, "blake2b_rows: null pointer");
    if (!aligned16(d_digests)) return fail(ZK_ERR_ARG, "blake2b_rows: the digests start at a multiple of 16");
    const void* in[1] = {d_rows};
    const uint64_t len[1] = {n * row_bytes};
    if (overlaps_any(d_digests, n * DIGEST, in, len, 1)) return fail(ZK_ERR_ARG, "blake2b_rows: the digests overlap the rows");
    const bool words = (((uintptr_t)d_rows | row_bytes) & 7) == 0;
    if (words)
        hipLaunchKernelGGL(blake2b_rows_kernel<true>, dim3(fr_blocks(n)), dim3(MLE_TILE), 0, st, n, (const uint8_t*)d_rows, row_bytes, (uint8_t*)d_digests);
    else
        hipLaunchKernelGGL(blake2b_rows_kernel<false>, dim3(fr_blocks(n)), dim3(MLE_TILE), 0, st, n, (const uint8_t*)d_rows, row_bytes, (uint8_t*)d_digests);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

static int blake2b_items(uint64_t n, const void* d_data, uint64_t data_bytes, const void* d_offsets, void* d_digests, hipStream_t st) {
    ZK_HIP_RC(leaves_in_range(n, "blake2b_items"));
    if (!d_digests || !d_offsets || (!d_data && data_bytes)) return fail(ZK_ERR_ARG, "blake2b_items: null pointer");
    if (!aligned16(d_digests) || ((uintptr_t)d_offsets & 7))
        return fail(ZK_ERR_ARG, "blake2b_items: the digests start at a multiple of 16, the offsets at a multiple of 8");
    const void* in[2] = {d_data, d_offsets};
    const uint64_t len[2] = {data_bytes, (n + 1) * 8};
    if (overlaps_any(d_digests, n * DIGEST, in, len, 2)) return fail(ZK_ERR_ARG, "blake2b_items: the digests overlap an input");
    hipLaunchKernelGGL(blake2b_items_kernel, dim3(fr_blocks(n)), dim3(MLE_TILE), 0, st, n, (const uint8_t*)d_data, data_bytes,
                       (const uint64_t*)d_offsets, (uint8_t*)d_digests);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

static int merkle_build(uint64_t n, void* d_tree, hipStream_t st) {
    ZK_HIP_RC(tree_build_args("merkle_build", n, d_tree));
    return tree_build<DIGEST>(n, d_tree, [st](uint64_t width, const uint8_t* child, uint8_t* parent) {
        hipLaunchKernelGGL(merkle_level_kernel, dim3(fr_blocks((width + 1) / 2)), dim3(MLE_TILE), 0, st, width, child, parent);
    });
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_blake2b_rows_dev(uint64_t n, const void* d_rows, uint64_t row_bytes, void* d_digests, void* stream) {
    return blake2b_rows(n, d_rows, row_bytes, d_digests, (hipStream_t)stream);
}

int zk_blake2b_items_dev(uint64_t n, const void* d_data, uint64_t data_bytes, const void* d_offsets, void* d_digests, void* stream) {
    return blake2b_items(n, d_data, data_bytes, d_offsets, d_digests, (hipStream_t)stream);
}

int zk_merkle_layout(uint64_t n, int* depth, uint64_t* level_offset, uint64_t* nodes) {
    ZK_HIP_RC(leaves_in_range(n, "merkle_layout"));
    const TreeLayout lay = tree_layout(n);
    if (depth) *depth = lay.depth;
    if (nodes) *nodes = lay.nodes;
    if (level_offset)
        for (int l = 0; l <= lay.depth; ++l) level_offset[l] = lay.offset[l];
    return ZK_OK;
}

int zk_merkle_build_dev(uint64_t n, void* d_tree, void* stream) { return merkle_build(n, d_tree, (hipStream_t)stream); }

int zk_merkle_paths_dev(uint64_t n, const void* d_tree, uint64_t k, const void* d_indices, void* d_paths, void* stream) {
    return tree_paths<DIGEST>("merkle_paths", n, d_tree, k, d_indices, d_paths, (hipStream_t)stream);
}

}  // extern "C"
