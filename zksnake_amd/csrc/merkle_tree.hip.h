// merkle_tree.hip.h -- what a Merkle tree is apart from its hash: the layout of its levels, the schedule that builds them, the
// gather of opening paths and the argument rules of both.  merkle.hip (BLAKE2b, 64-byte nodes) and poseidon.hip (32-byte nodes)
// bring the hash: a kernel that makes one level from the one below.  DESIGN.md section 4.12 describes the shape.
//
// A tree is its levels one after the other, NODE_BYTES per node: level 0 (the n leaf digests) first, level l has
// ceil(n_(l-1) / 2) nodes, the root is the last node.  A node without a right sibling is hashed with itself.
#pragma once
#include "fr_sum.hip.h"

namespace zkmi {

static_assert(ZK_MERKLE_MAX_LOG == ZK_POSEIDON_MAX_LOG && ZK_MERKLE_MAX_LOG == 26, "one leaf limit, the one leaves_in_range names");
constexpr int TREE_MAX_LOG = ZK_MERKLE_MAX_LOG;
constexpr uint64_t TREE_MAX_LEAVES = 1ull << TREE_MAX_LOG;

struct TreeLayout {
    int depth;
    uint64_t nodes;
    uint64_t offset[TREE_MAX_LOG + 1];   // of level l, in nodes
};

static TreeLayout tree_layout(uint64_t n) {
    TreeLayout lay{};
    uint64_t width = n;
    for (;;) {
        lay.offset[lay.depth] = lay.nodes;
        lay.nodes += width;
        if (width == 1) break;
        width = (width + 1) / 2;
        ++lay.depth;
    }
    return lay;
}

// entry (q, l) of the paths of k queries into a tree of n leaves: the sibling of query q's ancestor at level l, the ancestor
// itself where it has none.  An index past the leaves opens the last leaf.  A node is NODE_BYTES at a multiple of 16 (checked on
// the host): NODE_BYTES / 16 16-byte loads, all of them issued before the first store.
template <int NODE_BYTES>
__global__ __launch_bounds__(MLE_TILE) void tree_paths_kernel(uint64_t n, TreeLayout lay, const uint4* __restrict__ tree, uint64_t k,
                                                              const uint64_t* __restrict__ indices, uint4* __restrict__ paths) {
    constexpr int QUADS = NODE_BYTES / 16;
    static_assert(NODE_BYTES == QUADS * 16 && QUADS >= 1, "a node is whole 16-byte accesses");
    const uint64_t stride = (uint64_t)gridDim.x * MLE_TILE, depth = (uint64_t)lay.depth, items = k * depth;
    for (uint64_t e = (uint64_t)blockIdx.x * MLE_TILE + threadIdx.x; e < items; e += stride) {
        const uint64_t q = e / depth, l = e - q * depth;
        const uint64_t width = (n + (1ull << l) - 1) >> l, last = n - 1, want = indices[q];
        const uint64_t idx = (want < last ? want : last) >> l;
        const uint64_t sib = (idx ^ 1) < width ? idx ^ 1 : idx;
        const uint4* node = tree + (lay.offset[l] + sib) * QUADS;
        uint4 w[QUADS];
#pragma unroll
        for (int i = 0; i < QUADS; ++i) w[i] = node[i];
#pragma unroll
        for (int i = 0; i < QUADS; ++i) paths[e * QUADS + i] = w[i];
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------

// a count of leaves, or of items hashed one per lane: both hashes share the limit
static int leaves_in_range(uint64_t n, const char* who) {
    if (n == 0 || n > TREE_MAX_LEAVES) return fail(ZK_ERR_ARG, std::string(who) + ": need 1 <= n <= 2^26");
    return ZK_OK;
}

// the arguments of a build: level 0 is in place at the front of d_tree
static int tree_build_args(const char* who, uint64_t n, const void* d_tree) {
    ZK_HIP_RC(leaves_in_range(n, who));
    if (!d_tree) return fail(ZK_ERR_ARG, std::string(who) + ": null tree");
    if (!aligned16(d_tree)) return fail(ZK_ERR_ARG, std::string(who) + ": the tree starts at a multiple of 16");
    return ZK_OK;
}

// levels 1 .. depth from level 0: launch_level(width, child, parent) enqueues the hash's kernel that makes the (width + 1) / 2
// nodes at `parent` from the `width` nodes at `child`.  One launch per level, down to the root's single lane: one workgroup that
// finishes the narrow levels behind barriers was measured and did not beat the launches it replaces (EXPERIMENTS.md "Merkle trees")
template <int NODE_BYTES, class LaunchLevel>
static int tree_build(uint64_t n, void* d_tree, LaunchLevel launch_level) {
    uint8_t* level = (uint8_t*)d_tree;
    for (uint64_t width = n; width > 1; width = (width + 1) / 2) {
        uint8_t* parent = level + width * NODE_BYTES;
        launch_level(width, (const uint8_t*)level, parent);
        ZK_HIP(hipGetLastError());
        level = parent;
    }
    return ZK_OK;
}

template <int NODE_BYTES>
static int tree_paths(const char* who, uint64_t n, const void* d_tree, uint64_t k, const void* d_indices, void* d_paths, hipStream_t st) {
    auto bad = [who](const char* what) { return fail(ZK_ERR_ARG, std::string(who) + what); };
    ZK_HIP_RC(leaves_in_range(n, who));
    if (!d_tree) return bad(": null tree");
    if (k == 0) return ZK_OK;
    if (k > (1ull << 32)) return bad(": at most 2^32 queries a call");
    if (!d_indices || !d_paths) return bad(": null pointer");
    if (!aligned16(d_tree) || !aligned16(d_paths) || ((uintptr_t)d_indices & 7))
        return bad(": tree and paths start at a multiple of 16, the indices at a multiple of 8");
    const TreeLayout lay = tree_layout(n);
    const uint64_t items = k * (uint64_t)lay.depth;
    const void* in[2] = {d_tree, d_indices};
    const uint64_t len[2] = {lay.nodes * NODE_BYTES, k * 8};
    if (overlaps_any(d_paths, items * NODE_BYTES, in, len, 2)) return bad(": the paths overlap an input");
    if (items == 0) return ZK_OK;   // one leaf: the root is the leaf's digest and a path is empty
    hipLaunchKernelGGL(tree_paths_kernel<NODE_BYTES>, dim3(fr_blocks(items)), dim3(MLE_TILE), 0, st, n, lay, (const uint4*)d_tree, k,
                       (const uint64_t*)d_indices, (uint4*)d_paths);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

}  // namespace zkmi
