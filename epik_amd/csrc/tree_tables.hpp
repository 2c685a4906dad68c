// tree_tables.hpp -- the tree of the placement confidence (include/epik_amd.h: epik_amd_tree): its tables as one block
// of memory, the same on the host and on the device, the LCA query over them -- ONE __host__ __device__ function, which
// confidence_kernel and epik_amd_tree_lca_host both call -- and the host code that validates a tree and fills the block.
// Internal to libepik_amd.
//
// The block: TreeHeader | depth f64[N] | mid f64[N] | lift {u32 up, u32 first_of_up}[levels][N] | first u32[N].
// lift[l][b].up is the 2^l-th ancestor of b, the root where b has none; levels = max(1, ceil(log2 N)), so that
// 2^levels - 1 >= N - 1 >= the depth of any node.  Binary lifting over parent[] with the range test, not an Euler tour
// with a sparse table: a query's operands are post-order ids already and first[] is what the clade test needs anyway,
// so lifting adds one table and no second numbering; the ancestor's first[] sits beside the ancestor, which makes a
// level ONE dependent 8-byte load.  N * (20 + 8 * levels) bytes: 1.4 MB at N = 10 399 -- it lives in L2.
#ifndef EPIK_AMD_TREE_TABLES_HPP
#define EPIK_AMD_TREE_TABLES_HPP
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "epik_amd.h"

namespace epik_amd {

struct TreeHeader {
    uint32_t magic, num_branches, levels, reserved;
    uint64_t bytes, reserved2;
};
constexpr uint32_t kTreeMagic = 0x45455254u;  // "TREE"

struct LiftCell {
    uint32_t up, first;
};

// the tables of a block at `base` (host or device memory alike)
struct TreeView {
    const double *depth, *mid;
    const LiftCell *lift;
    const uint32_t *first;
    uint32_t n, levels;
};

inline uint32_t tree_levels(uint32_t n)
{
    uint32_t levels = 1;
    while (levels < 32 && (1ull << levels) < n) ++levels;
    return levels;
}
inline uint64_t tree_table_bytes(uint32_t n)
{
    const uint64_t first_bytes = ((uint64_t)n * 4 + 7) / 8 * 8;
    return sizeof(TreeHeader) + (uint64_t)n * 16 + (uint64_t)tree_levels(n) * n * sizeof(LiftCell) + first_bytes;
}
inline TreeView tree_view(const void *base, uint32_t n, uint32_t levels)
{
    const auto *at = static_cast<const uint8_t *>(base) + sizeof(TreeHeader);
    TreeView v{};
    v.n = n, v.levels = levels;
    v.depth = reinterpret_cast<const double *>(at);
    v.mid = v.depth + n;
    v.lift = reinterpret_cast<const LiftCell *>(v.mid + n);
    v.first = reinterpret_cast<const uint32_t *>(v.lift + (uint64_t)levels * n);
    return v;
}

// lca(a, b) for a, b < N: the ancestor-or-self c of max(a, b), lowest in the tree, with first[c] <= min(first[a], first[b]).
// first[] never grows on the way up, so the ancestors that fail the test are the lowest ones: jump over them by
// descending powers of two, then take one step.  At most levels + 1 rounds of dependent loads.
__host__ __device__ inline uint32_t tree_lca(const TreeView &t, uint32_t a, uint32_t b)
{
    uint32_t c = a > b ? a : b;
    const uint32_t fa = t.first[a], fb = t.first[b], lo = fa < fb ? fa : fb;
    if ((a > b ? fa : fb) <= lo) return c;
    for (uint32_t l = t.levels; l-- > 0;) {
        const LiftCell cell = t.lift[(uint64_t)l * t.n + c];
        if (cell.first > lo) c = cell.up;
    }
    return t.lift[c].up;
}

// Validates the tree in the order include/epik_amd.h gives and fills `base` (tree_table_bytes(n) bytes).  Host only.
// 0, or EPIK_AMD_ERR_INVALID with `err` naming the branch.
inline int tree_build(const uint32_t *parent, const double *branch_length, uint32_t n, void *base, std::string &err)
{
    const auto bad = [&](uint32_t b, const std::string &what) {
        err = "branch " + std::to_string(b) + ": " + what;
        return (int)EPIK_AMD_ERR_INVALID;
    };
    std::vector<uint32_t> children(n, 0), first(n), stack;
    for (uint32_t b = 0; b + 1 < n; ++b)
        if (parent[b] != EPIK_AMD_TREE_NO_PARENT && parent[b] > b && parent[b] < n) ++children[parent[b]];
    stack.reserve(64);
    for (uint32_t b = 0; b < n; ++b) {
        if (!(branch_length[b] >= 0.0) || !std::isfinite(branch_length[b])) return bad(b, "the branch length is negative or not finite");
        if (b + 1 < n) {
            if (parent[b] == EPIK_AMD_TREE_NO_PARENT) return bad(b, "a second root (only the last branch has no parent)");
            if (parent[b] <= b || parent[b] >= n) return bad(b, "the parent " + std::to_string(parent[b]) + " is not above its child");
        } else if (parent[b] != EPIK_AMD_TREE_NO_PARENT) {
            return bad(b, "the last branch is the root and has no parent");
        }
        // post-order: the subtrees finished so far wait on a stack; the children of b are the ones on top
        uint32_t taken = 0, lowest = b;
        while (!stack.empty() && parent[stack.back()] == b) lowest = first[stack.back()], stack.pop_back(), ++taken;
        if (taken != children[b])
            return bad(b, "its descendants are not exactly the post-order ids [" + std::to_string(lowest) + ", " + std::to_string(b) + "]");
        first[b] = lowest;
        stack.push_back(b);
    }
    const uint32_t levels = tree_levels(n);
    TreeHeader head{kTreeMagic, n, levels, 0, tree_table_bytes(n), 0};
    std::memset(base, 0, head.bytes);
    std::memcpy(base, &head, sizeof head);
    const TreeView v = tree_view(base, n, levels);
    auto *depth = const_cast<double *>(v.depth), *mid = const_cast<double *>(v.mid);
    auto *lift = const_cast<LiftCell *>(v.lift);
    std::memcpy(const_cast<uint32_t *>(v.first), first.data(), (size_t)n * 4);
    for (uint32_t b = n; b-- > 0;) {  // from the root down: one add each
        const double above = b + 1 < n ? depth[parent[b]] : 0.0;
        depth[b] = above + branch_length[b];
        mid[b] = depth[b] - branch_length[b] / 2;
        const uint32_t up = b + 1 < n ? parent[b] : b;
        lift[b] = {up, first[up]};
    }
    for (uint32_t l = 1; l < levels; ++l)
        for (uint32_t b = 0; b < n; ++b) lift[(uint64_t)l * n + b] = lift[(uint64_t)(l - 1) * n + lift[(uint64_t)(l - 1) * n + b].up];
    return EPIK_AMD_OK;
}

}  // namespace epik_amd
#endif
