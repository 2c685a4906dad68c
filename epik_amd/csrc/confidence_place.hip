// confidence_place.hip -- per-read placement confidence on the device: the tree object (epik_amd_tree_create / _destroy
// / _info / _build_host / _lca_host), epik_amd_confidence_device, and confidence_host_chunked, the host side that the
// four epik_amd_placer_confidence_* entries share (host_entry.hpp); epik_amd_placer_confidence_reads itself.
//
// No reference counterpart: the reference writes a jplace and leaves EDPL and LCA assignment to a second tool.
//
// The rule (include/epik_amd.h; epik_amd/host/confidence.cpp is the same rule on the CPU).  For read i,
// keep = keep_at_most, nr = min(n_rows[i], keep), tested in this order:
//   n_rows[i] == EPIK_AMD_ROWS_COUNTS_TOO_NARROW   clade = EPIK_AMD_CLADE_TOO_NARROW, the other fields 0
//   n_rows[i] == 0                                 clade = EPIK_AMD_CLADE_TOO_SHORT,  the other fields 0
//   kmer_counts[i * keep] == 0                     clade = EPIK_AMD_CLADE_NO_HIT,     the other fields 0
//   a row j < nr with branch >= N                  clade = EPIK_AMD_CLADE_BAD_ROW,    the other fields 0
// otherwise, with b_j, lwr_j of row j and q(x) = llrint(x * 2^30):
//   S_m = sum over j < m of q(lwr_j), S = S_nr; m = the smallest m >= 1 with S_m * 2^30 >= tau_q * S in uint64 (nr when
//   there is none); clade = the lca of b_0 ... b_(m-1); clade_mass_q = the sum of q(lwr_j) over j < nr with first[clade]
//   <= b_j <= clade, saturating at 2^32 - 1; edpl = 2 * sum over j < l < nr of (lwr_j * lwr_l) * d(b_j, b_l), the pairs
//   added in lexicographic (j, l) order in double, multiply and add never fused (__dmul_rn / __dadd_rn below).
//   d(a, a) = 0; a in the clade of b: mid[a] - mid[b], and the other way round; else (mid[a] - depth[c]) + (mid[b] -
//   depth[c]) with c = lca(a, b).
// Slots past n_rows are read (the loads are unconditional, for coalescing) but never looked at.
//
// confidence_kernel: a read belongs to a group of P lanes, P = the power of two >= keep (8 for keep 7: eight reads a
// wave), lane j of the group holds row j -- the wave's loads are consecutive 16-byte rows but for the P - keep idle lanes
// of each group.  The group sorts its branches by post-order id (ranks by P shuffles); lane r takes lca(sorted[r],
// sorted[r + 1]): nr - 1 table walks a read, all at once.  The lca of ANY two of the branches is the largest id among
// the adjacent lcas between them (everything between two ids lies in the clade of their lca, and one adjacent pair
// straddles two of its children), so the clade -- the lca of the prefix's lowest and highest id -- and the lca of each
// of the nr (nr - 1) / 2 pairs of the EDPL cost no further walk, only a maximum over a few cells in LDS.  The terms
// of the EDPL are formed a row against all later rows at a time, then added in the rule's order, every lane of the
// group the same adds.  Control flow is uniform over the workgroup (predicates, no early exit): every shuffle, ballot
// and barrier is met by all lanes.  One record has one writer: no atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "host_entry.hpp"
#include "tree_tables.hpp"

struct epik_amd_tree {
    int device = 0;
    uint32_t num_branches = 0, levels = 0;
    uint64_t bytes = 0;
    uint32_t max_blocks_cap = 0;  // EPIK_AMD_MAX_BLOCKS at create()
    void *d_tables = nullptr;
    epik_amd::TreeView view{};  // device pointers
};

namespace {

using namespace epik_amd;

constexpr uint32_t kLwrBits = EPIK_AMD_PROFILE_LWR_BITS;
constexpr uint64_t kMaxBlocks = 4096;  // (grid-stride beyond: 16 workgroups a CU)
static_assert(sizeof(epik_amd_confidence) == 16 && sizeof(epik_amd_placement) == 16);

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kBlock) void confidence_kernel(TreeView tree, const u32x4 *__restrict__ rows,
                                                            const uint32_t *__restrict__ n_rows,
                                                            const uint32_t *__restrict__ kmer_counts, uint64_t n, uint32_t keep,
                                                            uint32_t group, uint32_t tau_q, u32x4 *__restrict__ out)
{
    __shared__ uint32_t s_sorted[kBlock];  // per group: the branches by ascending id
    __shared__ uint32_t s_prefix[kBlock];  // ... 1 where the row of that id belongs to the prefix of the clade
    __shared__ uint32_t s_adj[kBlock];     // ... lca(sorted[r], sorted[r + 1])
    const int P = (int)group;
    const uint32_t j = threadIdx.x & (group - 1), base = threadIdx.x - j;  // my row; my group's first cell in LDS
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long gmask = (group == kWave ? ~0ull : ((1ull << group) - 1)) << (lane - j);
    const uint64_t per_block = kBlock / group, tiles = (n + per_block - 1) / per_block;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t i = t * per_block + threadIdx.x / group;
        const bool slot = i < n && j < keep;
        u32x4 row = {0, 0, 0, 0};
        uint32_t raw_nr = 0, hits = 0;
        if (slot) row = rows[i * keep + j];
        if (i < n) raw_nr = n_rows[i], hits = kmer_counts[i * keep];
        uint32_t cls = 0;
        if (raw_nr == EPIK_AMD_ROWS_COUNTS_TOO_NARROW)
            cls = EPIK_AMD_CLADE_TOO_NARROW;
        else if (raw_nr == 0)
            cls = EPIK_AMD_CLADE_TOO_SHORT;
        else if (hits == 0)
            cls = EPIK_AMD_CLADE_NO_HIT;
        uint32_t nr = cls ? 0u : std::min(raw_nr, keep);
        if ((__ballot(j < nr && row.x >= tree.n) & gmask) != 0) cls = EPIK_AMD_CLADE_BAD_ROW, nr = 0;
        const bool mine = j < nr;  // a row the rule looks at
        const uint32_t b = mine ? row.x : 0u;
        const double lwr = mine ? __hiloint2double((int)row.w, (int)row.z) : 0.0;
        const uint64_t q = mine ? (uint64_t)__double2ll_rn(lwr * (double)(1u << kLwrBits)) : 0ull;
        const double mid = tree.mid[b];

        // S_m, inclusive, and S
        unsigned long long s_m = q;
        for (int d = 1; d < P; d <<= 1) {
            const unsigned long long v = __shfl_up(s_m, d, P);
            if ((int)j >= d) s_m += v;
        }
        const unsigned long long s_all = __shfl(s_m, P - 1, P);
        const unsigned long long reached = __ballot(mine && (s_m << kLwrBits) >= (unsigned long long)tau_q * s_all) & gmask;
        const uint32_t m = reached ? (uint32_t)__ffsll((long long)reached) - 1 - (lane - j) + 1 : nr;

        // rank of my branch among the group's (ties by row; the idle lanes keep their own cells behind)
        uint32_t rank = mine ? 0u : j;
        for (int l = 0; l < P; ++l) {
            const uint32_t other = __shfl(b, l, P);
            if (mine && (uint32_t)l < nr && (other < b || (other == b && (uint32_t)l < j))) ++rank;
        }
        __syncthreads();  // (the cells of the tile before)
        s_sorted[base + rank] = b;
        s_prefix[base + rank] = mine && j < m ? 1u : 0u;
        __syncthreads();
        const uint32_t here = s_sorted[base + j];
        const uint32_t next = s_sorted[base + std::min(j + 1, group - 1)];
        s_adj[base + j] = j + 1 < nr ? tree_lca(tree, here, next) : 0u;
        const unsigned long long in_prefix = __ballot(s_prefix[base + j] != 0) & gmask;
        __syncthreads();

        // the clade: the lca of the prefix's lowest and highest id
        uint32_t clade = 0;
        if (nr) {
            const uint32_t lo = (uint32_t)__ffsll((long long)in_prefix) - 1 - (lane - j);
            const uint32_t hi = 63u - (uint32_t)__clzll((long long)in_prefix) - (lane - j);
            clade = s_sorted[base + lo];
            for (uint32_t r = lo; r < hi; ++r) clade = std::max(clade, s_adj[base + r]);
        }
        const uint32_t clade_first = tree.first[clade];
        unsigned long long in_clade = mine && clade_first <= b && b <= clade ? q : 0ull;
        for (int d = P / 2; d > 0; d >>= 1) in_clade += __shfl_xor(in_clade, d, P);

        // the EDPL: row j0 against every later row l, lane l forming the term; then the adds, in (j0, l) order
        double sum = 0.0;
        for (uint32_t j0 = 0; j0 + 1 < keep; ++j0) {
            const uint32_t b0 = __shfl(b, (int)j0, P), rank0 = __shfl(rank, (int)j0, P);
            const double mid0 = __shfl(mid, (int)j0, P), lwr0 = __shfl(lwr, (int)j0, P);
            double term = 0.0;
            if (mine && j > j0) {
                const uint32_t r_lo = std::min(rank0, rank), r_hi = std::max(rank0, rank), top = std::max(b0, b);
                uint32_t c = s_adj[base + r_lo];
                for (uint32_t r = r_lo + 1; r < r_hi; ++r) c = std::max(c, s_adj[base + r]);
                double dist;
                if (c == top) {  // one lies in the clade of the other (or they are the same branch)
                    dist = b0 < b ? __dsub_rn(mid0, mid) : __dsub_rn(mid, mid0);
                } else {
                    const double depth = tree.depth[c];
                    dist = __dadd_rn(__dsub_rn(mid0, depth), __dsub_rn(mid, depth));
                }
                term = __dmul_rn(__dmul_rn(lwr0, lwr), dist);
            }
            for (uint32_t l = j0 + 1; l < keep; ++l) {
                const double add = __shfl(term, (int)l, P);
                if (l < nr) sum = __dadd_rn(sum, add);
            }
        }
        if (i < n && j == 0) {
            u32x4 rec = {cls, 0u, 0u, 0u};
            if (!cls) {
                const double edpl = __dmul_rn(2.0, sum);
                rec.x = clade;
                rec.y = in_clade > 0xffffffffull ? 0xffffffffu : (uint32_t)in_clade;
                rec.z = (uint32_t)__double2loint(edpl);
                rec.w = (uint32_t)__double2hiint(edpl);
            }
            out[i] = rec;
        }
    }
}

int confidence_device_impl(const epik_amd_tree *tree, const void *d_rows, const void *d_n_rows, const void *d_kmer_counts,
                           uint64_t n, uint32_t keep, uint32_t tau_q, void *d_out, hipStream_t stream)
{
    if (!tree) return fail_with(EPIK_AMD_ERR_INVALID, "null tree");
    if (tau_q > (1u << kLwrBits)) return fail_with(EPIK_AMD_ERR_INVALID, "tau_q must lie in [0, 2^30]");
    if (keep == 0 || keep > kWave) return fail_with(EPIK_AMD_ERR_INVALID, "keep must be in [1, 64]");
    if (n == 0) return EPIK_AMD_OK;
    if (!d_rows || !d_n_rows || !d_kmer_counts || !d_out)
        return fail_with(EPIK_AMD_ERR_INVALID, "null device buffer (the k-mer counts are required: they tell a read without hits)");
    if (n > 0xffffffffull) return fail_with(EPIK_AMD_ERR_INVALID, "a batch of 2^32 reads or more");
    HIP_TRY(hipSetDevice(tree->device));
    uint32_t group = 1;
    while (group < keep) group *= 2;
    const uint64_t per_block = kBlock / group, tiles = (n + per_block - 1) / per_block;
    const uint64_t max_blocks = tree->max_blocks_cap ? std::min<uint64_t>(kMaxBlocks, tree->max_blocks_cap) : kMaxBlocks;
    hipLaunchKernelGGL(confidence_kernel, dim3((uint32_t)std::min(tiles, max_blocks)), dim3(kBlock), 0, stream, tree->view,
                       static_cast<const u32x4 *>(d_rows), static_cast<const uint32_t *>(d_n_rows),
                       static_cast<const uint32_t *>(d_kmer_counts), n, keep, group, tau_q, static_cast<u32x4 *>(d_out));
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

// what the sink of a placement with confidence carries from chunk to chunk
struct ConfidenceSink {
    const epik_amd_tree *tree;
    uint32_t keep, tau_q;
    epik_amd_confidence *d_conf, *conf;  // [n] of the whole batch: on the device, on the host
    epik_amd_profile *profile;           // or null
    const uint32_t *d_weights;           // [n] on the device, or null
};

int confidence_chunk(void *ctx, const epik_amd_placement *d_rows, const uint32_t *d_n_rows, const uint32_t *d_counts,
                     uint64_t first, uint64_t count, hipStream_t stream)
{
    const auto *sink = static_cast<const ConfidenceSink *>(ctx);
    if (const int rc = confidence_device_impl(sink->tree, d_rows, d_n_rows, d_counts, count, sink->keep, sink->tau_q,
                                              sink->d_conf + first, stream);
        rc != EPIK_AMD_OK)
        return rc;
    HIP_TRY(hipMemcpyAsync(sink->conf + first, sink->d_conf + first, count * sizeof(epik_amd_confidence), hipMemcpyDeviceToHost, stream));
    if (!sink->profile) return EPIK_AMD_OK;
    return epik_amd_profile_add_device(sink->profile, d_rows, d_n_rows, d_counts, sink->d_weights ? sink->d_weights + first : nullptr,
                                       count, stream);
}

int no_workspace(const epik_amd_placer *, uint64_t, uint64_t, uint32_t, uint64_t *bytes)
{
    *bytes = 0;
    return EPIK_AMD_OK;
}

int place_forward(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets, uint64_t n, uint32_t, void *, uint64_t,
                  void *d_rows, void *d_n_rows, void *d_kmer_counts, void *, hipStream_t stream)
{
    return epik_amd_placer_place_device(p, d_seqs, d_seq_offsets, n, d_rows, d_n_rows, d_kmer_counts, stream);
}

constexpr HostVariant kForwardHost{.chunk_reads = 1u << 18, .chunk_bytes = 64u << 20, .chunk_reads_env = "EPIK_AMD_CONFIDENCE_CHUNK_READS",
                                   .workspace_bytes = no_workspace, .zeroed_bytes = nullptr, .place_device = place_forward};

}  // namespace

namespace epik_amd {

int confidence_host_chunked(epik_amd_placer *p, const ConfidenceRequest &req, const char *seqs, const uint64_t *seq_offsets,
                            uint64_t n, uint32_t mode, uint64_t longest_placed, const HostVariant &v, epik_amd_placement *rows,
                            uint32_t *n_rows, uint32_t *kmer_counts, uint8_t *label)
{
    if (!p) return fail_with(EPIK_AMD_ERR_INVALID, "null placer");
    if (!req.tree) return fail_with(EPIK_AMD_ERR_INVALID, "null tree");
    if (!req.conf) return fail_with(EPIK_AMD_ERR_INVALID, "null confidence buffer");
    if (req.tau_q > (1u << kLwrBits)) return fail_with(EPIK_AMD_ERR_INVALID, "tau_q must lie in [0, 2^30]");
    if (req.tree->device != p->device || req.tree->num_branches != p->params.num_branches)
        return fail_with(EPIK_AMD_ERR_INVALID, "the tree was created for another placer (device or num_branches differ)");
    if (p->plan.shard_count > 1)
        return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "placement confidence needs a whole database, not a k-mer-space shard");
    if (req.profile)
        if (const int rc = check_profile_pair(p, req.profile); rc != EPIK_AMD_OK) return rc;
    HIP_TRY(hipSetDevice(p->device));
    struct DeviceArrays {  // (freed however the call ends; place_host_chunked has drained the stream by then, or never used it)
        void *conf = nullptr, *weights = nullptr;
        hipStream_t stream = nullptr;
        ~DeviceArrays()
        {
            if (conf || weights) (void)hipStreamSynchronize(stream);
            if (conf) (void)hipFree(conf);
            if (weights) (void)hipFree(weights);
        }
    } d;
    d.stream = p->stream;
    HIP_TRY(hipMalloc(&d.conf, n * sizeof(epik_amd_confidence)));
    if (req.profile && req.weights) {
        HIP_TRY(hipMalloc(&d.weights, n * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(d.weights, req.weights, n * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    }
    ConfidenceSink ctx{req.tree, p->params.keep_at_most, req.tau_q, static_cast<epik_amd_confidence *>(d.conf), req.conf,
                       req.profile, static_cast<const uint32_t *>(d.weights)};
    const ChunkSink sink{confidence_chunk, &ctx};
    return place_host_chunked(p, seqs, seq_offsets, n, mode, longest_placed, v, rows, n_rows, kmer_counts, label, &sink);
}

int tree_first_device(const epik_amd_tree *tree, int *device, uint32_t *num_branches, const uint32_t **d_first)
{
    if (!tree) return fail_with(EPIK_AMD_ERR_INVALID, "null tree");
    *device = tree->device, *num_branches = tree->num_branches, *d_first = tree->view.first;
    return EPIK_AMD_OK;
}

}  // namespace epik_amd

extern "C" {

int epik_amd_tree_build_host(const uint32_t *parent, const double *branch_length, uint32_t num_branches, void *tables,
                             uint64_t *table_bytes)
{
    try {
        if (num_branches == 0) return fail_with(EPIK_AMD_ERR_INVALID, "a tree has at least one branch");
        if (table_bytes) *table_bytes = tree_table_bytes(num_branches);
        if (!tables) return table_bytes ? EPIK_AMD_OK : fail_with(EPIK_AMD_ERR_INVALID, "null argument");
        if (!parent || !branch_length) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
        std::string err;
        if (const int rc = tree_build(parent, branch_length, num_branches, tables, err); rc != EPIK_AMD_OK) return fail_with(rc, err);
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("tree_build_host: ") + e.what());
    }
}

int epik_amd_tree_lca_host(const void *tables, const uint32_t *a, const uint32_t *b, uint64_t n, uint32_t *out)
{
    if (!tables || (n && (!a || !b || !out))) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    TreeHeader head;
    std::memcpy(&head, tables, sizeof head);
    if (head.magic != kTreeMagic || head.num_branches == 0 || head.levels != tree_levels(head.num_branches))
        return fail_with(EPIK_AMD_ERR_INVALID, "not the tables of epik_amd_tree_build_host");
    const TreeView v = tree_view(tables, head.num_branches, head.levels);
    for (uint64_t i = 0; i < n; ++i) {
        if (a[i] >= v.n || b[i] >= v.n) return fail_with(EPIK_AMD_ERR_INVALID, "query " + std::to_string(i) + " names a branch outside the tree");
        out[i] = tree_lca(v, a[i], b[i]);
    }
    return EPIK_AMD_OK;
}

int epik_amd_tree_create(int32_t device, const uint32_t *parent, const double *branch_length, uint32_t num_branches,
                         epik_amd_tree **out)
{
    try {
        if (!out) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
        *out = nullptr;
        if (!parent || !branch_length) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
        if (num_branches == 0) return fail_with(EPIK_AMD_ERR_INVALID, "a tree has at least one branch");
        std::vector<uint8_t> tables(tree_table_bytes(num_branches));
        std::string err;
        if (const int rc = tree_build(parent, branch_length, num_branches, tables.data(), err); rc != EPIK_AMD_OK) return fail_with(rc, err);
        if (device < 0 || device >= epik_amd_device_count())
            return fail_with(EPIK_AMD_ERR_NO_DEVICE, "HIP device " + std::to_string(device) + " is not available (no CPU fallback exists)");
        auto *tree = new (std::nothrow) epik_amd_tree;
        if (!tree) return fail_with(EPIK_AMD_ERR_INVALID, "out of memory");
        tree->device = device;
        tree->num_branches = num_branches;
        tree->levels = tree_levels(num_branches);
        tree->bytes = tables.size();
        if (const char *e = std::getenv("EPIK_AMD_MAX_BLOCKS")) tree->max_blocks_cap = (uint32_t)std::strtoul(e, nullptr, 10);
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipMalloc(&tree->d_tables, tables.size());
        if (e == hipSuccess) e = hipMemcpy(tree->d_tables, tables.data(), tables.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (tree->d_tables) (void)hipFree(tree->d_tables);
            delete tree;
            return fail_with(EPIK_AMD_ERR_HIP, std::string("epik_amd_tree_create: ") + hipGetErrorString(e));
        }
        tree->view = tree_view(tree->d_tables, num_branches, tree->levels);
        *out = tree;
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("tree_create: ") + e.what());
    }
}

void epik_amd_tree_destroy(epik_amd_tree *tree)
{
    if (!tree) return;
    if (hipSetDevice(tree->device) == hipSuccess) {
        (void)hipDeviceSynchronize();
        (void)hipFree(tree->d_tables);
    }
    delete tree;
}

int epik_amd_tree_info(const epik_amd_tree *tree, uint32_t *num_branches, uint32_t *levels, uint64_t *table_bytes)
{
    if (!tree) return fail_with(EPIK_AMD_ERR_INVALID, "null tree");
    if (num_branches) *num_branches = tree->num_branches;
    if (levels) *levels = tree->levels;
    if (table_bytes) *table_bytes = tree->bytes;
    return EPIK_AMD_OK;
}

int epik_amd_confidence_device(const epik_amd_tree *tree, const void *d_rows, const void *d_n_rows, const void *d_kmer_counts,
                               uint64_t n, uint32_t keep, uint32_t tau_q, void *d_out, void *stream)
{
    return confidence_device_impl(tree, d_rows, d_n_rows, d_kmer_counts, n, keep, tau_q, d_out, static_cast<hipStream_t>(stream));
}

int epik_amd_placer_confidence_reads(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                     epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts, const epik_amd_tree *tree,
                                     uint32_t tau_q, epik_amd_confidence *conf, epik_amd_profile *profile, const uint32_t *weights)
{
    try {  // std::vector: nothing may leave through the C ABI
        if (!p) return fail_with(EPIK_AMD_ERR_INVALID, "null placer");
        if (n == 0) return EPIK_AMD_OK;
        uint64_t longest = 0;
        if (const int rc = check_host_reads(seqs, seq_offsets, n, longest); rc != EPIK_AMD_OK) return rc;
        return confidence_host_chunked(p, ConfidenceRequest{tree, tau_q, conf, profile, weights}, seqs, seq_offsets, n, 0, longest,
                                       kForwardHost, rows, n_rows, kmer_counts, nullptr);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("confidence_reads: ") + e.what());
    }
}

}  // extern "C"
