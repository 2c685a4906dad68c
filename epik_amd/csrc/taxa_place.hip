// taxa_place.hip -- taxonomic assignment of reads and samples on the device: the object epik_amd_taxonomy_* (create /
// destroy / reset / info / read / add_cells / add_device) and epik_amd_taxonomy_assign_host (include/epik_amd.h).
//
// No reference counterpart: the reference writes a jplace and leaves the question to a second tool.
//
// The rule is stated once, in include/epik_amd.h (epik_amd/host/taxonomy.cpp is the same rule on the
// CPU).  Every cell is a uint64 that wraps and integer adds commute -- no float atomic may appear in this file -- and the
// comparison mass(c) * 2^30 >= tau_q * S is made on 128-bit integers (high words by shift and __umul64hi): nothing wraps.
//
// taxa_kernel: confidence_kernel's shape (confidence_place.hip) with cohort_add_kernel's cells (cohort_place.hip).  A
// read belongs to a group of P lanes, P = the power of two >= keep, lane j of the group holds row j and gathers
// t_j = label[b_j].  The group sorts its taxa by id (ranks by P shuffles; the idle lanes stay behind with a taxon above
// all and no mass); lane r takes lca(sorted[r], sorted[r + 1]) over the taxonomy's tables: tree_lca, the function the
// confidence kernel calls.  The lowest qualifying taxon is the lca of the rows inside it, and the lca of ANY subset of
// an id-sorted set is one of its members or of its adjacent lcas, so the candidates are the nr row taxa and the nr - 1
// adjacent lcas: a lane weighs two, both in ONE pass over the group's sorted cells in LDS (every lane of a group reads
// the same cell: a broadcast) against first[c], compares exactly, and the group takes the minimum id.  The same pass
// sums the run of equal taxa a lane stands in: the run's first lane adds w * that sum to direct[] -- most rows of a
// read share a taxon, and one add per run, not per row, is what reaches the cells.  Control flow is uniform over the
// workgroup (predicates, no early exit): every shuffle, ballot and barrier is met by all lanes.  One record has one
// writer.
//
// The cells: a workgroup takes a CONTIGUOUS range of tiles (kBlock / P reads each) and keeps direct[T] | assigned[T] of
// ONE current sample in LDS: the sample of the first read of the tile at hand.  Reads of that sample add into LDS, reads
// of any other straight into the matrix; when the next tile begins in another sample the workgroup adds its non-zero
// LDS cells and the six totals (kept per lane, reduced over the wave and the workgroup) to the current sample's row and
// switches.  With LDS = false (taxonomies beyond kLdsLimit, EPIK_AMD_PROFILE_LDS=0) every cell add goes to global
// memory; the totals of the current sample are still reduced first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../host/taxonomy.hpp"
#include "cohort_device.hpp"
#include "host_entry.hpp"
#include "tree_tables.hpp"

struct epik_amd_taxonomy {
    int device = 0;
    uint32_t num_taxa = 0, num_samples = 0, num_branches = 0, keep = 0;
    bool lds = false;             // latched at create(): the LDS path
    uint32_t lds_blocks = 0;      // ... and its grid: kMaxBlocks, or a workgroup per CU beyond kLdsBudget
    uint32_t max_blocks_cap = 0;  // the placer's EPIK_AMD_MAX_BLOCKS
    void *d_tables = nullptr;     // the taxonomy's tree tables (tree_tables.hpp)
    epik_amd::TreeView view{};    // ... device pointers
    uint32_t *d_label = nullptr;  // [N]
    uint64_t *d_cells = nullptr;  // [S] x (direct[T] | assigned[T] | totals[kTotals]) | bad_samples
};

namespace {

using namespace epik_amd;

constexpr uint32_t kLwrBits = EPIK_AMD_PROFILE_LWR_BITS;
constexpr uint32_t kTotals = 6;  // placed, no_hit, too_short, too_narrow, no_mass, bad_reads: epik_amd_taxa_totals
// what the regimes leave for the kernel's own LDS beside the cells: s_q, s_sorted and the totals are 3 128 bytes; 4 096 is
// deliberate head-room, and the static_assert below keeps the arrays inside it
constexpr uint32_t kStaticLds = 4096;
static_assert(kBlock * (sizeof(uint64_t) + sizeof(uint32_t)) + 8 * sizeof(uint64_t) <= kStaticLds,
              "s_q, s_sorted and block_totals (6 totals, bad_samples, padding) must fit kStaticLds");
constexpr uint64_t kLdsBudget = (48u << 10) - kStaticLds;       // three workgroups a CU up to 2 816 taxa
constexpr uint64_t kLdsLimit = (160u << 10) - 64 - kStaticLds;  // ... and one up to 9 980
constexpr uint64_t kMaxBlocks = 1024;
constexpr uint32_t kNoSample = 0xffffffffu, kNoTaxon = 0xffffffffu;

static_assert(sizeof(epik_amd_taxa_totals) == kTotals * sizeof(uint64_t));
static_assert(sizeof(epik_amd_taxon_record) == 16 && sizeof(epik_amd_placement) == 16);

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ inline void add64(uint64_t *cell, uint64_t v)
{
    atomicAdd(reinterpret_cast<unsigned long long *>(cell), (unsigned long long)v);
}

__device__ inline uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_down((unsigned long long)v, d);
    return v;  // (lane 0 holds the sum)
}

// mass * 2^30 >= tau_q * total, as 128-bit integers
__device__ inline bool qualifies(uint64_t mass, uint32_t tau_q, uint64_t total)
{
    const uint64_t l_hi = mass >> (64 - kLwrBits), l_lo = mass << kLwrBits;
    const uint64_t r_hi = __umul64hi((uint64_t)tau_q, total), r_lo = (uint64_t)tau_q * total;
    return l_hi > r_hi || (l_hi == r_hi && l_lo >= r_lo);
}

template <bool LDS>
__global__ __launch_bounds__(kBlock) void taxa_kernel(TreeView taxa, const uint32_t *__restrict__ label, uint32_t num_branches,
                                                      const u32x4 *__restrict__ rows, const uint32_t *__restrict__ n_rows,
                                                      const uint32_t *__restrict__ kmer_counts,
                                                      const uint32_t *__restrict__ weights, const uint32_t *__restrict__ samples,
                                                      uint64_t n, uint32_t keep, uint32_t group, uint32_t tau_q,
                                                      uint32_t num_samples, uint64_t *__restrict__ g_cells,
                                                      u32x4 *__restrict__ records)
{
    extern __shared__ uint64_t lds_cells[];  // LDS: direct[T] | assigned[T] of the current sample
    __shared__ uint64_t s_q[kBlock];         // per group: q of the rows, by ascending taxon
    __shared__ uint32_t s_sorted[kBlock];    // ... the taxa
    __shared__ uint64_t block_totals[kTotals + 1];  // the current sample's totals, and the workgroup's bad_samples
    const uint32_t T = taxa.n, cells = 2 * T;
    const uint64_t stride = (uint64_t)cells + kTotals;
    if (LDS)
        for (uint32_t c = threadIdx.x; c < cells; c += kBlock) lds_cells[c] = 0;
    if (threadIdx.x <= kTotals) block_totals[threadIdx.x] = 0;
    __syncthreads();

    uint64_t tot[kTotals] = {0, 0, 0, 0, 0, 0};  // of the current sample, this lane's
    uint64_t bad_samples = 0;
    uint32_t cur = kNoSample;  // (the same in every lane of the workgroup)

    // the current sample's LDS cells and totals go to its row; every lane of the workgroup comes here together
    const auto flush = [&]() {
        __syncthreads();  // (the adds of the tiles so far)
#pragma unroll
        for (uint32_t k = 0; k < kTotals; ++k) {
            const uint64_t sum = wave_sum(tot[k]);
            if (threadIdx.x % kWave == 0 && sum) add64(&block_totals[k], sum);
            tot[k] = 0;
        }
        __syncthreads();
        if (cur != kNoSample) {
            uint64_t *row = g_cells + cur * stride;
            if (LDS)
                for (uint32_t c = threadIdx.x; c < cells; c += kBlock)
                    if (const uint64_t v = lds_cells[c]) {
                        add64(&row[c], v);
                        lds_cells[c] = 0;
                    }
            if (threadIdx.x < kTotals)
                if (const uint64_t v = block_totals[threadIdx.x]) {
                    add64(&row[cells + threadIdx.x], v);
                    block_totals[threadIdx.x] = 0;
                }
        }
        __syncthreads();
    };

    const int P = (int)group;
    const uint32_t j = threadIdx.x & (group - 1), base = threadIdx.x - j;  // my row; my group's first cell in LDS
    const uint32_t lane = threadIdx.x % kWave;
    const unsigned long long gmask = (group == kWave ? ~0ull : ((1ull << group) - 1)) << (lane - j);
    const uint64_t per_block = kBlock / group, tiles = (n + per_block - 1) / per_block;
    const uint64_t per = (tiles + gridDim.x - 1) / gridDim.x, t_begin = blockIdx.x * per, t_end = t_begin + per < tiles ? t_begin + per : tiles;
    for (uint64_t t = t_begin; t < t_end; ++t) {
        const uint64_t read0 = t * per_block;  // (< n: t < tiles)
        const uint32_t lead = samples ? __builtin_amdgcn_readfirstlane(samples[read0]) : 0u;  // (one address: uniform)
        if (lead < num_samples && lead != cur) {
            flush();
            cur = lead;
        }
        const uint64_t i = read0 + threadIdx.x / group;
        const bool live = i < n;
        u32x4 row = {0, 0, 0, 0};
        uint32_t raw_nr = 0, hits = 0, smp = 0, w = 0;
        if (live && j < keep) row = rows[i * keep + j];
        if (live) raw_nr = n_rows[i], hits = kmer_counts[i * keep], smp = samples ? samples[i] : 0u, w = weights ? weights[i] : 1u;
        uint32_t cls = 0;
        if (raw_nr == EPIK_AMD_ROWS_COUNTS_TOO_NARROW)
            cls = EPIK_AMD_TAXON_TOO_NARROW;
        else if (raw_nr == 0)
            cls = EPIK_AMD_TAXON_TOO_SHORT;
        else if (hits == 0)
            cls = EPIK_AMD_TAXON_NO_HIT;
        uint32_t nr = cls ? 0u : std::min(raw_nr, keep);
        if ((__ballot(j < nr && row.x >= num_branches) & gmask) != 0) cls = EPIK_AMD_TAXON_BAD_ROW, nr = 0;
        const bool mine = j < nr;  // a row the rule looks at (its branch is < N)
        const uint32_t tx = mine ? label[row.x] : kNoTaxon;
        const double lwr = mine ? __hiloint2double((int)row.w, (int)row.z) : 0.0;
        const uint64_t q = mine ? (uint64_t)__double2ll_rn(lwr * (double)(1u << kLwrBits)) : 0ull;
        unsigned long long total = q;
        for (int d = P / 2; d > 0; d >>= 1) total += __shfl_xor(total, d, P);
        if (!cls && total == 0) cls = EPIK_AMD_TAXON_NO_MASS;  // (lanes past n: cls is TOO_SHORT already)
        const uint32_t t0 = __shfl(tx, 0, P);

        // rank of my taxon among the group's (ties by row; the idle lanes keep their own cells behind)
        uint32_t rank = mine ? 0u : j;
        for (int l = 0; l < P; ++l) {
            const uint32_t other = __shfl(tx, l, P);
            if (mine && (uint32_t)l < nr && (other < tx || (other == tx && (uint32_t)l < j))) ++rank;
        }
        __syncthreads();  // (the cells of the tile before)
        s_sorted[base + rank] = tx;
        s_q[base + rank] = q;
        __syncthreads();
        const uint32_t here = s_sorted[base + j];  // kNoTaxon from nr on
        const uint32_t next = s_sorted[base + std::min(j + 1, group - 1)];
        const bool has_here = j < nr, has_adj = j + 1 < nr;
        const uint32_t adj = has_adj ? tree_lca(taxa, here, next) : kNoTaxon;
        const uint32_t first_here = has_here ? taxa.first[here] : 0u, first_adj = has_adj ? taxa.first[adj] : 0u;
        const bool run_first = has_here && (j == 0 || s_sorted[base + j - 1] != here);
        uint64_t mass_here = 0, mass_adj = 0, run = 0;
        for (int l = 0; l < P; ++l) {  // (one address a group: broadcasts; idle cells hold kNoTaxon and 0)
            const uint32_t tl = s_sorted[base + l];
            const uint64_t ql = s_q[base + l];
            mass_here += (first_here <= tl && tl <= here) ? ql : 0ull;
            mass_adj += (has_adj && first_adj <= tl && tl <= adj) ? ql : 0ull;
            run += tl == here ? ql : 0ull;
        }
        const bool ok_here = has_here && !cls && qualifies(mass_here, tau_q, total);
        const bool ok_adj = has_adj && !cls && qualifies(mass_adj, tau_q, total);
        uint32_t mine_best = std::min(ok_here ? here : kNoTaxon, ok_adj ? adj : kNoTaxon);
        uint32_t best = mine_best;
        for (int d = P / 2; d > 0; d >>= 1) best = std::min(best, (uint32_t)__shfl_xor(best, d, P));
        // the mass of the winner, from the first lane that weighed it (placed reads: the lca of all rows always qualifies)
        const unsigned long long holders = __ballot(!cls && live && mine_best == best) & gmask;
        const uint64_t my_mass = (ok_here && here == best) ? mass_here : mass_adj;
        const int src = holders ? __ffsll((long long)holders) - 1 : (int)lane;
        const uint64_t best_mass = __shfl((unsigned long long)my_mass, src);

        if (live && j == 0 && records) {
            u32x4 rec = {cls, 0u, 0u, 0u};
            if (!cls) {
                rec.x = best;
                rec.y = best_mass > 0xffffffffull ? 0xffffffffu : (uint32_t)best_mass;
                rec.z = t0;
                rec.w = total > 0xffffffffull ? 0xffffffffu : (uint32_t)total;
            }
            records[i] = rec;
        }

        // the cells
        const bool in_sample = live && smp < num_samples, own = in_sample && smp == cur;
        uint64_t *g_row = g_cells + (in_sample ? smp : 0u) * stride;
        if (live && j == 0) {
            if (!in_sample) {
                ++bad_samples;
            } else {
                const uint32_t k = !cls ? 0u : cls == EPIK_AMD_TAXON_NO_HIT ? 1u : cls == EPIK_AMD_TAXON_TOO_SHORT ? 2u
                                   : cls == EPIK_AMD_TAXON_TOO_NARROW ? 3u : cls == EPIK_AMD_TAXON_NO_MASS ? 4u : 5u;
                const uint64_t v = k == 5 ? 1u : w;
                if (own) {
#pragma unroll
                    for (uint32_t c = 0; c < kTotals; ++c) tot[c] += c == k ? v : 0u;
                } else if (v) {
                    add64(&g_row[cells + k], v);
                }
                if (!cls && w) {
                    if (LDS && own)
                        add64(&lds_cells[T + best], w);
                    else
                        add64(&g_row[T + best], w);
                }
            }
        }
        if (in_sample && !cls && run_first && w && run) {
            if (LDS && own)  // (ds_add_u64)
                add64(&lds_cells[here], (uint64_t)w * run);
            else
                add64(&g_row[here], (uint64_t)w * run);
        }
    }
    flush();
    const uint64_t bad = wave_sum(bad_samples);
    if (threadIdx.x % kWave == 0 && bad) add64(&block_totals[kTotals], bad);
    __syncthreads();
    if (threadIdx.x == 0 && block_totals[kTotals]) add64(&g_cells[num_samples * stride], block_totals[kTotals]);
}

// dst[c] += src[c]: the cells of another device's object, uploaded (add_cells)
__global__ __launch_bounds__(kBlock) void taxa_merge_kernel(uint64_t *__restrict__ dst, const uint64_t *__restrict__ src, uint64_t count)
{
    for (uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x; c < count; c += (uint64_t)gridDim.x * kBlock) dst[c] += src[c];
}

uint64_t row_stride(const epik_amd_taxonomy *tx) { return 2ull * tx->num_taxa + kTotals; }
uint64_t cell_count(const epik_amd_taxonomy *tx) { return tx->num_samples * row_stride(tx) + 1; }

int check_tau(uint32_t tau_q)
{
    if (tau_q <= (1u << (kLwrBits - 1)) || tau_q > (1u << kLwrBits))
        return fail_with(EPIK_AMD_ERR_INVALID, "tau_q must lie in (2^29, 2^30]: more than half of the mass, at most all of it");
    return EPIK_AMD_OK;
}

// the taxonomy's tables (the tree's, with branch lengths of zero) and the labels: validated; "branch" reads "taxon"
int build_tables(const uint32_t *taxon_parent, uint32_t num_taxa, const uint32_t *label, uint32_t num_branches,
                 std::vector<uint8_t> &tables)
{
    if (num_taxa == 0) return fail_with(EPIK_AMD_ERR_INVALID, "a taxonomy has at least one taxon, the root (num_taxa is 0)");
    tables.resize(tree_table_bytes(num_taxa));
    const std::vector<double> zero(num_taxa, 0.0);
    std::string err;
    if (const int rc = tree_build(taxon_parent, zero.data(), num_taxa, tables.data(), err); rc != EPIK_AMD_OK) {
        if (err.rfind("branch ", 0) == 0) err = "taxon " + err.substr(7);
        for (size_t at; (at = err.find("last branch")) != std::string::npos;) err.replace(at, 11, "last taxon");
        return fail_with(rc, err);
    }
    for (uint32_t b = 0; b < num_branches; ++b)
        if (label[b] >= num_taxa)
            return fail_with(EPIK_AMD_ERR_INVALID, "branch " + std::to_string(b) + ": its label " + std::to_string(label[b]) +
                                                       " is no taxon (num_taxa is " + std::to_string(num_taxa) + ")");
    return EPIK_AMD_OK;
}

int add_device_impl(epik_amd_taxonomy *tx, const void *d_rows, const void *d_n_rows, const void *d_kmer_counts,
                    const void *d_weights, const void *d_samples, uint64_t n, uint32_t tau_q, void *d_records, void *stream);

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

void free_taxonomy(epik_amd_taxonomy *tx)
{
    (void)hipFree(tx->d_tables), (void)hipFree(tx->d_label), (void)hipFree(tx->d_cells);
}

}  // namespace

extern "C" {

int epik_amd_taxonomy_create(const epik_amd_placer *p, const uint32_t *taxon_parent, uint32_t num_taxa, const uint32_t *label,
                             uint32_t num_samples, epik_amd_taxonomy **out)
{
    try {
        if (!out) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
        *out = nullptr;
        if (!p) return fail_with(EPIK_AMD_ERR_INVALID, "null placer");
        if (!taxon_parent || !label) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
        if (num_samples == 0) return fail_with(EPIK_AMD_ERR_INVALID, "a taxonomy object has at least one sample (num_samples is 0)");
        if (p->plan.shard_count > 1)
            return fail_with(EPIK_AMD_ERR_INVALID, "taxonomic assignment needs a whole database, not a k-mer-space shard");
        std::vector<uint8_t> tables;
        if (const int rc = build_tables(taxon_parent, num_taxa, label, p->params.num_branches, tables); rc != EPIK_AMD_OK) return rc;
        auto *tx = new (std::nothrow) epik_amd_taxonomy;
        if (!tx) return fail_with(EPIK_AMD_ERR_INVALID, "out of memory");
        tx->device = p->device;
        tx->num_taxa = num_taxa, tx->num_samples = num_samples;
        tx->num_branches = p->params.num_branches, tx->keep = p->params.keep_at_most;
        tx->max_blocks_cap = p->max_blocks_cap;
        const uint64_t lds_bytes = 2 * sizeof(uint64_t) * (uint64_t)num_taxa;
        tx->lds = lds_bytes <= kLdsLimit;
        // EPIK_AMD_PROFILE_LDS=0|1 (tests), as for a profile: the global or the LDS path whatever the taxonomy
        if (const char *e = std::getenv("EPIK_AMD_PROFILE_LDS")) {
            if (std::strcmp(e, "0") == 0)
                tx->lds = false;
            else if (std::strcmp(e, "1") == 0 && !tx->lds) {
                delete tx;
                return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "EPIK_AMD_PROFILE_LDS=1: the cells of this taxonomy do not fit the LDS path");
            }
        }
        const size_t bytes = cell_count(tx) * sizeof(uint64_t);
        hipError_t e = hipSetDevice(tx->device);
        tx->lds_blocks = kMaxBlocks;
        if (e == hipSuccess && tx->lds && lds_bytes > kLdsBudget) {
            int cus = 0;
            e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, tx->device);
            tx->lds_blocks = (uint32_t)std::max(1, cus);
            if (e == hipSuccess)
                e = hipFuncSetAttribute(reinterpret_cast<const void *>(&taxa_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)(kLdsLimit));
        }
        if (e == hipSuccess) e = hipMalloc(&tx->d_tables, tables.size());
        if (e == hipSuccess) e = hipMemcpy(tx->d_tables, tables.data(), tables.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&tx->d_label), std::max<size_t>(1, tx->num_branches) * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemcpy(tx->d_label, label, (size_t)tx->num_branches * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&tx->d_cells), bytes);
        if (e == hipSuccess) e = hipMemset(tx->d_cells, 0, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            free_taxonomy(tx);
            delete tx;
            return fail_with(EPIK_AMD_ERR_HIP, std::string("epik_amd_taxonomy_create: ") + hipGetErrorString(e));
        }
        tx->view = tree_view(tx->d_tables, num_taxa, tree_levels(num_taxa));
        *out = tx;
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("taxonomy_create: ") + e.what());
    }
}

void epik_amd_taxonomy_destroy(epik_amd_taxonomy *tx)
{
    if (!tx) return;
    if (hipSetDevice(tx->device) == hipSuccess) {
        (void)hipDeviceSynchronize();
        free_taxonomy(tx);
    }
    delete tx;
}

int epik_amd_taxonomy_reset(epik_amd_taxonomy *tx)
{
    if (!tx) return fail_with(EPIK_AMD_ERR_INVALID, "null taxonomy");
    HIP_TRY(hipSetDevice(tx->device));
    HIP_TRY(hipDeviceSynchronize());  // (the adds enqueued so far, on whatever stream)
    HIP_TRY(hipMemset(tx->d_cells, 0, cell_count(tx) * sizeof(uint64_t)));
    HIP_TRY(hipDeviceSynchronize());
    return EPIK_AMD_OK;
}

int epik_amd_taxonomy_info(const epik_amd_taxonomy *tx, uint32_t *num_taxa, uint32_t *num_samples, uint32_t *num_branches,
                           uint32_t *lds_path)
{
    if (!tx) return fail_with(EPIK_AMD_ERR_INVALID, "null taxonomy");
    if (num_taxa) *num_taxa = tx->num_taxa;
    if (num_samples) *num_samples = tx->num_samples;
    if (num_branches) *num_branches = tx->num_branches;
    if (lds_path) *lds_path = tx->lds ? 1 : 0;
    return EPIK_AMD_OK;
}

int epik_amd_taxonomy_read(epik_amd_taxonomy *tx, uint64_t *direct, uint64_t *assigned, epik_amd_taxa_totals *totals,
                           uint64_t *bad_samples)
{
    if (!tx) return fail_with(EPIK_AMD_ERR_INVALID, "null taxonomy");
    HIP_TRY(hipSetDevice(tx->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t T = tx->num_taxa, S = tx->num_samples, pitch = row_stride(tx) * sizeof(uint64_t), row = T * sizeof(uint64_t);
    if (direct) HIP_TRY(hipMemcpy2D(direct, row, tx->d_cells, pitch, row, S, hipMemcpyDeviceToHost));
    if (assigned) HIP_TRY(hipMemcpy2D(assigned, row, tx->d_cells + T, pitch, row, S, hipMemcpyDeviceToHost));
    if (totals) HIP_TRY(hipMemcpy2D(totals, sizeof *totals, tx->d_cells + 2 * T, pitch, sizeof *totals, S, hipMemcpyDeviceToHost));
    if (bad_samples) HIP_TRY(hipMemcpy(bad_samples, tx->d_cells + S * row_stride(tx), sizeof *bad_samples, hipMemcpyDeviceToHost));
    return EPIK_AMD_OK;
}

int epik_amd_taxonomy_add_cells(epik_amd_taxonomy *tx, const uint64_t *direct, const uint64_t *assigned,
                                const epik_amd_taxa_totals *totals)
{
    try {
        if (!tx) return fail_with(EPIK_AMD_ERR_INVALID, "null taxonomy");
        const size_t T = tx->num_taxa, S = tx->num_samples, stride = row_stride(tx);
        std::vector<uint64_t> cells(S * stride, 0);
        for (size_t s = 0; s < S; ++s) {
            if (direct) std::memcpy(&cells[s * stride], direct + s * T, T * sizeof(uint64_t));
            if (assigned) std::memcpy(&cells[s * stride + T], assigned + s * T, T * sizeof(uint64_t));
            if (totals) std::memcpy(&cells[s * stride + 2 * T], totals + s, sizeof *totals);
        }
        HIP_TRY(hipSetDevice(tx->device));
        struct Upload {
            void *d = nullptr;
            ~Upload()
            {
                if (d) (void)hipDeviceSynchronize(), (void)hipFree(d);
            }
        } up;
        HIP_TRY(hipMalloc(&up.d, cells.size() * sizeof(uint64_t)));
        HIP_TRY(hipMemcpy(up.d, cells.data(), cells.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIP_TRY(hipDeviceSynchronize());  // (the adds enqueued so far: this one is no atomic)
        const uint64_t blocks = std::min<uint64_t>((cells.size() + kBlock - 1) / kBlock, tx->max_blocks_cap ? tx->max_blocks_cap : kMaxBlocks);
        hipLaunchKernelGGL(taxa_merge_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, nullptr, tx->d_cells,
                           static_cast<const uint64_t *>(up.d), (uint64_t)cells.size());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("taxonomy_add_cells: ") + e.what());
    }
}

int epik_amd_taxonomy_add_device(epik_amd_taxonomy *tx, const void *d_rows, const void *d_n_rows, const void *d_kmer_counts,
                                 const void *d_weights, const void *d_samples, uint64_t n, uint32_t tau_q, void *d_records,
                                 void *stream)
{
    return add_device_impl(tx, d_rows, d_n_rows, d_kmer_counts, d_weights, d_samples, n, tau_q, d_records, stream);
}

int epik_amd_placer_taxa_reads(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                               epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts, epik_amd_taxonomy *taxonomy,
                               uint32_t tau_q, epik_amd_taxon_record *records, const uint32_t *weights, const uint32_t *samples,
                               epik_amd_profile *profile, epik_amd_cohort *cohort)
{
    try {  // std::vector: nothing may leave through the C ABI
        if (!p) return fail_with(EPIK_AMD_ERR_INVALID, "null placer");
        if (n == 0) return EPIK_AMD_OK;
        uint64_t longest = 0;
        if (const int rc = check_host_reads(seqs, seq_offsets, n, longest); rc != EPIK_AMD_OK) return rc;
        return taxa_host_chunked(p, TaxaRequest{taxonomy, tau_q, records, weights, samples, profile, cohort}, seqs, seq_offsets, n,
                                 0, longest, kForwardHost, rows, n_rows, kmer_counts, nullptr);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("taxa_reads: ") + e.what());
    }
}

}  // extern "C"

namespace {

int add_device_impl(epik_amd_taxonomy *tx, const void *d_rows, const void *d_n_rows, const void *d_kmer_counts,
                    const void *d_weights, const void *d_samples, uint64_t n, uint32_t tau_q, void *d_records, void *stream)
{
    if (!tx) return fail_with(EPIK_AMD_ERR_INVALID, "null taxonomy");
    if (const int rc = check_tau(tau_q); rc != EPIK_AMD_OK) return rc;
    if (n == 0) return EPIK_AMD_OK;
    if (!d_rows || !d_n_rows || !d_kmer_counts)
        return fail_with(EPIK_AMD_ERR_INVALID, "null device buffer (the k-mer counts are required: they tell a read without hits)");
    if (n > 0xffffffffull) return fail_with(EPIK_AMD_ERR_INVALID, "a batch of 2^32 reads or more");
    HIP_TRY(hipSetDevice(tx->device));
    uint32_t group = 1;
    while (group < tx->keep) group *= 2;
    const uint64_t per_block = kBlock / group, tiles = (n + per_block - 1) / per_block;
    const uint64_t own_blocks = tx->lds ? tx->lds_blocks : kMaxBlocks;
    const uint64_t max_blocks = tx->max_blocks_cap ? std::min<uint64_t>(own_blocks, tx->max_blocks_cap) : own_blocks;
    const dim3 grid((uint32_t)std::max<uint64_t>(1, std::min(tiles, max_blocks)));
    const auto *rows = static_cast<const u32x4 *>(d_rows);
    const auto *n_rows = static_cast<const uint32_t *>(d_n_rows), *counts = static_cast<const uint32_t *>(d_kmer_counts);
    const auto *weights = static_cast<const uint32_t *>(d_weights), *samples = static_cast<const uint32_t *>(d_samples);
    auto *records = static_cast<u32x4 *>(d_records);
    const auto s = static_cast<hipStream_t>(stream);
    if (tx->lds)
        hipLaunchKernelGGL(taxa_kernel<true>, grid, dim3(kBlock), 2 * sizeof(uint64_t) * tx->num_taxa, s, tx->view, tx->d_label,
                           tx->num_branches, rows, n_rows, counts, weights, samples, n, tx->keep, group, tau_q, tx->num_samples,
                           tx->d_cells, records);
    else
        hipLaunchKernelGGL(taxa_kernel<false>, grid, dim3(kBlock), 0, s, tx->view, tx->d_label, tx->num_branches, rows, n_rows,
                           counts, weights, samples, n, tx->keep, group, tau_q, tx->num_samples, tx->d_cells, records);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

// what the sink of a placement with taxonomic assignment carries from chunk to chunk
struct TaxaSink {
    TaxaRequest req;
    epik_amd_taxon_record *d_records;   // [n] of the whole batch on the device, or null
    const uint32_t *d_weights, *d_samples;  // [n] on the device, or null
};

int taxa_chunk(void *ctx, const epik_amd_placement *d_rows, const uint32_t *d_n_rows, const uint32_t *d_counts, uint64_t first,
               uint64_t count, hipStream_t stream)
{
    const auto *sink = static_cast<const TaxaSink *>(ctx);
    const uint32_t *w = sink->d_weights ? sink->d_weights + first : nullptr, *smp = sink->d_samples ? sink->d_samples + first : nullptr;
    if (const int rc = add_device_impl(sink->req.taxonomy, d_rows, d_n_rows, d_counts, w, smp, count, sink->req.tau_q,
                                       sink->d_records ? sink->d_records + first : nullptr, stream);
        rc != EPIK_AMD_OK)
        return rc;
    if (sink->d_records)
        HIP_TRY(hipMemcpyAsync(sink->req.records + first, sink->d_records + first, count * sizeof(epik_amd_taxon_record),
                               hipMemcpyDeviceToHost, stream));
    if (sink->req.profile) return epik_amd_profile_add_device(sink->req.profile, d_rows, d_n_rows, d_counts, w, count, stream);
    if (sink->req.cohort) return epik_amd_cohort_add_device(sink->req.cohort, d_rows, d_n_rows, d_counts, w, smp, count, stream);
    return EPIK_AMD_OK;
}

}  // namespace

namespace epik_amd {

int taxa_host_chunked(epik_amd_placer *p, const TaxaRequest &req, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                      uint32_t mode, uint64_t longest_placed, const HostVariant &v, epik_amd_placement *rows, uint32_t *n_rows,
                      uint32_t *kmer_counts, uint8_t *label)
{
    if (!p) return fail_with(EPIK_AMD_ERR_INVALID, "null placer");
    const epik_amd_taxonomy *tx = req.taxonomy;
    if (!tx) return fail_with(EPIK_AMD_ERR_INVALID, "null taxonomy");
    if (const int rc = check_tau(req.tau_q); rc != EPIK_AMD_OK) return rc;
    if (tx->device != p->device || tx->num_branches != p->params.num_branches || tx->keep != p->params.keep_at_most)
        return fail_with(EPIK_AMD_ERR_INVALID, "the taxonomy was created for another placer (device, num_branches or keep_at_most differ)");
    if (p->plan.shard_count > 1)
        return fail_with(EPIK_AMD_ERR_INVALID, "taxonomic assignment needs a whole database, not a k-mer-space shard");
    if (req.profile && req.cohort) return fail_with(EPIK_AMD_ERR_INVALID, "a profile or a cohort may be chained, not both");
    if (req.profile)
        if (const int rc = check_profile_pair(p, req.profile); rc != EPIK_AMD_OK) return rc;
    if (req.cohort) {
        const epik_amd_cohort *c = req.cohort;
        if (c->device != p->device || c->num_branches != p->params.num_branches || c->keep != p->params.keep_at_most)
            return fail_with(EPIK_AMD_ERR_INVALID, "the cohort was created for another placer (device, num_branches or keep_at_most differ)");
        if (!req.samples) return fail_with(EPIK_AMD_ERR_INVALID, "null samples (a cohort placement names the sample of every read)");
    }
    HIP_TRY(hipSetDevice(p->device));
    struct DeviceArrays {  // (freed however the call ends; place_host_chunked has drained the stream by then, or never used it)
        void *records = nullptr, *weights = nullptr, *samples = nullptr;
        hipStream_t stream = nullptr;
        ~DeviceArrays()
        {
            if (records || weights || samples) (void)hipStreamSynchronize(stream);
            if (records) (void)hipFree(records);
            if (weights) (void)hipFree(weights);
            if (samples) (void)hipFree(samples);
        }
    } d;
    d.stream = p->stream;
    if (req.records) HIP_TRY(hipMalloc(&d.records, n * sizeof(epik_amd_taxon_record)));
    if (req.weights) {
        HIP_TRY(hipMalloc(&d.weights, n * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(d.weights, req.weights, n * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    }
    if (req.samples) {
        HIP_TRY(hipMalloc(&d.samples, n * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(d.samples, req.samples, n * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    }
    TaxaSink ctx{req, static_cast<epik_amd_taxon_record *>(d.records), static_cast<const uint32_t *>(d.weights),
                 static_cast<const uint32_t *>(d.samples)};
    const ChunkSink sink{taxa_chunk, &ctx};
    return place_host_chunked(p, seqs, seq_offsets, n, mode, longest_placed, v, rows, n_rows, kmer_counts, label, &sink);
}

}  // namespace epik_amd

extern "C" {

int epik_amd_taxonomy_assign_host(const uint32_t *taxon_parent, uint32_t num_taxa, const uint32_t *label, uint32_t num_branches,
                                  uint32_t keep, const epik_amd_placement *rows, const uint32_t *n_rows,
                                  const uint32_t *kmer_counts, const uint32_t *weights, const uint32_t *samples, uint64_t n,
                                  uint32_t num_samples, uint32_t tau_q, epik_amd_taxon_record *records, uint64_t *direct,
                                  uint64_t *assigned, epik_amd_taxa_totals *totals, uint64_t *bad_samples)
{
    try {
        if (!taxon_parent || !label) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
        if (const int rc = check_tau(tau_q); rc != EPIK_AMD_OK) return rc;
        if (keep == 0 || keep > kWave) return fail_with(EPIK_AMD_ERR_INVALID, "keep must be in [1, 64]");
        const bool with_cells = direct || assigned || totals || bad_samples;
        if (with_cells && !(direct && assigned && totals && bad_samples))
            return fail_with(EPIK_AMD_ERR_INVALID, "null argument (the cells come all four, or none of them)");
        if (with_cells && num_samples == 0) return fail_with(EPIK_AMD_ERR_INVALID, "a taxonomy object has at least one sample (num_samples is 0)");
        std::vector<uint8_t> tables;
        if (const int rc = build_tables(taxon_parent, num_taxa, label, num_branches, tables); rc != EPIK_AMD_OK) return rc;
        if (n == 0) return EPIK_AMD_OK;
        if (!rows || !n_rows || !kmer_counts) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
        taxa_cells cells(with_cells ? num_samples : 0, num_taxa);
        taxa_assign(taxon_parent, num_taxa, label, num_branches, keep, rows, n_rows, kmer_counts, weights, samples, n,
                    tau_q, records, with_cells ? &cells : nullptr);
        if (with_cells) {
            for (size_t c = 0; c < cells.direct.size(); ++c) direct[c] += cells.direct[c], assigned[c] += cells.assigned[c];
            for (uint32_t s = 0; s < num_samples; ++s) {
                totals[s].placed += cells.totals[s].placed, totals[s].no_hit += cells.totals[s].no_hit;
                totals[s].too_short += cells.totals[s].too_short, totals[s].too_narrow += cells.totals[s].too_narrow;
                totals[s].no_mass += cells.totals[s].no_mass, totals[s].bad_reads += cells.totals[s].bad_reads;
            }
            *bad_samples += cells.bad_samples;
        }
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("taxonomy_assign_host: ") + e.what());
    }
}

}  // extern "C"
