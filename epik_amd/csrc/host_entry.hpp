// host_entry.hpp -- the host side shared by the placements around epik_amd_placer_place_device: the synchronous
// host-buffer entry points of strand_place.hip, frame_place.hip and mates_place.hip are place_host_chunked over a
// HostVariant each, and their profile-only twins (profile_place.hip: profile_host_chunked) the same with a sink per
// chunk and nothing copied out; shard_place.hip takes the HIP-error macro and the batch check; the complement on
// character classes serves strand_place.hip and mates_place.hip.  Internal to libepik_amd.
#ifndef EPIK_AMD_HOST_ENTRY_HPP
#define EPIK_AMD_HOST_ENTRY_HPP
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "placer_impl.hpp"

#define HIP_TRY(expr)                                                                                            \
    do {                                                                                                         \
        const hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return epik_amd::fail_with(EPIK_AMD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

namespace epik_amd {

// the kernels around the placement run workgroups of four waves
constexpr uint32_t kWave = 64, kBlockWaves = 4, kBlock = kWave * kBlockWaves;

inline uint64_t align_up(uint64_t x) { return (x + 255) / 256 * 256; }
__host__ __device__ inline uint32_t bitrev4(uint32_t c) { return (c & 1u) << 3 | (c & 2u) << 1 | (c & 4u) >> 1 | (c & 8u) >> 3; }
__host__ __device__ inline bool has_rows(uint32_t n_rows) { return n_rows != 0 && n_rows != EPIK_AMD_ROWS_COUNTS_TOO_NARROW; }

// workgroups for `units` waves of work: at least one, at most max_blocks (the kernels stride over the rest)
inline uint32_t grid_for(uint64_t units, uint64_t max_blocks)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((units + kBlockWaves - 1) / kBlockWaves, max_blocks));
}

// The checks epik_amd_placer_place makes of a host batch of n >= 1 reads, in its order and words; `longest` gets the
// batch's longest read.
inline int check_host_reads(const char *seqs, const uint64_t *seq_offsets, uint64_t n, uint64_t &longest);
inline int check_host_batch(const char *seqs, const uint64_t *seq_offsets, uint64_t n, const void *rows,
                            const void *n_rows, uint64_t &longest)
{
    if (!seqs || !seq_offsets || !rows || !n_rows) return fail_with(EPIK_AMD_ERR_INVALID, "null host buffer");
    return check_host_reads(seqs, seq_offsets, n, longest);
}
// ... the part of it that looks at the reads alone (an entry point that takes no rows back)
inline int check_host_reads(const char *seqs, const uint64_t *seq_offsets, uint64_t n, uint64_t &longest)
{
    if (!seqs || !seq_offsets) return fail_with(EPIK_AMD_ERR_INVALID, "null host buffer");
    if (seq_offsets[0] != 0) return fail_with(EPIK_AMD_ERR_INVALID, "seq_offsets[0] must be 0");
    longest = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (seq_offsets[i + 1] < seq_offsets[i] || seq_offsets[i + 1] - seq_offsets[i] > 0xffffffffull)
            return fail_with(EPIK_AMD_ERR_INVALID, "seq_offsets not monotone, or a read of 2^32 characters or more");
        longest = std::max<uint64_t>(longest, seq_offsets[i + 1] - seq_offsets[i]);
    }
    return EPIK_AMD_OK;
}

// For every byte, a byte of the complemented class (by value in a kernel's arguments: no allocation)
struct ComplementMap {
    uint8_t byte[256];
};

// For every byte c, a byte whose class is bitrev4(char_class[c]) -- from the handle's own table
inline int complement_map(const epik_amd_placer *p, ComplementMap &map)
{
    if (p->h_char_class.size() != 256) return fail_with(EPIK_AMD_ERR_INVALID, "placer has no character table");
    int rep[16];
    std::fill(rep, rep + 16, -1);
    for (int c = 255; c >= 0; --c) {  // (the smallest byte of each class)
        const uint32_t cls = p->h_char_class[c];
        if (cls > 15) return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "character class outside the four nucleotide states");
        rep[cls] = c;
    }
    for (int c = 0; c < 256; ++c) {
        const uint32_t comp = bitrev4(p->h_char_class[c]);
        if (rep[comp] < 0)
            return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "the character table has no character of class " + std::to_string(comp) +
                                                           ", the complement of byte " + std::to_string(c) + "'s");
        map.byte[c] = (uint8_t)rep[comp];
    }
    return EPIK_AMD_OK;
}

// k-mers a sequence may have with counts of that width (capi.hip's rule: the top bit of 16- and 32-bit counts is a flag)
inline uint64_t max_kmers_of_counts(int counts) { return counts == kCounts8 ? 255u : counts == kCounts16 ? 32767u : 0x7fffffffull; }

// The count width of a host entry point, as epik_amd_placer_place chooses it, from the longest sequence the call
// places: epik_amd_placer_choose_counts, or a forced width kept unless it cannot hold that sequence's k-mers (no read
// comes back EPIK_AMD_ROWS_COUNTS_TOO_NARROW from a host entry point).  The handle's count state is restored when
// the guard goes, however the call ends.
struct CountWidthGuard {
    CountWidthGuard(epik_amd_placer *p_, uint64_t longest) : p(p_), counts(p_->counts), hint(p_->longest_read_hint)
    {
        if (!p->counts_forced) {
            rc = epik_amd_placer_choose_counts(p, longest);
            return;
        }
        const uint64_t k = p->params.kmer_size, kmers = longest >= k ? longest - k + 1 : 0;
        if (kmers > max_kmers_of_counts(p->counts)) p->counts = kmers > max_kmers_of_counts(kCounts16) ? kCounts32 : kCounts16;
        p->longest_read_hint = longest;
    }
    ~CountWidthGuard() { p->counts = counts, p->longest_read_hint = hint; }
    epik_amd_placer *p;
    int counts;
    uint64_t hint;
    int rc = EPIK_AMD_OK;  // of the choice
};

// What place_host_chunked needs of a placement around epik_amd_placer_place_device
struct HostVariant {
    uint64_t chunk_reads, chunk_bytes;  // the device budget per chunk
    const char *chunk_reads_env;        // overrides chunk_reads (tests: fewer reads per chunk)
    // its epik_amd_placer_*_workspace_bytes
    int (*workspace_bytes)(const epik_amd_placer *p, uint64_t n, uint64_t seq_bytes, uint32_t mode, uint64_t *bytes);
    // the bytes at the start of the workspace zeroed before each chunk is placed (nullptr: none)
    uint64_t (*zeroed_bytes)(const epik_amd_placer *p, uint64_t n, uint32_t mode);
    // its asynchronous device entry; d_label: a byte per read (strand, frame)
    int (*place_device)(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets, uint64_t n, uint32_t mode,
                        void *d_workspace, uint64_t workspace_bytes, void *d_rows, void *d_n_rows, void *d_kmer_counts,
                        void *d_label, hipStream_t stream);
    // offsets an item takes in seq_offsets: 1, a read; 2, a pair of mates (reads 2i and 2i + 1) -- n, the chunks, rows
    // and label bytes count items
    uint64_t item_reads = 1;
    // used instead of place_device when set: a device entry that is also told the characters of its batch
    int (*place_device_sized)(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets, uint64_t n, uint64_t seq_bytes,
                              uint32_t mode, void *d_workspace, uint64_t workspace_bytes, void *d_rows, void *d_n_rows,
                              void *d_kmer_counts, void *d_label, hipStream_t stream) = nullptr;
};

// What may look at every chunk of place_host_chunked while it is on the device: called once the chunk is placed,
// with its device rows, row counts and k-mer counts, the index of its first item in the batch and its number of items;
// whatever it enqueues goes on `stream`, the handle's, ahead of the copies out.
struct ChunkSink {
    int (*fn)(void *ctx, const epik_amd_placement *d_rows, const uint32_t *d_n_rows, const uint32_t *d_kmer_counts,
              uint64_t first, uint64_t count, hipStream_t stream);
    void *ctx;
};

// The synchronous host-buffer entry point of a variant, once the caller has checked the handle, the mode and the
// batch (n >= 1, check_host_batch): the count width for `longest_placed`, the longest sequence the device entry
// places; then the batch in chunks through one device allocation, each copied in, placed on the handle's stream,
// copied out and waited for.  rows, n_rows and kmer_counts may be NULL, each by itself: that part stays on the device
// (with a sink and all three NULL nothing but the label bytes crosses back).
inline int place_host_chunked(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                              uint32_t mode, uint64_t longest_placed, const HostVariant &v, epik_amd_placement *rows,
                              uint32_t *n_rows, uint32_t *kmer_counts, uint8_t *label, const ChunkSink *sink = nullptr)
{
    HIP_TRY(hipSetDevice(p->device));
    const CountWidthGuard width(p, longest_placed);
    if (width.rc != EPIK_AMD_OK) return width.rc;

    // chunks of at most chunk_reads items and chunk_bytes characters (a longer item: a chunk of its own)
    const uint64_t s = v.item_reads;
    uint64_t chunk_reads = v.chunk_reads;
    if (const char *e = std::getenv(v.chunk_reads_env)) chunk_reads = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
    std::vector<uint64_t> starts{0};
    uint64_t max_reads = 0, max_bytes = 0;
    for (uint64_t r0 = 0; r0 < n;) {
        uint64_t r1 = r0 + 1;
        while (r1 < n && r1 - r0 < chunk_reads && seq_offsets[s * (r1 + 1)] - seq_offsets[s * r0] <= v.chunk_bytes) ++r1;
        max_reads = std::max(max_reads, r1 - r0);
        max_bytes = std::max(max_bytes, seq_offsets[s * r1] - seq_offsets[s * r0]);
        starts.push_back(r0 = r1);
    }
    const uint64_t keep = p->params.keep_at_most;
    uint64_t ws_bytes = 0;
    if (const int rc = v.workspace_bytes(p, max_reads, max_bytes, mode, &ws_bytes); rc != EPIK_AMD_OK) return rc;
    // one allocation: seqs | offsets | rows | n_rows | counts | label | workspace
    const uint64_t o_offs = align_up(max_bytes + 1), o_rows = o_offs + align_up((s * max_reads + 1) * sizeof(uint64_t));
    const uint64_t o_nrows = o_rows + align_up(max_reads * keep * sizeof(epik_amd_placement));
    const uint64_t o_counts = o_nrows + align_up(max_reads * sizeof(uint32_t));
    const uint64_t o_label = o_counts + align_up(max_reads * keep * sizeof(uint32_t));
    const uint64_t o_ws = o_label + align_up(max_reads);
    struct ChunkBuffers {  // (freed however the call ends, after its stream has drained)
        void *base = nullptr;
        hipStream_t stream = nullptr;
        ~ChunkBuffers()
        {
            if (stream) (void)hipStreamSynchronize(stream);
            if (base) (void)hipFree(base);
        }
    } buf;
    HIP_TRY(hipMalloc(&buf.base, o_ws + ws_bytes));
    buf.stream = p->stream;
    uint8_t *d = static_cast<uint8_t *>(buf.base);
    auto *d_offs = reinterpret_cast<uint64_t *>(d + o_offs);
    auto *d_rows = reinterpret_cast<epik_amd_placement *>(d + o_rows);
    auto *d_nrows = reinterpret_cast<uint32_t *>(d + o_nrows);
    auto *d_counts = reinterpret_cast<uint32_t *>(d + o_counts);
    uint8_t *d_label = d + o_label, *d_ws = ws_bytes ? d + o_ws : nullptr;
    std::vector<uint64_t> offs(s * max_reads + 1);
    for (size_t c = 0; c + 1 < starts.size(); ++c) {
        const uint64_t r0 = starts[c], cnt = starts[c + 1] - r0, b0 = seq_offsets[s * r0], bytes = seq_offsets[s * (r0 + cnt)] - b0;
        for (uint64_t i = 0; i <= s * cnt; ++i) offs[i] = seq_offsets[s * r0 + i] - b0;
        if (bytes) HIP_TRY(hipMemcpyAsync(d, seqs + b0, bytes, hipMemcpyHostToDevice, p->stream));
        HIP_TRY(hipMemcpyAsync(d_offs, offs.data(), (s * cnt + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
        // rows beyond n_rows[i] are never written by the kernels: zero, as epik_amd_placer_place leaves them
        HIP_TRY(hipMemsetAsync(d_rows, 0, cnt * keep * sizeof(epik_amd_placement), p->stream));
        HIP_TRY(hipMemsetAsync(d_counts, 0, cnt * keep * sizeof(uint32_t), p->stream));
        if (const uint64_t zeroed = v.zeroed_bytes ? v.zeroed_bytes(p, cnt, mode) : 0) HIP_TRY(hipMemsetAsync(d_ws, 0, zeroed, p->stream));
        uint64_t chunk_ws = 0;
        if (const int rc = v.workspace_bytes(p, cnt, bytes, mode, &chunk_ws); rc != EPIK_AMD_OK) return rc;
        if (const int rc = v.place_device_sized
                               ? v.place_device_sized(p, d, d_offs, cnt, bytes, mode, d_ws, chunk_ws, d_rows, d_nrows, d_counts, d_label, p->stream)
                               : v.place_device(p, d, d_offs, cnt, mode, d_ws, chunk_ws, d_rows, d_nrows, d_counts, d_label, p->stream);
            rc != EPIK_AMD_OK)
            return rc;
        if (sink)
            if (const int rc = sink->fn(sink->ctx, d_rows, d_nrows, d_counts, r0, cnt, p->stream); rc != EPIK_AMD_OK) return rc;
        if (rows) HIP_TRY(hipMemcpyAsync(rows + r0 * keep, d_rows, cnt * keep * sizeof(epik_amd_placement), hipMemcpyDeviceToHost, p->stream));
        if (n_rows) HIP_TRY(hipMemcpyAsync(n_rows + r0, d_nrows, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
        if (kmer_counts)
            HIP_TRY(hipMemcpyAsync(kmer_counts + r0 * keep, d_counts, cnt * keep * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
        if (label) HIP_TRY(hipMemcpyAsync(label + r0, d_label, cnt, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
    }
    return EPIK_AMD_OK;
}

// The profile-only host entry of a variant (profile_place.hip), once the caller has checked the handle, the mode and
// the reads (n >= 1, check_host_reads): place_host_chunked with every chunk's rows added to `profile` on the device,
// read i with weights[i] (NULL: 1), and nothing copied out but the label bytes (NULL: not even those).
int profile_host_chunked(epik_amd_placer *p, epik_amd_profile *profile, const char *seqs, const uint64_t *seq_offsets,
                         const uint32_t *weights, uint64_t n, uint32_t mode, uint64_t longest_placed, const HostVariant &v,
                         uint8_t *label);

// ... and whether that profile was created for this placer's device and shape (EPIK_AMD_ERR_INVALID otherwise)
int check_profile_pair(const epik_amd_placer *p, const epik_amd_profile *profile);

// What a host entry with placement confidence adds to its place_* twin (confidence_place.hip): the tree and tau_q of
// the rule, conf[n] on the host, and optionally a profile the rows are added to on the way, item i with weights[i]
// (host, or NULL: 1).
struct ConfidenceRequest {
    const epik_amd_tree *tree;
    uint32_t tau_q;
    epik_amd_confidence *conf;
    epik_amd_profile *profile;
    const uint32_t *weights;
};

// The confidence host entry of a variant, once the caller has checked the handle, the mode and the reads (n >= 1,
// check_host_reads): place_host_chunked with a sink that runs confidence_kernel on every chunk's device rows, copies
// its 16 bytes per item back and chains the profile add; rows, n_rows and kmer_counts may be NULL, each by itself.
int confidence_host_chunked(epik_amd_placer *p, const ConfidenceRequest &req, const char *seqs, const uint64_t *seq_offsets,
                            uint64_t n, uint32_t mode, uint64_t longest_placed, const HostVariant &v, epik_amd_placement *rows,
                            uint32_t *n_rows, uint32_t *kmer_counts, uint8_t *label);

// What the cohort's KR distance needs of a tree (confidence_place.hip owns the object): its device, N and first[] there.
int tree_first_device(const epik_amd_tree *tree, int *device, uint32_t *num_branches, const uint32_t **d_first);

// The cohort host entry of a variant (cohort_place.hip), once the caller has checked the handle, the mode and the reads
// (n >= 1, check_host_reads): profile_host_chunked with item i added to row samples[i] of `cohort` (HOST uint32 [n]);
// weights and samples are uploaded once and every chunk's add takes both offset by the chunk's first item.
int cohort_host_chunked(epik_amd_placer *p, epik_amd_cohort *cohort, const char *seqs, const uint64_t *seq_offsets,
                        const uint32_t *weights, const uint32_t *samples, uint64_t n, uint32_t mode, uint64_t longest_placed,
                        const HostVariant &v, uint8_t *label);

// What a host entry with taxonomic assignment adds to its place_* twin (taxa_place.hip): the object whose cells every
// chunk's rows are added to, tau_q, records[n] on the host (NULL: the records are not computed: cells only), weights
// and samples of the items (host, or NULL: 1 and sample 0), and optionally a profile OR a cohort (not both) that the
// same rows are added to on the way.
struct TaxaRequest {
    epik_amd_taxonomy *taxonomy;
    uint32_t tau_q;
    epik_amd_taxon_record *records;
    const uint32_t *weights, *samples;
    epik_amd_profile *profile;
    epik_amd_cohort *cohort;
};

// The taxonomy host entry of a variant, once the caller has checked the handle, the mode and the reads (n >= 1,
// check_host_reads): place_host_chunked with a sink that runs taxa_kernel on every chunk's device rows, copies the
// records back where they are asked for and chains the profile or the cohort add; weights and samples are uploaded once;
// rows, n_rows and kmer_counts may be NULL, each by itself.
int taxa_host_chunked(epik_amd_placer *p, const TaxaRequest &req, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                      uint32_t mode, uint64_t longest_placed, const HostVariant &v, epik_amd_placement *rows, uint32_t *n_rows,
                      uint32_t *kmer_counts, uint8_t *label);

}  // namespace epik_amd
#endif
