// mates_place.hip -- paired-end reads placed jointly, one placement per fragment: epik_amd_placer_mates_separator,
// epik_amd_placer_mates_workspace_bytes, epik_amd_placer_place_mates_device, epik_amd_placer_place_mates,
// epik_amd_placer_profile_mates (include/epik_amd.h).
//
// No reference counterpart: the reference knows single reads only (place.cpp:294, to_kmers over the read as given).
//
// The rule (include/epik_amd.h).  For a pair (m1, m2), sep a byte of character class 0:
//     J = m1 . sep . rc(m2)     orientation FR (Illumina paired-end)
//     J = m1 . sep . m2         orientation FF (EPIK_AMD_MATES_FF)
// and the placement of the pair is the placement of J, strand modes included: the reverse strand of J is the pair with
// its mates swapped.  Windows over sep are skipped as windows over any invalid character are, so every branch gets the
// log-scores of both mates' k-mers, mate 1's first, in k-mer order.
//
// Device side: no placement kernel of its own.  mate_join_kernel writes the J of every pair and their offsets into the
// caller's workspace; epik_amd_placer_place_strands_device places them (revcomp_kernel, the placement kernels,
// strand_select_kernel -- all unchanged).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "host_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint64_t kMaxBlocks = 8192;  // (grid-stride beyond, as revcomp_kernel)
constexpr uint32_t kStrandMask = 0xffu, kKnownBits = kStrandMask | EPIK_AMD_MATES_FF;

// len bytes from src to dst, unchanged, by the whole wave.  The destination is written in aligned dwords between a head
// and a tail of single bytes; a dword comes from the one or two aligned source dwords that hold its bytes (every one
// of them holds at least one byte of the source range, so none lies on a page the range does not touch).  Four tiles
// of 64 dwords are loaded before their stores.
__device__ inline void copy_forward(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t len, uint32_t lane)
{
    const uint64_t head = std::min<uint64_t>(len, (4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3);
    const uint64_t words = (len - head) / 4, tail = head + 4 * words;
    if (lane < head) dst[lane] = src[lane];
    if (lane < len - tail) dst[tail + lane] = src[tail + lane];
    if (words == 0) return;
    const uint32_t misalign = (uint32_t)(reinterpret_cast<uintptr_t>(src + head) & 3);
    const uint32_t shift = 8 * misalign;  // (the same for every dword of the copy)
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(src + head - misalign);
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
    for (uint64_t t0 = lane; t0 < words; t0 += 4 * kWave) {
        uint32_t lo[4], hi[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
            const uint64_t t = t0 + u * kWave;
            lo[u] = t < words ? sw[t] : 0u;
            hi[u] = t < words && shift ? sw[t + 1] : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
            const uint64_t t = t0 + u * kWave;
            if (t < words) dw[t] = shift ? (uint32_t)((((uint64_t)hi[u] << 32) | lo[u]) >> shift) : lo[u];
        }
    }
}

// A wave takes 64 pairs at a time -- their offsets loaded once, a lane each -- writes their joined offsets, then joins
// them one after the other: mate 1 copied (copy_forward), the separator, mate 2 through the complement map reversed
// (FR: tiles of 64 bytes, four tiles' loads in flight before their stores, as revcomp_kernel) or copied (FF).  Pairs
// of any length, empty mates included.  joined_offsets[i] = seq_offsets[2 i] - seq_offsets[0] + i, no scan; nothing is
// written at or beyond out + out_cap, and no joined offset exceeds out_cap (a pair whose offsets do not fit what the
// caller sized is left unwritten).
__global__ __launch_bounds__(kBlock) void mate_join_kernel(const uint8_t *__restrict__ seqs,
                                                           const uint64_t *__restrict__ seq_offsets, uint64_t n,
                                                           uint8_t *__restrict__ out, uint64_t out_cap,
                                                           uint64_t *__restrict__ joined_offsets, uint32_t ff, uint8_t sep,
                                                           ComplementMap map)
{
    __shared__ uint8_t lut[256];
    lut[threadIdx.x] = map.byte[threadIdx.x];  // (kBlock == 256)
    __syncthreads();
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t waves = (uint64_t)gridDim.x * kBlockWaves;
    const uint64_t base = seq_offsets[0];
    for (uint64_t r0 = ((uint64_t)blockIdx.x * kBlockWaves + threadIdx.x / kWave) * kWave; r0 < n; r0 += waves * kWave) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(kWave, n - r0);
        uint64_t my_b = 0, my_m = 0, my_e = 0;
        if (lane < cnt) {
            const uint64_t i = r0 + lane;
            my_b = seq_offsets[2 * i], my_m = seq_offsets[2 * i + 1], my_e = seq_offsets[2 * i + 2];
            joined_offsets[i] = std::min(my_b - base + i, out_cap);
            if (i + 1 == n) joined_offsets[n] = std::min(my_e - base + n, out_cap);
        }
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint64_t b = __shfl(my_b, (int)j), m = __shfl(my_m, (int)j), e = __shfl(my_e, (int)j);
            if (b < base || m < b || e < m) continue;
            const uint64_t at = b - base + r0 + j, len1 = m - b, len2 = e - m;
            if (e - base + r0 + j + 1 > out_cap) continue;  // (outside the workspace the caller sized: nothing is written)
            copy_forward(seqs + b, out + at, len1, lane);
            uint8_t *second = out + at + len1 + 1;
            if (lane == 0) second[-1] = sep;
            if (ff) {
                copy_forward(seqs + m, second, len2, lane);
                continue;
            }
            for (uint64_t t0 = lane; t0 < len2; t0 += 4 * kWave) {
                uint32_t c[4];
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u) {
                    const uint64_t t = t0 + u * kWave;
                    c[u] = t < len2 ? seqs[e - 1 - t] : 0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u) {
                    const uint64_t t = t0 + u * kWave;
                    if (t < len2) second[t] = lut[c[u]];
                }
            }
        }
    }
}

int check_handle(const epik_amd_placer *p, uint32_t mode)
{
    if (!p) return fail_with(EPIK_AMD_ERR_INVALID, "null placer");
    if ((mode & ~kKnownBits) || (mode & kStrandMask) > EPIK_AMD_STRAND_BOTH)
        return fail_with(EPIK_AMD_ERR_INVALID, "mates mode must be a strand mode (FORWARD, REVERSE or BOTH), with EPIK_AMD_MATES_FF or without");
    if (p->params.alphabet_size != 4)
        return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "mates placement needs a nucleotide placer (alphabet_size 4)");
    if (p->plan.shard_count > 1)
        return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "mates placement needs a whole database, not a k-mer-space shard");
    return EPIK_AMD_OK;
}

// '-' when the handle's table has it invalid, else the smallest byte of class 0
int separator_of(const epik_amd_placer *p, uint8_t &sep)
{
    if (p->h_char_class.size() != 256) return fail_with(EPIK_AMD_ERR_INVALID, "placer has no character table");
    if (p->h_char_class[(uint8_t)'-'] == 0) {
        sep = (uint8_t)'-';
        return EPIK_AMD_OK;
    }
    for (int c = 0; c < 256; ++c)
        if (p->h_char_class[c] == 0) {
            sep = (uint8_t)c;
            return EPIK_AMD_OK;
        }
    return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "the character table has no invalid character (class 0) to separate the mates with");
}

// the workspace: what the strand placement of the joined batch needs (its reverse rows first: the host entry zeroes
// them) | joined_offsets [n + 1] | the joined bytes
struct WorkspaceLayout {
    uint64_t strand_bytes = 0, offsets = 0, joined = 0, joined_cap = 0, total = 0;
};
int layout_of(const epik_amd_placer *p, uint64_t n, uint64_t seq_bytes, uint32_t mode, WorkspaceLayout &l)
{
    l.joined_cap = seq_bytes + n;  // (a separator per pair)
    if (const int rc = epik_amd_placer_strand_workspace_bytes(p, n, l.joined_cap, mode & kStrandMask, &l.strand_bytes); rc != EPIK_AMD_OK)
        return rc;
    l.offsets = l.strand_bytes;
    l.joined = l.offsets + align_up((n + 1) * sizeof(uint64_t));
    l.total = l.joined + align_up(l.joined_cap + 1);
    return EPIK_AMD_OK;
}

int place_mates_device_impl(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets, uint64_t n, uint64_t seq_bytes,
                            uint32_t mode, void *d_workspace, uint64_t workspace_bytes, void *d_rows, void *d_n_rows,
                            void *d_kmer_counts, void *d_strand, hipStream_t stream)
{
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (n == 0) return EPIK_AMD_OK;
    if (!d_seqs || !d_seq_offsets || !d_rows || !d_n_rows) return fail_with(EPIK_AMD_ERR_INVALID, "null device buffer");
    WorkspaceLayout l;
    if (const int rc = layout_of(p, n, seq_bytes, mode, l); rc != EPIK_AMD_OK) return rc;
    if (!d_workspace || workspace_bytes < l.total)
        return fail_with(EPIK_AMD_ERR_INVALID, "workspace smaller than epik_amd_placer_mates_workspace_bytes");
    uint8_t sep = 0;
    if (const int rc = separator_of(p, sep); rc != EPIK_AMD_OK) return rc;
    const uint32_t ff = (mode & EPIK_AMD_MATES_FF) ? 1u : 0u;
    ComplementMap map{};
    if (!ff)
        if (const int rc = complement_map(p, map); rc != EPIK_AMD_OK) return rc;
    HIP_TRY(hipSetDevice(p->device));
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    auto *joined_offsets = reinterpret_cast<uint64_t *>(ws + l.offsets);
    hipLaunchKernelGGL(mate_join_kernel, dim3(grid_for((n + kWave - 1) / kWave, kMaxBlocks)), dim3(kBlock), 0, stream,
                       static_cast<const uint8_t *>(d_seqs), static_cast<const uint64_t *>(d_seq_offsets), n, ws + l.joined,
                       l.joined_cap, joined_offsets, ff, sep, map);
    HIP_TRY(hipGetLastError());
    return epik_amd_placer_place_strands_device(p, ws + l.joined, joined_offsets, n, mode & kStrandMask,
                                                l.strand_bytes ? ws : nullptr, l.strand_bytes, d_rows, d_n_rows, d_kmer_counts,
                                                d_strand, stream);
}

int workspace_bytes_impl(const epik_amd_placer *p, uint64_t n, uint64_t seq_bytes, uint32_t mode, uint64_t *bytes)
{
    if (!bytes) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    *bytes = 0;
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (n == 0) return EPIK_AMD_OK;
    WorkspaceLayout l;
    if (const int rc = layout_of(p, n, seq_bytes, mode, l); rc != EPIK_AMD_OK) return rc;
    *bytes = l.total;
    return EPIK_AMD_OK;
}

// The host entry zeroes the reverse strand's rows of a `both` placement before every chunk, as place_strands does:
// they open the strand placement's workspace, which opens this one (all of it but the reversed bytes: the strand
// workspace of a batch without characters, less the one aligned unit those take).
uint64_t reverse_rows_bytes(const epik_amd_placer *p, uint64_t n, uint32_t mode)
{
    uint64_t bytes = 0;
    if (epik_amd_placer_strand_workspace_bytes(p, n, 0, mode & kStrandMask, &bytes) != EPIK_AMD_OK || bytes < align_up(1)) return 0;
    return bytes - align_up(1);
}

constexpr HostVariant kMatesHost{.chunk_reads = 1u << 18, .chunk_bytes = 64u << 20, .chunk_reads_env = "EPIK_AMD_MATES_CHUNK_READS",
                                 .workspace_bytes = workspace_bytes_impl, .zeroed_bytes = reverse_rows_bytes,
                                 .place_device = nullptr, .item_reads = 2, .place_device_sized = place_mates_device_impl};

// The checks of a host batch of n >= 1 pairs (2 n reads); `longest` gets the longest joined sequence
int check_host_pairs(const char *seqs, const uint64_t *seq_offsets, uint64_t n, uint64_t &longest)
{
    if (n > 0x7fffffffull) return fail_with(EPIK_AMD_ERR_INVALID, "a batch of 2^31 pairs or more");
    uint64_t longest_mate = 0;
    if (const int rc = check_host_reads(seqs, seq_offsets, 2 * n, longest_mate); rc != EPIK_AMD_OK) return rc;
    longest = 0;
    for (uint64_t i = 0; i < n; ++i) longest = std::max<uint64_t>(longest, seq_offsets[2 * i + 2] - seq_offsets[2 * i] + 1);
    if (longest > 0xffffffffull) return fail_with(EPIK_AMD_ERR_INVALID, "a pair of 2^32 characters or more");
    return EPIK_AMD_OK;
}

int place_mates_impl(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n, uint32_t mode,
                     epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts, uint8_t *strand)
{
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (n == 0) return EPIK_AMD_OK;
    if (!rows || !n_rows) return fail_with(EPIK_AMD_ERR_INVALID, "null host buffer");
    uint64_t longest = 0;
    if (const int rc = check_host_pairs(seqs, seq_offsets, n, longest); rc != EPIK_AMD_OK) return rc;
    return place_host_chunked(p, seqs, seq_offsets, n, mode, longest, kMatesHost, rows, n_rows, kmer_counts, strand);
}

// the same placement with the rows left on the device and summed into a profile there (profile_place.hip)
int profile_mates_impl(epik_amd_placer *p, epik_amd_profile *profile, const char *seqs, const uint64_t *seq_offsets,
                       const uint32_t *weights, uint64_t n, uint32_t mode, uint8_t *strand)
{
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (!profile) return fail_with(EPIK_AMD_ERR_INVALID, "null profile");
    if (n == 0) return EPIK_AMD_OK;
    uint64_t longest = 0;
    if (const int rc = check_host_pairs(seqs, seq_offsets, n, longest); rc != EPIK_AMD_OK) return rc;
    return profile_host_chunked(p, profile, seqs, seq_offsets, weights, n, mode, longest, kMatesHost, strand);
}

}  // namespace

extern "C" {

int epik_amd_placer_mates_separator(const epik_amd_placer *p, uint8_t *sep)
{
    if (!sep) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    *sep = 0;
    if (const int rc = check_handle(p, EPIK_AMD_STRAND_FORWARD); rc != EPIK_AMD_OK) return rc;
    return separator_of(p, *sep);
}

int epik_amd_placer_mates_workspace_bytes(const epik_amd_placer *p, uint64_t n_pairs, uint64_t seq_bytes, uint32_t mode,
                                          uint64_t *bytes)
{
    return workspace_bytes_impl(p, n_pairs, seq_bytes, mode, bytes);
}

int epik_amd_placer_place_mates_device(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets, uint64_t n_pairs,
                                       uint64_t seq_bytes, uint32_t mode, void *d_workspace, uint64_t workspace_bytes,
                                       void *d_rows, void *d_n_rows, void *d_kmer_counts, void *d_strand, void *stream)
{
    return place_mates_device_impl(p, d_seqs, d_seq_offsets, n_pairs, seq_bytes, mode, d_workspace, workspace_bytes, d_rows,
                                   d_n_rows, d_kmer_counts, d_strand, static_cast<hipStream_t>(stream));
}

int epik_amd_placer_place_mates(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n_pairs,
                                uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                uint8_t *strand)
{
    try {  // std::vector: nothing may leave through the C ABI
        return place_mates_impl(p, seqs, seq_offsets, n_pairs, mode, rows, n_rows, kmer_counts, strand);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("place_mates: ") + e.what());
    }
}

int epik_amd_placer_profile_mates(epik_amd_placer *p, epik_amd_profile *profile, const char *seqs,
                                  const uint64_t *seq_offsets, const uint32_t *weights, uint64_t n_pairs, uint32_t mode,
                                  uint8_t *strand)
{
    try {
        return profile_mates_impl(p, profile, seqs, seq_offsets, weights, n_pairs, mode, strand);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("profile_mates: ") + e.what());
    }
}

int epik_amd_placer_cohort_mates(epik_amd_placer *p, epik_amd_cohort *cohort, const char *seqs, const uint64_t *seq_offsets,
                                  const uint32_t *weights, const uint32_t *samples, uint64_t n_pairs, uint32_t mode, uint8_t *strand)
{
    try {  // (profile_mates with a row of cells per sample: cohort_place.hip)
        if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
        if (!cohort) return fail_with(EPIK_AMD_ERR_INVALID, "null cohort");
        if (n_pairs == 0) return EPIK_AMD_OK;
        uint64_t longest = 0;
        if (const int rc = check_host_pairs(seqs, seq_offsets, n_pairs, longest); rc != EPIK_AMD_OK) return rc;
        return cohort_host_chunked(p, cohort, seqs, seq_offsets, weights, samples, n_pairs, mode, longest, kMatesHost, strand);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("cohort_mates: ") + e.what());
    }
}

int epik_amd_placer_confidence_mates(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n_pairs,
                                       uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                       uint8_t *strand, const epik_amd_tree *tree, uint32_t tau_q, epik_amd_confidence *conf,
                                       epik_amd_profile *profile, const uint32_t *weights)
{
    try {  // (place_mates with the confidence records of confidence_place.hip computed from each chunk's device rows)
        if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
        if (n_pairs == 0) return EPIK_AMD_OK;
        uint64_t longest = 0;
        if (const int rc = check_host_pairs(seqs, seq_offsets, n_pairs, longest); rc != EPIK_AMD_OK) return rc;
        return confidence_host_chunked(p, ConfidenceRequest{tree, tau_q, conf, profile, weights}, seqs, seq_offsets, n_pairs, mode,
                                       longest, kMatesHost, rows, n_rows, kmer_counts, strand);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("confidence_mates: ") + e.what());
    }
}

int epik_amd_placer_taxa_mates(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n_pairs,
                                       uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                       uint8_t *strand, epik_amd_taxonomy *taxonomy, uint32_t tau_q,
        epik_amd_taxon_record *records, const uint32_t *weights, const uint32_t *samples, epik_amd_profile *profile,
        epik_amd_cohort *cohort)
{
    try {  // (the same with the taxonomic assignment of taxa_place.hip run on each chunk's device rows)
        if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
        if (n_pairs == 0) return EPIK_AMD_OK;
        uint64_t longest = 0;
        if (const int rc = check_host_pairs(seqs, seq_offsets, n_pairs, longest); rc != EPIK_AMD_OK) return rc;
        return taxa_host_chunked(p, TaxaRequest{taxonomy, tau_q, records, weights, samples, profile, cohort}, seqs, seq_offsets, n_pairs, mode,
                                       longest, kMatesHost, rows, n_rows, kmer_counts, strand);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("taxa_mates: ") + e.what());
    }
}

}  // extern "C"
