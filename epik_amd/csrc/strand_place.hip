// strand_place.hip -- nucleotide reads placed on either strand: epik_amd_placer_strand_workspace_bytes,
// epik_amd_placer_place_strands_device, epik_amd_placer_place_strands (include/epik_amd.h).
//
// No reference counterpart: the reference places a read in the orientation it arrives in (place.cpp:294,
// to_kmers over the read as given).  Short reads of a shotgun sample come from either strand, and a read of the
// opposite strand finds almost none of its k-mers in the database.
//
// Semantics:
//   * The complement is defined on character CLASSES: state s <-> 3 - s in the A C G T order of
//     epik_amd/alphabet.py -- the same unverified i2l state order everything else here rests on.  On a class
//     bitmask that is a 4-bit bit reversal: R (AG) <-> Y (CT), K <-> M, B <-> V, D <-> H; S, W and N map to
//     themselves; U complements to A; a character of class 0 (invalid) stays invalid.
//   * The reverse strand of read r is the read whose character j has class bitrev4(char_class[r[len-1-j]]).  Its
//     rows are exactly those of the host-side reverse complement of r, the ambiguous-k-mer path included (whose order
//     is the k-mer position in that reversed read).
//   * `both`: F = the forward result, R = the reverse one.  R is chosen when R has rows and either F has none or
//     R[0].score > F[0].score (float32, strict); else F -- a tie goes to forward (palindromic reads, reads without
//     hits on either strand).  Both strands have the same number of k-mers, so n_rows == 0 (shorter than k) and
//     EPIK_AMD_ROWS_COUNTS_TOO_NARROW always agree and report forward.  Rows, n_rows and k-mer counts are those of
//     the chosen strand, unchanged: LWRs are not renormalised across strands.  The scores compare because both
//     strands divide by the same n_kmers in the correction.
//   * Strand byte per read: 0 forward (+), 1 reverse (-).
//   * Nucleotide handles only (alphabet_size 4), whole databases only (no k-mer-space shard).
//
// Device side: the placement itself is epik_amd_placer_place_device, unchanged (every kernel and path it takes);
// here only two kernels around it:
//   revcomp_kernel        the reverse-complemented bytes of the batch into the workspace, at the caller's offsets
//                         (reversal stays inside each read's range, so d_seq_offsets serves both strands);
//   strand_select_kernel  forward placed into the caller's buffers, reverse into the workspace: overwrites the reads
//                         where reverse wins and writes the strand byte of every read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "host_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint64_t kMaxBlocks = 8192;  // (grid-stride beyond: a million reads is 256 K waves of work either way)

__global__ __launch_bounds__(kBlock) void revcomp_kernel(const uint8_t *__restrict__ seqs,
                                                         const uint64_t *__restrict__ seq_offsets, uint64_t n,
                                                         uint8_t *__restrict__ out, uint64_t out_cap, ComplementMap map)
{
    __shared__ uint8_t lut[256];
    lut[threadIdx.x] = map.byte[threadIdx.x];  // (kBlock == 256)
    __syncthreads();
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t waves = (uint64_t)gridDim.x * kBlockWaves;
    // A wave takes 64 reads at a time -- their offsets in one load -- and reverses them one after the other, in
    // tiles of 64 bytes, four tiles' loads in flight before their stores; reads of any length.
    for (uint64_t r0 = ((uint64_t)blockIdx.x * kBlockWaves + threadIdx.x / kWave) * kWave; r0 < n; r0 += waves * kWave) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(kWave, n - r0);
        const uint64_t my_b = lane < cnt ? seq_offsets[r0 + lane] : 0, my_e = lane < cnt ? seq_offsets[r0 + lane + 1] : 0;
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint64_t b = __shfl(my_b, (int)j), e = __shfl(my_e, (int)j);
            if (e < b || e > out_cap) continue;  // (outside the workspace the caller sized: nothing is written)
            const uint64_t len = e - b;
            for (uint64_t t0 = lane; t0 < len; t0 += 4 * kWave) {
                uint32_t c[4];
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u) {
                    const uint64_t t = t0 + u * kWave;
                    c[u] = t < len ? seqs[e - 1 - t] : 0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u) {
                    const uint64_t t = t0 + u * kWave;
                    if (t < len) out[b + t] = lut[c[u]];
                }
            }
        }
    }
}

// One wavefront per 64 reads: lane l decides for read 64 g + l, then the wave copies the rows of the reads where
// reverse won, 64 row slots at a time.  Every decision of the wave is loaded before any of its stores, and no other
// wave touches these reads: the forward rows a decision reads are never overwritten under it.
__global__ __launch_bounds__(kBlock) void strand_select_kernel(uint64_t n, uint32_t keep,
                                                               epik_amd_placement *__restrict__ rows,
                                                               uint32_t *__restrict__ n_rows,
                                                               uint32_t *__restrict__ counts,
                                                               const epik_amd_placement *__restrict__ rev_rows,
                                                               const uint32_t *__restrict__ rev_n_rows,
                                                               const uint32_t *__restrict__ rev_counts,
                                                               uint8_t *__restrict__ strand)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t groups = (n + kWave - 1) / kWave, waves = (uint64_t)gridDim.x * kBlockWaves;
    for (uint64_t g = (uint64_t)blockIdx.x * kBlockWaves + threadIdx.x / kWave; g < groups; g += waves) {
        const uint64_t first = g * kWave, i = first + lane;
        bool take = false;
        uint32_t nr = 0;
        if (i < n) {
            const uint32_t nf = n_rows[i];
            nr = rev_n_rows[i];
            if (has_rows(nr)) take = !has_rows(nf) || rev_rows[i * keep].score > rows[i * keep].score;
        }
        const unsigned long long mask = __ballot(take);
        if (i < n) {
            if (strand) strand[i] = take ? 1 : 0;
            if (take) n_rows[i] = nr;
        }
        if (mask == 0) continue;
        const uint64_t slots = std::min<uint64_t>(kWave, n - first) * keep;
        for (uint64_t s = lane; s < slots; s += kWave) {
            if (!((mask >> (s / keep)) & 1ull)) continue;
            const uint64_t at = first * keep + s;
            rows[at] = rev_rows[at];
            if (counts) counts[at] = rev_counts[at];
        }
    }
}

// what the workspace of a `both` placement holds ahead of the reversed bytes: the reverse strand's rows
struct WorkspaceLayout {
    uint64_t rows = 0, n_rows = 0, counts = 0, seqs = 0;  // byte offsets
    uint64_t per_read_bytes = 0;                          // = seqs
};
WorkspaceLayout layout_of(uint64_t n, uint32_t keep, uint32_t mode)
{
    WorkspaceLayout l;
    if (mode == EPIK_AMD_STRAND_BOTH) {
        l.rows = 0;
        l.n_rows = align_up(n * keep * sizeof(epik_amd_placement));
        l.counts = l.n_rows + align_up(n * sizeof(uint32_t));
        l.seqs = l.counts + align_up(n * keep * sizeof(uint32_t));
    }
    l.per_read_bytes = l.seqs;
    return l;
}

int check_handle(const epik_amd_placer *p, uint32_t mode)
{
    if (!p) return fail_with(EPIK_AMD_ERR_INVALID, "null placer");
    if (mode > EPIK_AMD_STRAND_BOTH) return fail_with(EPIK_AMD_ERR_INVALID, "strand mode must be FORWARD, REVERSE or BOTH");
    if (p->params.alphabet_size != 4)
        return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "strand placement needs a nucleotide placer (alphabet_size 4)");
    if (p->plan.shard_count > 1)
        return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "strand placement needs a whole database, not a k-mer-space shard");
    return EPIK_AMD_OK;
}

int place_strands_device_impl(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets, uint64_t n,
                              uint32_t mode, void *d_workspace, uint64_t workspace_bytes, void *d_rows, void *d_n_rows,
                              void *d_kmer_counts, void *d_strand, hipStream_t stream)
{
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (n == 0) return EPIK_AMD_OK;
    if (!d_seqs || !d_seq_offsets || !d_rows || !d_n_rows) return fail_with(EPIK_AMD_ERR_INVALID, "null device buffer");
    const uint32_t keep = p->params.keep_at_most;
    const WorkspaceLayout l = layout_of(n, keep, mode);
    if (mode != EPIK_AMD_STRAND_FORWARD && (!d_workspace || workspace_bytes <= l.per_read_bytes))
        return fail_with(EPIK_AMD_ERR_INVALID, "workspace smaller than epik_amd_placer_strand_workspace_bytes");
    ComplementMap map{};
    if (mode != EPIK_AMD_STRAND_FORWARD)
        if (const int rc = complement_map(p, map); rc != EPIK_AMD_OK) return rc;
    HIP_TRY(hipSetDevice(p->device));
    const auto *offs = static_cast<const uint64_t *>(d_seq_offsets);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    uint8_t *strand = static_cast<uint8_t *>(d_strand);

    if (mode != EPIK_AMD_STRAND_REVERSE) {  // forward: straight into the caller's buffers
        if (const int rc = epik_amd_placer_place_device(p, d_seqs, d_seq_offsets, n, d_rows, d_n_rows, d_kmer_counts, stream);
            rc != EPIK_AMD_OK)
            return rc;
        if (mode == EPIK_AMD_STRAND_FORWARD) {
            if (strand) HIP_TRY(hipMemsetAsync(strand, 0, n, stream));
            return EPIK_AMD_OK;
        }
    }
    uint8_t *rc_seqs = ws + l.seqs;
    hipLaunchKernelGGL(revcomp_kernel, dim3(grid_for((n + kWave - 1) / kWave, kMaxBlocks)), dim3(kBlock), 0, stream,
                       static_cast<const uint8_t *>(d_seqs), offs, n, rc_seqs, workspace_bytes - l.seqs, map);
    HIP_TRY(hipGetLastError());
    if (mode == EPIK_AMD_STRAND_REVERSE) {
        if (const int rc = epik_amd_placer_place_device(p, rc_seqs, d_seq_offsets, n, d_rows, d_n_rows, d_kmer_counts, stream);
            rc != EPIK_AMD_OK)
            return rc;
        if (strand) HIP_TRY(hipMemsetAsync(strand, 1, n, stream));
        return EPIK_AMD_OK;
    }
    auto *rev_rows = reinterpret_cast<epik_amd_placement *>(ws + l.rows);
    auto *rev_n_rows = reinterpret_cast<uint32_t *>(ws + l.n_rows);
    auto *rev_counts = d_kmer_counts ? reinterpret_cast<uint32_t *>(ws + l.counts) : nullptr;
    if (const int rc = epik_amd_placer_place_device(p, rc_seqs, d_seq_offsets, n, rev_rows, rev_n_rows, rev_counts, stream);
        rc != EPIK_AMD_OK)
        return rc;
    hipLaunchKernelGGL(strand_select_kernel, dim3(grid_for((n + kWave - 1) / kWave, kMaxBlocks)), dim3(kBlock), 0, stream,
                       n, keep, static_cast<epik_amd_placement *>(d_rows), static_cast<uint32_t *>(d_n_rows),
                       static_cast<uint32_t *>(d_kmer_counts), rev_rows, rev_n_rows, rev_counts, strand);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

// The host entry zeroes what a `both` placement holds ahead of the reversed bytes before every chunk:
// strand_select_kernel copies all keep row slots of a read where reverse won, and the placement writes n_rows of them.
uint64_t reverse_rows_bytes(const epik_amd_placer *p, uint64_t n, uint32_t mode)
{
    return layout_of(n, p->params.keep_at_most, mode).per_read_bytes;
}

constexpr HostVariant kStrandHost{.chunk_reads = 1u << 18, .chunk_bytes = 64u << 20, .chunk_reads_env = "EPIK_AMD_STRAND_CHUNK_READS",
                                  .workspace_bytes = epik_amd_placer_strand_workspace_bytes,
                                  .zeroed_bytes = reverse_rows_bytes, .place_device = place_strands_device_impl};

int place_strands_impl(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n, uint32_t mode,
                       epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts, uint8_t *strand)
{
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (n == 0) return EPIK_AMD_OK;
    uint64_t longest = 0;
    if (const int rc = check_host_batch(seqs, seq_offsets, n, rows, n_rows, longest); rc != EPIK_AMD_OK) return rc;
    return place_host_chunked(p, seqs, seq_offsets, n, mode, longest, kStrandHost, rows, n_rows, kmer_counts, strand);
}

// the same placement with the rows left on the device and summed into a profile there (profile_place.hip)
int profile_strands_impl(epik_amd_placer *p, epik_amd_profile *profile, const char *seqs, const uint64_t *seq_offsets,
                         const uint32_t *weights, uint64_t n, uint32_t mode, uint8_t *strand)
{
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (!profile) return fail_with(EPIK_AMD_ERR_INVALID, "null profile");
    if (n == 0) return EPIK_AMD_OK;
    uint64_t longest = 0;
    if (const int rc = check_host_reads(seqs, seq_offsets, n, longest); rc != EPIK_AMD_OK) return rc;
    return profile_host_chunked(p, profile, seqs, seq_offsets, weights, n, mode, longest, kStrandHost, strand);
}

}  // namespace

extern "C" {

int epik_amd_placer_strand_workspace_bytes(const epik_amd_placer *p, uint64_t n, uint64_t seq_bytes, uint32_t mode,
                                           uint64_t *bytes)
{
    if (!bytes) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    *bytes = 0;
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (mode == EPIK_AMD_STRAND_FORWARD || n == 0) return EPIK_AMD_OK;
    // (+1: a batch of empty reads still has a workspace of more than its per-read part)
    *bytes = layout_of(n, p->params.keep_at_most, mode).seqs + align_up(seq_bytes + 1);
    return EPIK_AMD_OK;
}

int epik_amd_placer_place_strands_device(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets, uint64_t n,
                                         uint32_t mode, void *d_workspace, uint64_t workspace_bytes, void *d_rows,
                                         void *d_n_rows, void *d_kmer_counts, void *d_strand, void *stream)
{
    return place_strands_device_impl(p, d_seqs, d_seq_offsets, n, mode, d_workspace, workspace_bytes, d_rows, d_n_rows,
                                     d_kmer_counts, d_strand, static_cast<hipStream_t>(stream));
}

int epik_amd_placer_place_strands(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                  uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                  uint8_t *strand)
{
    try {  // std::vector: nothing may leave through the C ABI
        return place_strands_impl(p, seqs, seq_offsets, n, mode, rows, n_rows, kmer_counts, strand);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("place_strands: ") + e.what());
    }
}

int epik_amd_placer_profile_strands(epik_amd_placer *p, epik_amd_profile *profile, const char *seqs,
                                    const uint64_t *seq_offsets, const uint32_t *weights, uint64_t n, uint32_t mode,
                                    uint8_t *strand)
{
    try {
        return profile_strands_impl(p, profile, seqs, seq_offsets, weights, n, mode, strand);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("profile_strands: ") + e.what());
    }
}

int epik_amd_placer_cohort_strands(epik_amd_placer *p, epik_amd_cohort *cohort, const char *seqs, const uint64_t *seq_offsets,
                                    const uint32_t *weights, const uint32_t *samples, uint64_t n, uint32_t mode, uint8_t *strand)
{
    try {  // (profile_strands with a row of cells per sample: cohort_place.hip)
        if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
        if (!cohort) return fail_with(EPIK_AMD_ERR_INVALID, "null cohort");
        if (n == 0) return EPIK_AMD_OK;
        uint64_t longest = 0;
        if (const int rc = check_host_reads(seqs, seq_offsets, n, longest); rc != EPIK_AMD_OK) return rc;
        return cohort_host_chunked(p, cohort, seqs, seq_offsets, weights, samples, n, mode, longest, kStrandHost, strand);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("cohort_strands: ") + e.what());
    }
}

int epik_amd_placer_confidence_strands(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                         uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                         uint8_t *strand, const epik_amd_tree *tree, uint32_t tau_q, epik_amd_confidence *conf,
                                         epik_amd_profile *profile, const uint32_t *weights)
{
    try {  // (place_strands with the confidence records of confidence_place.hip computed from each chunk's device rows)
        if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
        if (n == 0) return EPIK_AMD_OK;
        uint64_t longest = 0;
        if (const int rc = check_host_reads(seqs, seq_offsets, n, longest); rc != EPIK_AMD_OK) return rc;
        return confidence_host_chunked(p, ConfidenceRequest{tree, tau_q, conf, profile, weights}, seqs, seq_offsets, n, mode,
                                       longest, kStrandHost, rows, n_rows, kmer_counts, strand);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("confidence_strands: ") + e.what());
    }
}

int epik_amd_placer_taxa_strands(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                         uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                         uint8_t *strand, epik_amd_taxonomy *taxonomy, uint32_t tau_q,
        epik_amd_taxon_record *records, const uint32_t *weights, const uint32_t *samples, epik_amd_profile *profile,
        epik_amd_cohort *cohort)
{
    try {  // (the same with the taxonomic assignment of taxa_place.hip run on each chunk's device rows)
        if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
        if (n == 0) return EPIK_AMD_OK;
        uint64_t longest = 0;
        if (const int rc = check_host_reads(seqs, seq_offsets, n, longest); rc != EPIK_AMD_OK) return rc;
        return taxa_host_chunked(p, TaxaRequest{taxonomy, tau_q, records, weights, samples, profile, cohort}, seqs, seq_offsets, n, mode,
                                       longest, kStrandHost, rows, n_rows, kmer_counts, strand);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("taxa_strands: ") + e.what());
    }
}

}  // extern "C"
