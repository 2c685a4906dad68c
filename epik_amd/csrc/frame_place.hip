// frame_place.hip -- nucleotide reads placed on an amino-acid database through their translated frames:
// epik_amd_codon_table, epik_amd_placer_frame_workspace_bytes, epik_amd_placer_place_frames_device,
// epik_amd_placer_place_frames (include/epik_amd.h).
//
// No reference counterpart: the reference places a read in the alphabet of its database (place.cpp:294).  A shotgun
// read is DNA, and a protein tree (amoA, nifH, rpoB, ...) is searched with it only after translation; five of the six
// frames are noise, and choosing the frame is the step done wrong by hand.
//
// Semantics:
//   * Frames.  Frame +f (f = 1, 2, 3) translates the codons that start at offset f-1 of the read; frame -f does the
//     same on the reverse complement.  An incomplete trailing codon is dropped: a read of length L gives frames of
//     floor((L - f + 1) / 3) residues (0 when that is negative).  The reverse complement is strand_place.hip's: the
//     class bitmask reversed, in A C G T order.
//   * Codon -> residue: one 4096-entry byte table indexed by the three nucleotide class masks (4 bits each, first
//     nucleotide most significant), built at compile time from the standard genetic code (NCBI table 1, which also
//     serves table 11).  A codon with a class-0 (invalid) character is '*'.  Otherwise every combination of its
//     ambiguous characters (at most 64) is expanded: one amino acid -> that letter; only stops -> '*'; the sets
//     {D,N}, {E,Q}, {I,L} -> B, Z, J; any other set, a mix of stops and amino acids included -> X.  U is T, lower
//     case is upper case.  '*' must be class 0 in the handle's class table (alphabet.py), so that k-mers across a
//     stop or a gap are skipped as for any invalid character: EPIK_AMD_ERR_UNSUPPORTED otherwise.
//   * Choosing a frame.  A frame has rows when its n_rows is neither 0 nor EPIK_AMD_ROWS_COUNTS_TOO_NARROW.  Its key
//     is score[0] / (float)(len_f - k + 1), a float32 division rounded to nearest: the per-k-mer score (frames of one
//     read differ by a residue, and the correction adds one log_threshold term per k-mer, so raw scores do not
//     compare).  The frame with rows and the strictly greatest key wins; a tie goes to the earlier frame in the order
//     +1 +2 +3 -1 -2 -3.  No frame with rows: the read reports the first frame of the mode with its n_rows (0).  Any
//     frame EPIK_AMD_ROWS_COUNTS_TOO_NARROW: the read is too.  Rows, counts and LWRs are the winning frame's, not
//     renormalised.
//   * Frame byte per read: 0..5 for +1 +2 +3 -1 -2 -3.
//   * Amino-acid handles (alphabet_size 20) of a whole database only (no k-mer-space shard).
//
// Device side: the placement itself is epik_amd_placer_place_device, unchanged, called ONCE over all the frames of the
// batch (frame read m*i + j, m = 3 or 6).  Around it:
//   frame_length_kernel  per read the residues of one direction's three frames, max(L - 2, 0);
//   (hipCUB)             their exclusive sum: where each read's frames start;
//   translate_kernel     one pass over each read's window produces both directions' frames, read-major;
//   frame_select_kernel  the m-way rule: writes the caller's rows, n_rows, counts and frame bytes.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>

#include "host_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint64_t kMaxBlocks = 4096;
// codon starts per window of translate_kernel: a multiple of 3, and the window (+2 bytes, +15 of alignment) in one
// 16-byte load per lane
constexpr uint32_t kTile = 768;
static_assert(kTile % 3 == 0 && (kTile + 2 + 15 + 15) / 16 <= kWave, "one window, one load per lane");

// ---- the tables (compile time) --------------------------------------------------------------------------------

struct ByteTable256 {
    uint8_t v[256];
};
struct alignas(16) CodonTable {
    uint8_t v[4096];
};

// nucleotide class bitmask of every byte: A 1, C 2, G 4, T 8 (alphabet.py's A C G T order); U is T; IUPAC codes;
// lower case as upper; anything else 0
constexpr ByteTable256 make_nucl_class()
{
    ByteTable256 t{};
    const char *codes[][2] = {{"A", "A"},  {"C", "C"},  {"G", "G"},  {"T", "T"},  {"U", "T"},   {"R", "AG"},
                              {"Y", "CT"}, {"S", "CG"}, {"W", "AT"}, {"K", "GT"}, {"M", "AC"},  {"B", "CGT"},
                              {"D", "AGT"}, {"H", "ACT"}, {"V", "ACG"}, {"N", "ACGT"}};
    for (const auto &code : codes) {
        uint8_t mask = 0;
        for (const char *s = code[1]; *s; ++s) mask |= *s == 'A' ? 1 : *s == 'C' ? 2 : *s == 'G' ? 4 : 8;
        t.v[(uint8_t)code[0][0]] = mask;
        t.v[(uint8_t)(code[0][0] - 'A' + 'a')] = mask;
    }
    return t;
}

// NCBI translation table 1, codons in T C A G order of the first, second and third nucleotide
constexpr const char kStandardCode[] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";

constexpr CodonTable make_codon_table()
{
    CodonTable t{};
    const uint32_t tcag[4] = {3, 1, 0, 2};  // bit of T, C, A, G in the class mask -> position in kStandardCode
    uint32_t pos_of_bit[4] = {};
    for (uint32_t q = 0; q < 4; ++q) pos_of_bit[tcag[q]] = q;
    for (uint32_t idx = 0; idx < 4096; ++idx) {
        const uint32_t c[3] = {idx >> 8 & 15u, idx >> 4 & 15u, idx & 15u};
        if (!c[0] || !c[1] || !c[2]) {
            t.v[idx] = '*';
            continue;
        }
        bool seen[26] = {};
        bool stop = false;
        uint32_t distinct = 0;
        char one = 0;
        for (uint32_t a = 0; a < 4; ++a)
            for (uint32_t b = 0; b < 4; ++b)
                for (uint32_t d = 0; d < 4; ++d) {
                    if (!(c[0] >> a & 1u) || !(c[1] >> b & 1u) || !(c[2] >> d & 1u)) continue;
                    const char aa = kStandardCode[pos_of_bit[a] * 16 + pos_of_bit[b] * 4 + pos_of_bit[d]];
                    if (aa == '*') {
                        stop = true;
                    } else if (!seen[aa - 'A']) {
                        seen[aa - 'A'] = true;
                        ++distinct;
                        one = aa;
                    }
                }
        char out = 'X';
        if (!stop && distinct == 1)
            out = one;
        else if (stop && distinct == 0)
            out = '*';
        else if (!stop && distinct == 2)
            out = seen['D' - 'A'] && seen['N' - 'A'] ? 'B' : seen['E' - 'A'] && seen['Q' - 'A'] ? 'Z'
                  : seen['I' - 'A'] && seen['L' - 'A']                                       ? 'J'
                                                                                             : 'X';
        t.v[idx] = (uint8_t)out;
    }
    return t;
}

constexpr CodonTable kCodonTable = make_codon_table();
__device__ const ByteTable256 d_nucl_class = make_nucl_class();
__device__ const CodonTable d_codon_table = make_codon_table();

// ---- kernels --------------------------------------------------------------------------------------------------

// the LDS of one wave is written and read by its own lanes only: order the two within the wave
__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a wave-uniform value in scalar registers
__device__ inline uint64_t uniform(uint64_t x)
{
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32 |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
}

// per read the residues of one direction's three frames (none for a read of 2^32 characters or more); slot n gets 0 (the exclusive sum's last slot is the total)
__global__ __launch_bounds__(kBlock) void frame_length_kernel(const uint64_t *__restrict__ seq_offsets, uint64_t n,
                                                              uint64_t *__restrict__ totals)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * kBlock) {
        uint64_t t = 0;
        if (i < n) {
            const uint64_t b = seq_offsets[i], e = seq_offsets[i + 1];
            t = e > b + 2 && e - b <= 0xffffffffull ? e - b - 2 : 0;
        }
        totals[i] = t;
    }
}

// A wave takes 64 reads at a time -- their offsets and frame bases in one load each -- and translates them one
// after the other, in windows of kTile codon starts: the window's bytes (+2) come in with one aligned 16-byte load
// per lane into the wave's LDS; then the lanes walk the window's outputs -- per frame a contiguous run of residues --
// so that neighbouring lanes store neighbouring bytes, each reading its codon from LDS and its residue from the LDS
// copy of the codon table.  Frame read m*i + d*3 + f: direction d (forward first when both), frame f.  Frame offsets
// are clamped to the workspace (out_cap): a workspace too small gives wrong frames, never an access outside it.
__global__ __launch_bounds__(kBlock) void translate_kernel(const uint8_t *__restrict__ seqs,
                                                           const uint64_t *__restrict__ seq_offsets, uint64_t n,
                                                           const uint64_t *__restrict__ read_base, uint32_t mode,
                                                           uint8_t *__restrict__ out, uint64_t out_cap,
                                                           uint64_t *__restrict__ frame_offsets)
{
    __shared__ alignas(16) uint8_t codon[4096];
    __shared__ uint8_t nclass[256];
    __shared__ uint4 window[kBlockWaves][kWave];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(d_codon_table.v);
        reinterpret_cast<uint4 *>(codon)[threadIdx.x] = src[threadIdx.x];  // (kBlock * 16 == 4096)
        nclass[threadIdx.x] = d_nucl_class.v[threadIdx.x];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const bool fwd = mode != EPIK_AMD_FRAMES_REVERSE, rev = mode != EPIK_AMD_FRAMES_FORWARD;
    const uint32_t dirs = fwd && rev ? 2 : 1, m = 3 * dirs;
    const uint8_t *win = reinterpret_cast<const uint8_t *>(window[wave]);
    const uint64_t waves = (uint64_t)gridDim.x * kBlockWaves;
    for (uint64_t r0 = ((uint64_t)blockIdx.x * kBlockWaves + wave) * kWave; r0 < n; r0 += waves * kWave) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(kWave, n - r0);
        const uint64_t my_b = lane < cnt ? seq_offsets[r0 + lane] : 0, my_e = lane < cnt ? seq_offsets[r0 + lane + 1] : 0;
        const uint64_t my_o = lane < cnt ? dirs * read_base[r0 + lane] : 0;
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint64_t i = r0 + j;
            // (wave-uniform: in scalar registers; positions inside a read in 32 bits)
            const uint64_t b = uniform(__shfl(my_b, (int)j)), e = uniform(__shfl(my_e, (int)j));
            const uint64_t ob = uniform(__shfl(my_o, (int)j));
            const uint32_t len = e > b && e - b <= 0xffffffffull ? (uint32_t)(e - b) : 0u, T = len > 2 ? len - 2 : 0u;
            const uint32_t flen0 = len / 3, flen1 = len > 1 ? (len - 1) / 3 : 0u;
            const uint64_t fstart[3] = {0, flen0, (uint64_t)flen0 + flen1};
            if (lane < m) {
                const uint32_t f = lane % 3;
                frame_offsets[m * i + lane] = std::min(ob + (lane / 3) * (uint64_t)T + (f == 0 ? 0 : f == 1 ? fstart[1] : fstart[2]), out_cap);
            }
            if (i == n - 1 && lane == 0) frame_offsets[m * n] = std::min(ob + dirs * (uint64_t)T, out_cap);
            if (ob + dirs * (uint64_t)T > out_cap) continue;
            for (uint32_t t0 = 0; t0 < T; t0 += std::min(kTile, T - t0)) {
                const uint32_t t1 = t0 + std::min(kTile, T - t0);
                const uint8_t *w = seqs + b + t0;
                const uintptr_t a0 = reinterpret_cast<uintptr_t>(w) & ~uintptr_t(15);
                const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(w) - a0);
                const uint32_t chunks = (shift + (t1 - t0) + 2 + 15) / 16;
                wave_sync();  // (the previous window's reads are done)
                // (an aligned 16-byte block holding a byte of the read lies in the same page as that byte)
                if (lane < chunks) window[wave][lane] = reinterpret_cast<const uint4 *>(a0)[lane];
                wave_sync();
                // The runs of this window: forward frame f holds the residues r with 3r + f in [t0, t1), reverse
                // frame g those with p = 3r + g in [T - t1, T - t0) (p = T - 1 - j, the codon start in the reverse
                // complement).  (Every loop over the six runs unrolled: the arrays stay in registers.)
                uint32_t lo[6], pre[7];
                uint64_t start[6];
                pre[0] = 0;
#pragma unroll
                for (uint32_t k = 0; k < 6; ++k) {
                    const bool forward = fwd && k < 3;
                    const uint32_t f = k % 3;
                    const uint32_t x0 = forward ? t0 : T - t1, x1 = forward ? t1 : T - t0;
                    const uint32_t below0 = x0 > f ? (x0 - f + 2) / 3 : 0u, below1 = x1 > f ? (x1 - f + 2) / 3 : 0u;
                    lo[k] = below0;
                    start[k] = ob + (k / 3) * (uint64_t)T + fstart[f];
                    pre[k + 1] = pre[k] + (k < m ? below1 - below0 : 0u);
                }
                for (uint32_t q = lane; q < pre[6]; q += kWave) {
                    uint32_t k = 0, r = 0;
                    uint64_t at_out = 0;
#pragma unroll
                    for (uint32_t kk = 0; kk < 6; ++kk)
                        if (q >= pre[kk] && q < pre[kk + 1]) k = kk, r = lo[kk] + (q - pre[kk]), at_out = start[kk] + r;
                    const uint32_t f = k % 3;
                    const bool forward = fwd && k < 3;
                    const uint32_t jj = forward ? 3 * r + f : T - 1 - (3 * r + f);
                    const uint32_t at = shift + (jj - t0);
                    const uint32_t c0 = nclass[win[at]], c1 = nclass[win[at + 1]], c2 = nclass[win[at + 2]];
                    const uint32_t idx = forward ? c0 << 8 | c1 << 4 | c2 : bitrev4(c2) << 8 | bitrev4(c1) << 4 | bitrev4(c0);
                    out[at_out] = codon[idx];
                }
            }
        }
    }
}

// One wavefront per 64 reads: lane l decides for read 64 g + l among its m frames, then the wave copies the winning
// frames' rows, 64 row slots at a time.
__global__ __launch_bounds__(kBlock) void frame_select_kernel(uint64_t n, uint32_t m, uint32_t keep, uint32_t kmer_size,
                                                              uint32_t first_frame,
                                                              const uint64_t *__restrict__ frame_offsets,
                                                              const epik_amd_placement *__restrict__ f_rows,
                                                              const uint32_t *__restrict__ f_n_rows,
                                                              const uint32_t *__restrict__ f_counts,
                                                              epik_amd_placement *__restrict__ rows,
                                                              uint32_t *__restrict__ n_rows, uint32_t *__restrict__ counts,
                                                              uint8_t *__restrict__ frame)
{
    // (the winners go through LDS, not __shfl: in the copy loop below the lane that decided may be inactive)
    __shared__ uint32_t s_win[kBlockWaves][kWave], s_copy[kBlockWaves][kWave];
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const uint64_t groups = (n + kWave - 1) / kWave, waves = (uint64_t)gridDim.x * kBlockWaves;
    for (uint64_t g = (uint64_t)blockIdx.x * kBlockWaves + wave; g < groups; g += waves) {
        const uint64_t first = g * kWave, i = first + lane;
        uint32_t win = 0, copy = 0;
        if (i < n) {
            bool narrow = false;
            int best = -1;
            float best_key = 0.0f;
            for (uint32_t w = 0; w < m; ++w) {
                const uint64_t fr = m * i + w;
                const uint32_t nr = f_n_rows[fr];
                narrow |= nr == EPIK_AMD_ROWS_COUNTS_TOO_NARROW;
                if (!has_rows(nr)) continue;
                const uint64_t len = frame_offsets[fr + 1] - frame_offsets[fr];  // (rows: at least k residues)
                const float key = __fdiv_rn(f_rows[fr * keep].score, (float)(len - kmer_size + 1));
                if (best < 0 || key > best_key) best = (int)w, best_key = key;
            }
            if (narrow) {
                n_rows[i] = EPIK_AMD_ROWS_COUNTS_TOO_NARROW;
            } else if (best < 0) {
                n_rows[i] = f_n_rows[m * i];
            } else {
                win = (uint32_t)best;
                copy = f_n_rows[m * i + win];
                n_rows[i] = copy;
            }
            if (frame) frame[i] = (uint8_t)(first_frame + win);
        }
        wave_sync();  // (the previous group's reads of s_win / s_copy are done)
        s_win[wave][lane] = win;
        s_copy[wave][lane] = std::min(copy, keep);
        wave_sync();
        const uint64_t slots = std::min<uint64_t>(kWave, n - first) * keep;
        for (uint64_t s = lane; s < slots; s += kWave) {
            const uint32_t l = (uint32_t)(s / keep), t = (uint32_t)(s % keep);
            const uint32_t w = s_win[wave][l], c = s_copy[wave][l];
            if (t >= c) continue;
            const uint64_t src = (m * (first + l) + w) * keep + t;
            rows[first * keep + s] = f_rows[src];
            if (counts) counts[first * keep + s] = f_counts[src];
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------

uint32_t frames_of(uint32_t mode) { return mode == EPIK_AMD_FRAMES_BOTH ? 6 : 3; }

int scan_temp_bytes(uint64_t items, size_t &bytes)
{
    bytes = 0;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, static_cast<const uint64_t *>(nullptr),
                                                          static_cast<uint64_t *>(nullptr), (size_t)items);
    if (e != hipSuccess) return fail_with(EPIK_AMD_ERR_HIP, std::string("hipcub scan size: ") + hipGetErrorString(e));
    return EPIK_AMD_OK;
}

// the workspace: per-read and per-frame arrays, then the frame bytes
struct WorkspaceLayout {
    uint64_t totals = 0, base = 0, scan = 0, frame_offsets = 0, rows = 0, n_rows = 0, counts = 0, seqs = 0;  // byte offsets
    uint64_t scan_bytes = 0;
};
int layout_of(uint64_t n, uint32_t keep, uint32_t mode, WorkspaceLayout &l)
{
    const uint64_t m = frames_of(mode);
    size_t scan = 0;
    if (const int rc = scan_temp_bytes(n + 1, scan); rc != EPIK_AMD_OK) return rc;
    l.totals = 0;
    l.base = align_up((n + 1) * sizeof(uint64_t));
    l.scan = l.base + align_up((n + 1) * sizeof(uint64_t));
    l.scan_bytes = scan;
    l.frame_offsets = l.scan + align_up(scan);
    l.rows = l.frame_offsets + align_up((m * n + 1) * sizeof(uint64_t));
    l.n_rows = l.rows + align_up(m * n * keep * sizeof(epik_amd_placement));
    l.counts = l.n_rows + align_up(m * n * sizeof(uint32_t));
    l.seqs = l.counts + align_up(m * n * keep * sizeof(uint32_t));
    return EPIK_AMD_OK;
}
uint64_t frame_bytes(uint64_t seq_bytes, uint32_t mode) { return align_up((mode == EPIK_AMD_FRAMES_BOTH ? 2 : 1) * seq_bytes + 1); }

int check_handle(const epik_amd_placer *p, uint32_t mode)
{
    if (!p) return fail_with(EPIK_AMD_ERR_INVALID, "null placer");
    if (mode > EPIK_AMD_FRAMES_BOTH) return fail_with(EPIK_AMD_ERR_INVALID, "frame mode must be FORWARD, REVERSE or BOTH");
    if (p->params.alphabet_size != 20)
        return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "translated placement needs an amino-acid placer (alphabet_size 20)");
    if (p->plan.shard_count > 1)
        return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "translated placement needs a whole database, not a k-mer-space shard");
    if (p->h_char_class.size() != 256) return fail_with(EPIK_AMD_ERR_INVALID, "placer has no character table");
    if (p->h_char_class['*'] != 0)
        return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "translated placement needs '*' (a stop) to be an invalid character (class 0)");
    return EPIK_AMD_OK;
}

int place_frames_device_impl(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets, uint64_t n,
                             uint32_t mode, void *d_workspace, uint64_t workspace_bytes, void *d_rows, void *d_n_rows,
                             void *d_kmer_counts, void *d_frame, hipStream_t stream)
{
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (n == 0) return EPIK_AMD_OK;
    if (!d_seqs || !d_seq_offsets || !d_rows || !d_n_rows) return fail_with(EPIK_AMD_ERR_INVALID, "null device buffer");
    const uint32_t keep = p->params.keep_at_most, m = frames_of(mode);
    WorkspaceLayout l;
    if (const int rc = layout_of(n, keep, mode, l); rc != EPIK_AMD_OK) return rc;
    if (!d_workspace || workspace_bytes <= l.seqs)
        return fail_with(EPIK_AMD_ERR_INVALID, "workspace smaller than epik_amd_placer_frame_workspace_bytes");
    HIP_TRY(hipSetDevice(p->device));
    const auto *offs = static_cast<const uint64_t *>(d_seq_offsets);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    auto *totals = reinterpret_cast<uint64_t *>(ws + l.totals), *base = reinterpret_cast<uint64_t *>(ws + l.base);
    auto *f_offs = reinterpret_cast<uint64_t *>(ws + l.frame_offsets);
    auto *f_rows = reinterpret_cast<epik_amd_placement *>(ws + l.rows);
    auto *f_n_rows = reinterpret_cast<uint32_t *>(ws + l.n_rows);
    auto *f_counts = d_kmer_counts ? reinterpret_cast<uint32_t *>(ws + l.counts) : nullptr;
    uint8_t *f_seqs = ws + l.seqs;

    hipLaunchKernelGGL(frame_length_kernel, dim3(grid_for((n + 1 + kWave - 1) / kWave, kMaxBlocks)), dim3(kBlock), 0, stream,
                       offs, n, totals);
    HIP_TRY(hipGetLastError());
    size_t scan_bytes = l.scan_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(ws + l.scan, scan_bytes, static_cast<const uint64_t *>(totals), base,
                                             (size_t)(n + 1), stream));
    hipLaunchKernelGGL(translate_kernel, dim3(grid_for((n + kWave - 1) / kWave, kMaxBlocks)), dim3(kBlock), 0, stream,
                       static_cast<const uint8_t *>(d_seqs), offs, n, static_cast<const uint64_t *>(base), mode, f_seqs,
                       workspace_bytes - l.seqs, f_offs);
    HIP_TRY(hipGetLastError());
    if (const int rc = epik_amd_placer_place_device(p, f_seqs, f_offs, m * n, f_rows, f_n_rows, f_counts, stream);
        rc != EPIK_AMD_OK)
        return rc;
    hipLaunchKernelGGL(frame_select_kernel, dim3(grid_for((n + kWave - 1) / kWave, kMaxBlocks)), dim3(kBlock), 0, stream,
                       n, m, keep, p->params.kmer_size, mode == EPIK_AMD_FRAMES_REVERSE ? 3u : 0u,
                       static_cast<const uint64_t *>(f_offs), static_cast<const epik_amd_placement *>(f_rows),
                       static_cast<const uint32_t *>(f_n_rows), static_cast<const uint32_t *>(f_counts),
                       static_cast<epik_amd_placement *>(d_rows), static_cast<uint32_t *>(d_n_rows),
                       static_cast<uint32_t *>(d_kmer_counts), static_cast<uint8_t *>(d_frame));
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

constexpr HostVariant kFrameHost{.chunk_reads = 1u << 17, .chunk_bytes = 32u << 20, .chunk_reads_env = "EPIK_AMD_FRAME_CHUNK_READS",
                                 .workspace_bytes = epik_amd_placer_frame_workspace_bytes,
                                 .zeroed_bytes = nullptr, .place_device = place_frames_device_impl};

int place_frames_impl(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n, uint32_t mode,
                      epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts, uint8_t *frame)
{
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (n == 0) return EPIK_AMD_OK;
    uint64_t longest = 0;
    if (const int rc = check_host_batch(seqs, seq_offsets, n, rows, n_rows, longest); rc != EPIK_AMD_OK) return rc;
    // (the count width from the batch's longest FRAME: frame +1 of its longest read)
    return place_host_chunked(p, seqs, seq_offsets, n, mode, longest / 3, kFrameHost, rows, n_rows, kmer_counts, frame);
}

// the same placement with the rows left on the device and summed into a profile there (profile_place.hip)
int profile_frames_impl(epik_amd_placer *p, epik_amd_profile *profile, const char *seqs, const uint64_t *seq_offsets,
                        const uint32_t *weights, uint64_t n, uint32_t mode, uint8_t *frame)
{
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (!profile) return fail_with(EPIK_AMD_ERR_INVALID, "null profile");
    if (n == 0) return EPIK_AMD_OK;
    uint64_t longest = 0;
    if (const int rc = check_host_reads(seqs, seq_offsets, n, longest); rc != EPIK_AMD_OK) return rc;
    return profile_host_chunked(p, profile, seqs, seq_offsets, weights, n, mode, longest / 3, kFrameHost, frame);
}

}  // namespace

extern "C" {

int epik_amd_codon_table(uint8_t *out)
{
    if (!out) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    std::memcpy(out, kCodonTable.v, sizeof kCodonTable.v);
    return EPIK_AMD_OK;
}

int epik_amd_placer_frame_workspace_bytes(const epik_amd_placer *p, uint64_t n, uint64_t seq_bytes, uint32_t mode,
                                          uint64_t *bytes)
{
    if (!bytes) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    *bytes = 0;
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (n == 0) return EPIK_AMD_OK;
    WorkspaceLayout l;
    if (const int rc = layout_of(n, p->params.keep_at_most, mode, l); rc != EPIK_AMD_OK) return rc;
    *bytes = l.seqs + frame_bytes(seq_bytes, mode);
    return EPIK_AMD_OK;
}

int epik_amd_placer_place_frames_device(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets, uint64_t n,
                                        uint32_t mode, void *d_workspace, uint64_t workspace_bytes, void *d_rows,
                                        void *d_n_rows, void *d_kmer_counts, void *d_frame, void *stream)
{
    return place_frames_device_impl(p, d_seqs, d_seq_offsets, n, mode, d_workspace, workspace_bytes, d_rows, d_n_rows,
                                    d_kmer_counts, d_frame, static_cast<hipStream_t>(stream));
}

int epik_amd_placer_place_frames(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                 uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                 uint8_t *frame)
{
    try {  // std::vector: nothing may leave through the C ABI
        return place_frames_impl(p, seqs, seq_offsets, n, mode, rows, n_rows, kmer_counts, frame);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("place_frames: ") + e.what());
    }
}

int epik_amd_placer_profile_frames(epik_amd_placer *p, epik_amd_profile *profile, const char *seqs,
                                   const uint64_t *seq_offsets, const uint32_t *weights, uint64_t n, uint32_t mode,
                                   uint8_t *frame)
{
    try {
        return profile_frames_impl(p, profile, seqs, seq_offsets, weights, n, mode, frame);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("profile_frames: ") + e.what());
    }
}

int epik_amd_placer_cohort_frames(epik_amd_placer *p, epik_amd_cohort *cohort, const char *seqs, const uint64_t *seq_offsets,
                                   const uint32_t *weights, const uint32_t *samples, uint64_t n, uint32_t mode, uint8_t *frame)
{
    try {  // (profile_frames with a row of cells per sample: cohort_place.hip)
        if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
        if (!cohort) return fail_with(EPIK_AMD_ERR_INVALID, "null cohort");
        if (n == 0) return EPIK_AMD_OK;
        uint64_t longest = 0;
        if (const int rc = check_host_reads(seqs, seq_offsets, n, longest); rc != EPIK_AMD_OK) return rc;
        return cohort_host_chunked(p, cohort, seqs, seq_offsets, weights, samples, n, mode, longest / 3, kFrameHost, frame);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("cohort_frames: ") + e.what());
    }
}

int epik_amd_placer_confidence_frames(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                        uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                        uint8_t *frame, const epik_amd_tree *tree, uint32_t tau_q, epik_amd_confidence *conf,
                                        epik_amd_profile *profile, const uint32_t *weights)
{
    try {  // (place_frames with the confidence records of confidence_place.hip computed from each chunk's device rows)
        if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
        if (n == 0) return EPIK_AMD_OK;
        uint64_t longest = 0;
        if (const int rc = check_host_reads(seqs, seq_offsets, n, longest); rc != EPIK_AMD_OK) return rc;
        return confidence_host_chunked(p, ConfidenceRequest{tree, tau_q, conf, profile, weights}, seqs, seq_offsets, n, mode,
                                       longest / 3, kFrameHost, rows, n_rows, kmer_counts, frame);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("confidence_frames: ") + e.what());
    }
}

int epik_amd_placer_taxa_frames(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n,
                                        uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                                        uint8_t *frame, epik_amd_taxonomy *taxonomy, uint32_t tau_q,
        epik_amd_taxon_record *records, const uint32_t *weights, const uint32_t *samples, epik_amd_profile *profile,
        epik_amd_cohort *cohort)
{
    try {  // (the same with the taxonomic assignment of taxa_place.hip run on each chunk's device rows)
        if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
        if (n == 0) return EPIK_AMD_OK;
        uint64_t longest = 0;
        if (const int rc = check_host_reads(seqs, seq_offsets, n, longest); rc != EPIK_AMD_OK) return rc;
        return taxa_host_chunked(p, TaxaRequest{taxonomy, tau_q, records, weights, samples, profile, cohort}, seqs, seq_offsets, n, mode,
                                       longest / 3, kFrameHost, rows, n_rows, kmer_counts, frame);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("taxa_frames: ") + e.what());
    }
}

}  // extern "C"
