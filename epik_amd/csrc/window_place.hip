// window_place.hip -- long sequences painted by windows: epik_amd_placer_window_workspace_bytes,
// epik_amd_placer_place_windows_device, epik_amd_placer_place_windows, epik_amd_windows_paint_device and
// epik_amd_windows_paint_host (include/epik_amd.h, where the geometry and the rule are stated once).
//
// No reference counterpart: the reference places a query as one unit.  SHERPAS slides a window along the
// query on the CPU; here the windows of a batch are cut on the device and placed as reads of their own.
//
// Device side of the placement: epik_amd_placer_place_strands_device, unchanged, called ONCE over all the windows of
// the batch (epik_amd_placer_place_device for an amino-acid handle, which takes FORWARD only).  Around it:
//   window_count_kernel  per read its windows and their bytes (epik_amd_window_span);
//   (hipCUB)             the exclusive sums of both: win_offsets, and where each read's windows start;
//   window_cut_kernel    the windows' bytes and offsets into the workspace, a wave per read.
// Overlapping windows look every k-mer up about W / S times: an incremental sliding accumulate is another kernel.
//
// Painting: window_paint_kernel, a wave per read over tiles of 64 windows.  Lane l holds window 64 t + l and finds its
// call in two passes over the window's rows: a weighted majority vote (more than half of S is asked for, so the only
// group that can qualify is the vote's candidate), then the candidate's mass; no table of groups.  The segments of the
// tile come from the ballot of the lanes whose call differs from the window before (head flags), the sums of a run from
// a wave prefix sum, and the run left open at the end of a tile is carried into the next one in wave-uniform registers:
// that tile closes it, with its own windows added when its first window goes on with the same call.
// One record, one segment slot and one n_segments have one writer each.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint64_t kMaxBlocks = 4096;
constexpr uint32_t kLwrBits = EPIK_AMD_PROFILE_LWR_BITS;
static_assert(sizeof(epik_amd_window_record) == 16 && sizeof(epik_amd_window_segment) == 32 && sizeof(epik_amd_placement) == 16);

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the header's inline geometry is an export of the library too: its address taken, so that the host's copy is emitted
[[gnu::used]] uint64_t (*const kWindowSpanExport)(uint64_t, uint32_t, uint32_t, uint64_t, uint64_t *, uint64_t *) = &epik_amd_window_span;

// ---- cutting ----------------------------------------------------------------------------------------------------

// per read its windows and the bytes they take together; slot n gets 0 (the exclusive sums' last slot is the total)
__global__ __launch_bounds__(kBlock) void window_count_kernel(const uint64_t *__restrict__ seq_offsets, uint64_t n,
                                                              uint32_t window, uint32_t step, uint64_t *__restrict__ counts,
                                                              uint64_t *__restrict__ bytes)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * kBlock) {
        uint64_t nw = 0, len = 0;
        if (i < n) {
            const uint64_t b = seq_offsets[i], e = seq_offsets[i + 1];
            len = e > b ? e - b : 0;
            nw = epik_amd_window_span(len, window, step, 0, nullptr, nullptr);
        }
        counts[i] = nw;
        bytes[i] = nw * std::min<uint64_t>(len, window);
    }
}

// A wave per read: window w of the read goes to out[byte_base + w * wl, + wl), wl = min(L, W), and its offset to
// w_offsets[win_base + w]; the wave of the last read also closes the offsets.  Nothing is written for a window whose
// index or bytes lie beyond the totals the caller sized the workspace for (max_windows, out_cap).
__global__ __launch_bounds__(kBlock) void window_cut_kernel(const uint8_t *__restrict__ seqs,
                                                            const uint64_t *__restrict__ seq_offsets, uint64_t n,
                                                            uint32_t window, uint32_t step,
                                                            const uint64_t *__restrict__ win_base,
                                                            const uint64_t *__restrict__ byte_base, uint64_t max_windows,
                                                            uint8_t *__restrict__ out, uint64_t out_cap,
                                                            uint64_t *__restrict__ w_offsets)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t waves = (uint64_t)gridDim.x * kBlockWaves;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlockWaves + threadIdx.x / kWave; i < n; i += waves) {
        const uint64_t b = seq_offsets[i], e = seq_offsets[i + 1], len = e > b ? e - b : 0;
        const uint64_t wl = std::min<uint64_t>(len, window);
        const uint64_t nw = epik_amd_window_span(len, window, step, 0, nullptr, nullptr);
        const uint64_t w0 = win_base[i], o0 = byte_base[i];
        for (uint64_t w = lane; w < nw; w += kWave)
            if (w0 + w < max_windows) w_offsets[w0 + w] = std::min(o0 + w * wl, out_cap);
        if (i == n - 1 && lane == 0) w_offsets[std::min(w0 + nw, max_windows)] = std::min(o0 + nw * wl, out_cap);
        for (uint64_t w = 0; w < nw; ++w) {
            if (w0 + w >= max_windows || o0 + (w + 1) * wl > out_cap) break;
            uint64_t begin = 0;
            (void)epik_amd_window_span(len, window, step, w, &begin, nullptr);
            const uint8_t *src = seqs + b + begin;
            uint8_t *dst = out + o0 + w * wl;
            for (uint64_t t = lane; t < wl; t += kWave) dst[t] = src[t];
        }
    }
}

// ---- painting ---------------------------------------------------------------------------------------------------

// mass * 2^30 >= tau_q * total, as 128-bit integers (taxa_place.hip's comparison)
__device__ inline bool qualifies(uint64_t mass, uint32_t tau_q, uint64_t total)
{
    const uint64_t l_hi = mass >> (64 - kLwrBits), l_lo = mass << kLwrBits;
    const uint64_t r_hi = __umul64hi((uint64_t)tau_q, total), r_lo = (uint64_t)tau_q * total;
    return l_hi > r_hi || (l_hi == r_hi && l_lo >= r_lo);
}

__device__ inline uint64_t q_of(const u32x4 &row)
{
    return (uint64_t)__double2ll_rn(__hiloint2double((int)row.w, (int)row.z) * (double)(1u << kLwrBits));
}

// inclusive prefix sum over the wave
__device__ inline uint64_t wave_prefix(uint64_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < kWave; d <<= 1) {
        const uint64_t up = __shfl_up((unsigned long long)v, d);
        if (lane >= d) v += up;
    }
    return v;
}

__global__ __launch_bounds__(kBlock) void window_paint_kernel(const u32x4 *__restrict__ rows, const uint32_t *__restrict__ n_rows,
                                                              const uint32_t *__restrict__ kmer_counts,
                                                              const uint64_t *__restrict__ win_offsets, uint64_t n,
                                                              uint64_t num_windows, uint32_t keep,
                                                              const uint32_t *__restrict__ group, uint32_t num_branches,
                                                              uint32_t tau_q, u32x4 *__restrict__ records,
                                                              epik_amd_window_segment *__restrict__ segments,
                                                              uint32_t *__restrict__ n_segments)
{
    const uint32_t lane = threadIdx.x % kWave;
    const uint64_t waves = (uint64_t)gridDim.x * kBlockWaves;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlockWaves + threadIdx.x / kWave; i < n; i += waves) {
        const uint64_t v0 = std::min(win_offsets[i], num_windows), v1 = std::min(win_offsets[i + 1], num_windows);
        const uint64_t nw = v1 > v0 ? v1 - v0 : 0;
        // the run open at the end of the tile before: wave-uniform
        uint32_t carry_call = 0, started = 0;
        uint64_t carry_first = 0, carry_mass = 0, carry_total = 0;
        for (uint64_t t0 = 0; t0 < nw; t0 += kWave) {
            const bool live = t0 + lane < nw;
            const uint64_t v = v0 + t0 + lane;
            uint32_t call = 0, first_group = 0;
            uint64_t mass = 0, total = 0;
            if (live) {
                const uint32_t raw_nr = n_rows[v];
                const u32x4 *mine = rows + v * keep;
                if (raw_nr == EPIK_AMD_ROWS_COUNTS_TOO_NARROW) {
                    call = EPIK_AMD_WINDOW_TOO_NARROW;
                } else if (raw_nr == 0) {
                    call = EPIK_AMD_WINDOW_TOO_SHORT;
                } else if (kmer_counts[v * keep] == 0) {
                    call = EPIK_AMD_WINDOW_NO_HIT;
                } else {
                    const uint32_t nr = std::min(raw_nr, keep);
                    // the vote: the candidate holds `lead` more than everything else met so far
                    uint32_t cand = EPIK_AMD_WINDOW_NO_GROUP;
                    uint64_t lead = 0;
                    bool bad = false;
                    for (uint32_t j = 0; j < nr; ++j) {
                        const u32x4 row = mine[j];
                        if (row.x >= num_branches) {
                            bad = true;
                            break;
                        }
                        const uint32_t g = group[row.x];
                        const uint64_t q = q_of(row);
                        if (j == 0) first_group = g;
                        total += q;
                        if (g == cand)
                            lead += q;
                        else if (q > lead)
                            cand = g, lead = q - lead;
                        else
                            lead -= q;
                    }
                    if (bad) {
                        call = EPIK_AMD_WINDOW_BAD_ROW;
                    } else if (total == 0) {
                        call = EPIK_AMD_WINDOW_NO_MASS;
                    } else {
                        if (cand != EPIK_AMD_WINDOW_NO_GROUP)
                            for (uint32_t j = 0; j < nr; ++j) {
                                const u32x4 row = mine[j];
                                if (group[row.x] == cand) mass += q_of(row);
                            }
                        call = cand != EPIK_AMD_WINDOW_NO_GROUP && qualifies(mass, tau_q, total) ? cand : EPIK_AMD_WINDOW_AMBIGUOUS;
                    }
                }
                const bool called = call < EPIK_AMD_WINDOW_AMBIGUOUS;
                if (!called) mass = 0, total = 0, first_group = 0;
                if (records) {
                    const u32x4 rec = {call, mass > 0xffffffffull ? 0xffffffffu : (uint32_t)mass, first_group,
                                       total > 0xffffffffull ? 0xffffffffu : (uint32_t)total};
                    records[v] = rec;
                }
            }
            if (!segments && !n_segments) continue;
            // head flags: a window whose call differs from the one before it in the read
            uint32_t before = __shfl_up(call, 1);
            if (lane == 0) before = carry_call;
            const bool head = live && ((t0 == 0 && lane == 0) || call != before);
            const unsigned long long heads = __ballot(head), lives = __ballot(live);
            const uint32_t last = 63u - (uint32_t)__builtin_clzll(lives);  // (lives != 0: t0 < nw)
            const unsigned long long below = heads & (~0ull >> (63u - lane));  // the heads at or below my lane
            const uint64_t pre_mass = wave_prefix(mass, lane), pre_total = wave_prefix(total, lane);
            const bool continued = below == 0;  // my run came in from the tile before
            const uint32_t start = continued ? 0u : 63u - (uint32_t)__builtin_clzll(below);
            const uint64_t skip_mass = __shfl((unsigned long long)pre_mass, (int)(start ? start - 1 : 0));
            const uint64_t skip_total = __shfl((unsigned long long)pre_total, (int)(start ? start - 1 : 0));
            const uint64_t run_mass = pre_mass - (start ? skip_mass : 0) + (continued ? carry_mass : 0);
            const uint64_t run_total = pre_total - (start ? skip_total : 0) + (continued ? carry_total : 0);
            const uint64_t run_first = continued ? carry_first : t0 + start;
            const uint32_t slot = started + (uint32_t)__popcll(below) - 1u;  // (continued: the run the carry opened)
            const bool ends = live && (lane == last || ((heads >> 1 >> lane) & 1ull));
            const bool open = lane == last && t0 + kWave < nw;  // the read goes on: the next tile closes it
            if (t0 != 0 && lane == 0 && head && segments) {  // the run the tile before left open ends with that tile
                epik_amd_window_segment seg;
                seg.call = carry_call, seg.first_window = (uint32_t)carry_first, seg.num_windows = (uint32_t)(t0 - carry_first);
                seg.reserved = 0, seg.call_mass = carry_mass, seg.total = carry_total;
                segments[v0 + started - 1] = seg;
            }
            if (ends && !open && segments) {
                epik_amd_window_segment seg;
                seg.call = call, seg.first_window = (uint32_t)run_first, seg.num_windows = (uint32_t)(t0 + lane + 1 - run_first);
                seg.reserved = 0, seg.call_mass = run_mass, seg.total = run_total;
                segments[v0 + slot] = seg;
            }
            started += (uint32_t)__popcll(heads);
            carry_call = __shfl(call, (int)last);
            carry_first = __shfl((unsigned long long)run_first, (int)last);
            carry_mass = __shfl((unsigned long long)run_mass, (int)last);
            carry_total = __shfl((unsigned long long)run_total, (int)last);
        }
        if (n_segments && lane == 0) n_segments[i] = started;
    }
}

// ---- host side of the placement ---------------------------------------------------------------------------------

int scan_temp_bytes(uint64_t items, size_t &bytes)
{
    bytes = 0;
    const hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, static_cast<const uint64_t *>(nullptr),
                                                          static_cast<uint64_t *>(nullptr), (size_t)items);
    if (e != hipSuccess) return fail_with(EPIK_AMD_ERR_HIP, std::string("hipcub scan size: ") + hipGetErrorString(e));
    return EPIK_AMD_OK;
}

// amino-acid handles go straight to the placement (FORWARD only); nucleotide ones through the strand placement
bool through_strands(const epik_amd_placer *p, uint32_t mode) { return p->params.alphabet_size == 4 || mode != EPIK_AMD_STRAND_FORWARD; }

int check_handle(const epik_amd_placer *p, uint32_t mode)
{
    if (!p) return fail_with(EPIK_AMD_ERR_INVALID, "null placer");
    if (mode > EPIK_AMD_STRAND_BOTH) return fail_with(EPIK_AMD_ERR_INVALID, "strand mode must be FORWARD, REVERSE or BOTH");
    if (p->plan.shard_count > 1)
        return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "windowed placement needs a whole database, not a k-mer-space shard");
    if (through_strands(p, mode)) {  // (the strand placement's own check, in its words)
        uint64_t bytes = 0;
        return epik_amd_placer_strand_workspace_bytes(p, 0, 0, mode, &bytes);
    }
    return EPIK_AMD_OK;
}

int check_geometry(const epik_amd_placer *p, uint32_t window, uint32_t step)
{
    if (window < p->params.kmer_size || window >= 0x80000000u)
        return fail_with(EPIK_AMD_ERR_INVALID, "the window must hold a k-mer and be shorter than 2^31 (k <= window < 2^31)");
    if (step == 0 || step > window) return fail_with(EPIK_AMD_ERR_INVALID, "the window step must lie in [1, window]");
    return EPIK_AMD_OK;
}

// the workspace: per-read arrays, the scan's scratch, the windows' offsets, the strand placement's workspace, the windows' bytes
struct WorkspaceLayout {
    uint64_t counts = 0, bytes = 0, win_base = 0, byte_base = 0, scan = 0, w_offsets = 0, strand = 0, seqs = 0, end = 0;  // byte offsets
    uint64_t scan_bytes = 0, strand_bytes = 0;
};
int layout_of(const epik_amd_placer *p, uint64_t n, uint64_t num_windows, uint64_t window_bytes, uint32_t mode, WorkspaceLayout &l)
{
    size_t scan = 0;
    if (const int rc = scan_temp_bytes(n + 1, scan); rc != EPIK_AMD_OK) return rc;
    const uint64_t per_read = align_up((n + 1) * sizeof(uint64_t));
    l.counts = 0, l.bytes = per_read, l.win_base = 2 * per_read, l.byte_base = 3 * per_read, l.scan = 4 * per_read;
    l.scan_bytes = scan;
    l.w_offsets = l.scan + align_up(scan);
    l.strand = l.w_offsets + align_up((num_windows + 1) * sizeof(uint64_t));
    if (through_strands(p, mode))
        if (const int rc = epik_amd_placer_strand_workspace_bytes(p, num_windows, window_bytes, mode, &l.strand_bytes); rc != EPIK_AMD_OK)
            return rc;
    l.seqs = l.strand + align_up(l.strand_bytes);
    l.end = l.seqs + align_up(window_bytes + 1);
    return EPIK_AMD_OK;
}

int place_windows_device_impl(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets, uint64_t n, uint32_t window,
                              uint32_t step, uint32_t mode, uint64_t num_windows, uint64_t window_bytes, void *d_workspace,
                              uint64_t workspace_bytes, void *d_rows, void *d_n_rows, void *d_kmer_counts, void *d_strand,
                              void *d_win_offsets, hipStream_t stream)
{
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (const int rc = check_geometry(p, window, step); rc != EPIK_AMD_OK) return rc;
    if (n == 0) return EPIK_AMD_OK;
    if (!d_seqs || !d_seq_offsets || !d_rows || !d_n_rows) return fail_with(EPIK_AMD_ERR_INVALID, "null device buffer");
    if (num_windows < n) return fail_with(EPIK_AMD_ERR_INVALID, "num_windows is smaller than the batch: every read has a window");
    WorkspaceLayout l;
    if (const int rc = layout_of(p, n, num_windows, window_bytes, mode, l); rc != EPIK_AMD_OK) return rc;
    if (!d_workspace || workspace_bytes < l.end)
        return fail_with(EPIK_AMD_ERR_INVALID, "workspace smaller than epik_amd_placer_window_workspace_bytes");
    HIP_TRY(hipSetDevice(p->device));
    const auto *offs = static_cast<const uint64_t *>(d_seq_offsets);
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    auto *counts = reinterpret_cast<uint64_t *>(ws + l.counts), *bytes = reinterpret_cast<uint64_t *>(ws + l.bytes);
    auto *win_base = d_win_offsets ? static_cast<uint64_t *>(d_win_offsets) : reinterpret_cast<uint64_t *>(ws + l.win_base);
    auto *byte_base = reinterpret_cast<uint64_t *>(ws + l.byte_base);
    auto *w_offsets = reinterpret_cast<uint64_t *>(ws + l.w_offsets);
    uint8_t *w_seqs = ws + l.seqs;

    hipLaunchKernelGGL(window_count_kernel, dim3(grid_for((n + 1 + kWave - 1) / kWave, kMaxBlocks)), dim3(kBlock), 0, stream,
                       offs, n, window, step, counts, bytes);
    HIP_TRY(hipGetLastError());
    size_t scan_bytes = l.scan_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(ws + l.scan, scan_bytes, static_cast<const uint64_t *>(counts), win_base,
                                             (size_t)(n + 1), stream));
    scan_bytes = l.scan_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(ws + l.scan, scan_bytes, static_cast<const uint64_t *>(bytes), byte_base,
                                             (size_t)(n + 1), stream));
    // (a batch whose totals fall short of the caller's leaves offsets unwritten: all of them start at 0)
    HIP_TRY(hipMemsetAsync(w_offsets, 0, (num_windows + 1) * sizeof(uint64_t), stream));
    hipLaunchKernelGGL(window_cut_kernel, dim3(grid_for(n, kMaxBlocks)), dim3(kBlock), 0, stream,
                       static_cast<const uint8_t *>(d_seqs), offs, n, window, step, static_cast<const uint64_t *>(win_base),
                       static_cast<const uint64_t *>(byte_base), num_windows, w_seqs, window_bytes, w_offsets);
    HIP_TRY(hipGetLastError());
    if (through_strands(p, mode))
        return epik_amd_placer_place_strands_device(p, w_seqs, w_offsets, num_windows, mode, l.strand_bytes ? ws + l.strand : nullptr,
                                                    l.strand_bytes, d_rows, d_n_rows, d_kmer_counts, d_strand, stream);
    if (const int rc = epik_amd_placer_place_device(p, w_seqs, w_offsets, num_windows, d_rows, d_n_rows, d_kmer_counts, stream);
        rc != EPIK_AMD_OK)
        return rc;
    if (d_strand) HIP_TRY(hipMemsetAsync(d_strand, 0, num_windows, stream));
    return EPIK_AMD_OK;
}

int check_tau(uint32_t tau_q);
int check_groups(const uint32_t *group, uint32_t num_branches);
void launch_paint(const void *d_rows, const void *d_n_rows, const void *d_kmer_counts, const void *d_win_offsets, uint64_t n,
                  uint64_t num_windows, uint32_t keep, const void *d_group, uint32_t num_branches, uint32_t tau_q, void *d_records,
                  void *d_segments, void *d_n_segments, hipStream_t stream);

// What epik_amd_placer_paint_windows adds to place_windows: every chunk's windows painted on the device from the rows the
// placement left there; group[N] is uploaded once, the records, segments and segment counts are host arrays.
struct PaintRequest {
    const uint32_t *group;
    uint32_t tau_q;
    epik_amd_window_record *records;
    epik_amd_window_segment *segments;
    uint32_t *n_segments;
};

// The host entry: place_host_chunked's loop (host_entry.hpp) with a variable number of outputs per read.  With `paint`,
// rows and n_rows may be NULL as well: that part stays on the device.
int place_windows_impl(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n, uint32_t window,
                       uint32_t step, uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows, uint32_t *kmer_counts,
                       uint8_t *strand, uint64_t *win_offsets, const PaintRequest *paint = nullptr)
{
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (const int rc = check_geometry(p, window, step); rc != EPIK_AMD_OK) return rc;
    const uint32_t num_branches = p->params.num_branches;
    if (paint) {
        if (const int rc = check_tau(paint->tau_q); rc != EPIK_AMD_OK) return rc;
        if (!paint->group) return fail_with(EPIK_AMD_ERR_INVALID, "null host buffer");
        if (const int rc = check_groups(paint->group, num_branches); rc != EPIK_AMD_OK) return rc;
    }
    if (n == 0) {
        if (win_offsets) win_offsets[0] = 0;
        return EPIK_AMD_OK;
    }
    uint64_t longest = 0;
    if (const int rc = paint ? check_host_reads(seqs, seq_offsets, n, longest) : check_host_batch(seqs, seq_offsets, n, rows, n_rows, longest);
        rc != EPIK_AMD_OK)
        return rc;
    // the windows of every read: first[i], and the bytes they take
    std::vector<uint64_t> first(n + 1, 0), wbytes(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t len = seq_offsets[i + 1] - seq_offsets[i];
        const uint64_t nw = epik_amd_window_span(len, window, step, 0, nullptr, nullptr);
        if (nw > EPIK_AMD_WINDOW_MAX_PER_READ)
            return fail_with(EPIK_AMD_ERR_INVALID, "read " + std::to_string(i) + " has " + std::to_string(nw) +
                                                       " windows, more than 2^24: a larger step, or a wider window");
        first[i + 1] = first[i] + nw;
        wbytes[i + 1] = wbytes[i] + nw * std::min<uint64_t>(len, window);
    }
    HIP_TRY(hipSetDevice(p->device));
    const CountWidthGuard width(p, std::min<uint64_t>(longest, window));
    if (width.rc != EPIK_AMD_OK) return width.rc;

    // chunks of whole reads, of at most chunk_windows windows and chunk_bytes window bytes (a larger read: a chunk of its own)
    uint64_t chunk_windows = 1u << 18;
    const uint64_t chunk_bytes = 64u << 20;
    if (const char *e = std::getenv("EPIK_AMD_WINDOW_CHUNK_WINDOWS")) chunk_windows = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
    std::vector<uint64_t> starts{0};
    uint64_t max_reads = 0, max_chars = 0, max_windows = 0, max_wbytes = 0;
    for (uint64_t r0 = 0; r0 < n;) {
        uint64_t r1 = r0 + 1;
        while (r1 < n && first[r1 + 1] - first[r0] <= chunk_windows && wbytes[r1 + 1] - wbytes[r0] <= chunk_bytes) ++r1;
        max_reads = std::max(max_reads, r1 - r0);
        max_chars = std::max(max_chars, seq_offsets[r1] - seq_offsets[r0]);
        max_windows = std::max(max_windows, first[r1] - first[r0]);
        max_wbytes = std::max(max_wbytes, wbytes[r1] - wbytes[r0]);
        starts.push_back(r0 = r1);
    }
    const uint64_t keep = p->params.keep_at_most;
    WorkspaceLayout l;
    if (const int rc = layout_of(p, max_reads, max_windows, max_wbytes, mode, l); rc != EPIK_AMD_OK) return rc;
    // one allocation: seqs | offsets | win_offsets | rows | n_rows | counts | strand | (group | records | segments |
    // n_segments) | workspace
    const uint64_t o_offs = align_up(max_chars + 1), o_wo = o_offs + align_up((max_reads + 1) * sizeof(uint64_t));
    const uint64_t o_rows = o_wo + align_up((max_reads + 1) * sizeof(uint64_t));
    const uint64_t o_nrows = o_rows + align_up(max_windows * keep * sizeof(epik_amd_placement));
    const uint64_t o_counts = o_nrows + align_up(max_windows * sizeof(uint32_t));
    const uint64_t o_strand = o_counts + align_up(max_windows * keep * sizeof(uint32_t));
    const uint64_t o_group = o_strand + align_up(max_windows);
    const uint64_t o_records = o_group + (paint ? align_up(num_branches * sizeof(uint32_t)) : 0);
    const uint64_t o_segments = o_records + (paint ? align_up(max_windows * sizeof(epik_amd_window_record)) : 0);
    const uint64_t o_nsegs = o_segments + (paint ? align_up(max_windows * sizeof(epik_amd_window_segment)) : 0);
    const uint64_t o_ws = o_nsegs + (paint ? align_up(max_reads * sizeof(uint32_t)) : 0);
    struct ChunkBuffers {  // (freed however the call ends, after its stream has drained)
        void *base = nullptr;
        hipStream_t stream = nullptr;
        ~ChunkBuffers()
        {
            if (stream) (void)hipStreamSynchronize(stream);
            if (base) (void)hipFree(base);
        }
    } buf;
    HIP_TRY(hipMalloc(&buf.base, o_ws + l.end));
    buf.stream = p->stream;
    uint8_t *d = static_cast<uint8_t *>(buf.base);
    auto *d_offs = reinterpret_cast<uint64_t *>(d + o_offs), *d_wo = reinterpret_cast<uint64_t *>(d + o_wo);
    auto *d_rows = reinterpret_cast<epik_amd_placement *>(d + o_rows);
    auto *d_nrows = reinterpret_cast<uint32_t *>(d + o_nrows), *d_counts = reinterpret_cast<uint32_t *>(d + o_counts);
    uint8_t *d_strand = d + o_strand, *d_ws = d + o_ws;
    std::vector<uint64_t> offs(max_reads + 1), wo(max_reads + 1);
    if (win_offsets) win_offsets[0] = 0;
    if (paint && num_branches)
        HIP_TRY(hipMemcpyAsync(d + o_group, paint->group, num_branches * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    for (size_t c = 0; c + 1 < starts.size(); ++c) {
        const uint64_t r0 = starts[c], cnt = starts[c + 1] - r0, b0 = seq_offsets[r0], chars = seq_offsets[r0 + cnt] - b0;
        const uint64_t w0 = first[r0], nwin = first[r0 + cnt] - w0, nbytes = wbytes[r0 + cnt] - wbytes[r0];
        for (uint64_t i = 0; i <= cnt; ++i) offs[i] = seq_offsets[r0 + i] - b0;
        if (chars) HIP_TRY(hipMemcpyAsync(d, seqs + b0, chars, hipMemcpyHostToDevice, p->stream));
        HIP_TRY(hipMemcpyAsync(d_offs, offs.data(), (cnt + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
        // rows beyond n_rows are never written by the kernels: zero, as epik_amd_placer_place leaves them -- and so is
        // what a `both` placement keeps of the reverse strand, whose row slots are copied whole where reverse wins
        HIP_TRY(hipMemsetAsync(d_rows, 0, nwin * keep * sizeof(epik_amd_placement), p->stream));
        HIP_TRY(hipMemsetAsync(d_counts, 0, nwin * keep * sizeof(uint32_t), p->stream));
        WorkspaceLayout cl;
        if (const int rc = layout_of(p, cnt, nwin, nbytes, mode, cl); rc != EPIK_AMD_OK) return rc;
        if (cl.strand_bytes) HIP_TRY(hipMemsetAsync(d_ws + cl.strand, 0, cl.strand_bytes, p->stream));
        if (const int rc = place_windows_device_impl(p, d, d_offs, cnt, window, step, mode, nwin, nbytes, d_ws, cl.end, d_rows,
                                                     d_nrows, d_counts, d_strand, d_wo, p->stream);
            rc != EPIK_AMD_OK)
            return rc;
        if (paint) {  // (segment slots beyond n_segments: zero)
            HIP_TRY(hipMemsetAsync(d + o_segments, 0, nwin * sizeof(epik_amd_window_segment), p->stream));
            launch_paint(d_rows, d_nrows, d_counts, d_wo, cnt, nwin, (uint32_t)keep, d + o_group, num_branches, paint->tau_q,
                         d + o_records, d + o_segments, d + o_nsegs, p->stream);
            HIP_TRY(hipGetLastError());
            if (paint->records)
                HIP_TRY(hipMemcpyAsync(paint->records + w0, d + o_records, nwin * sizeof(epik_amd_window_record), hipMemcpyDeviceToHost, p->stream));
            if (paint->segments)
                HIP_TRY(hipMemcpyAsync(paint->segments + w0, d + o_segments, nwin * sizeof(epik_amd_window_segment), hipMemcpyDeviceToHost, p->stream));
            if (paint->n_segments)
                HIP_TRY(hipMemcpyAsync(paint->n_segments + r0, d + o_nsegs, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
        }
        if (rows) HIP_TRY(hipMemcpyAsync(rows + w0 * keep, d_rows, nwin * keep * sizeof(epik_amd_placement), hipMemcpyDeviceToHost, p->stream));
        if (n_rows) HIP_TRY(hipMemcpyAsync(n_rows + w0, d_nrows, nwin * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
        if (kmer_counts)
            HIP_TRY(hipMemcpyAsync(kmer_counts + w0 * keep, d_counts, nwin * keep * sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
        if (strand) HIP_TRY(hipMemcpyAsync(strand + w0, d_strand, nwin, hipMemcpyDeviceToHost, p->stream));
        // (the offsets the device counted, not the host's: what the rows were written by)
        HIP_TRY(hipMemcpyAsync(wo.data(), d_wo, (cnt + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        if (wo[cnt] != nwin) return fail_with(EPIK_AMD_ERR_INVALID, "place_windows: the device counted other windows than the host");
        if (win_offsets)
            for (uint64_t i = 1; i <= cnt; ++i) win_offsets[r0 + i] = w0 + wo[i];
    }
    return EPIK_AMD_OK;
}

// ---- host side of the painting ----------------------------------------------------------------------------------

int check_tau(uint32_t tau_q)
{
    if (tau_q <= (1u << (kLwrBits - 1)) || tau_q > (1u << kLwrBits))
        return fail_with(EPIK_AMD_ERR_INVALID, "tau_q must lie in (2^29, 2^30]: more than half of the mass, at most all of it");
    return EPIK_AMD_OK;
}

int check_groups(const uint32_t *group, uint32_t num_branches)
{
    for (uint32_t b = 0; b < num_branches; ++b)
        if (group[b] >= EPIK_AMD_WINDOW_AMBIGUOUS && group[b] != EPIK_AMD_WINDOW_NO_GROUP)
            return fail_with(EPIK_AMD_ERR_INVALID, "branch " + std::to_string(b) + ": its group id is a status code");
    return EPIK_AMD_OK;
}

void launch_paint(const void *d_rows, const void *d_n_rows, const void *d_kmer_counts, const void *d_win_offsets, uint64_t n,
                  uint64_t num_windows, uint32_t keep, const void *d_group, uint32_t num_branches, uint32_t tau_q, void *d_records,
                  void *d_segments, void *d_n_segments, hipStream_t stream)
{
    hipLaunchKernelGGL(window_paint_kernel, dim3(grid_for(n, kMaxBlocks)), dim3(kBlock), 0, stream,
                       static_cast<const u32x4 *>(d_rows), static_cast<const uint32_t *>(d_n_rows),
                       static_cast<const uint32_t *>(d_kmer_counts), static_cast<const uint64_t *>(d_win_offsets), n, num_windows,
                       keep, static_cast<const uint32_t *>(d_group), num_branches, tau_q, static_cast<u32x4 *>(d_records),
                       static_cast<epik_amd_window_segment *>(d_segments), static_cast<uint32_t *>(d_n_segments));
}

// The rule on the host, worded after the header: the mass of every group a window's rows name, one after the other.
int paint_host_impl(const epik_amd_placement *rows, const uint32_t *n_rows, const uint32_t *kmer_counts, const uint64_t *win_offsets,
                    uint64_t n, uint32_t keep, const uint32_t *group, uint32_t num_branches, uint32_t tau_q,
                    epik_amd_window_record *records, epik_amd_window_segment *segments, uint32_t *n_segments)
{
    if (const int rc = check_tau(tau_q); rc != EPIK_AMD_OK) return rc;
    if (n == 0) return EPIK_AMD_OK;
    if (!rows || !n_rows || !kmer_counts || !win_offsets || !group) return fail_with(EPIK_AMD_ERR_INVALID, "null host buffer");
    if (keep == 0) return fail_with(EPIK_AMD_ERR_INVALID, "keep is 0");
    for (uint64_t i = 0; i < n; ++i)
        if (win_offsets[i + 1] < win_offsets[i]) return fail_with(EPIK_AMD_ERR_INVALID, "win_offsets not monotone");
    if (const int rc = check_groups(group, num_branches); rc != EPIK_AMD_OK) return rc;
    typedef unsigned __int128 u128;
    if (segments) std::memset(segments + win_offsets[0], 0, (win_offsets[n] - win_offsets[0]) * sizeof(epik_amd_window_segment));
    std::vector<uint64_t> q(keep);
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t segs = 0;
        epik_amd_window_segment seg{};
        for (uint64_t v = win_offsets[i]; v < win_offsets[i + 1]; ++v) {
            epik_amd_window_record rec{};
            uint64_t mass = 0, total = 0;
            const epik_amd_placement *mine = rows + v * keep;
            if (n_rows[v] == EPIK_AMD_ROWS_COUNTS_TOO_NARROW) {
                rec.call = EPIK_AMD_WINDOW_TOO_NARROW;
            } else if (n_rows[v] == 0) {
                rec.call = EPIK_AMD_WINDOW_TOO_SHORT;
            } else if (kmer_counts[v * keep] == 0) {
                rec.call = EPIK_AMD_WINDOW_NO_HIT;
            } else {
                const uint32_t nr = std::min(n_rows[v], keep);
                bool bad = false;
                for (uint32_t j = 0; j < nr; ++j) bad |= mine[j].branch >= num_branches;
                if (bad) {
                    rec.call = EPIK_AMD_WINDOW_BAD_ROW;
                } else {
                    for (uint32_t j = 0; j < nr; ++j) total += q[j] = (uint64_t)std::llrint(mine[j].lwr * (double)(1u << kLwrBits));
                    rec.call = total ? EPIK_AMD_WINDOW_AMBIGUOUS : EPIK_AMD_WINDOW_NO_MASS;
                    for (uint32_t j = 0; j < nr && total; ++j) {
                        const uint32_t g = group[mine[j].branch];
                        if (g == EPIK_AMD_WINDOW_NO_GROUP) continue;
                        uint64_t m = 0;
                        for (uint32_t t = 0; t < nr; ++t) m += group[mine[t].branch] == g ? q[t] : 0;
                        if (((u128)m << kLwrBits) >= (u128)tau_q * total) rec.call = g, mass = m;
                    }
                }
            }
            if (rec.call < EPIK_AMD_WINDOW_AMBIGUOUS) {
                rec.call_mass_q = (uint32_t)std::min<uint64_t>(mass, 0xffffffffull);
                rec.first_group = group[mine[0].branch];
                rec.total_q = (uint32_t)std::min<uint64_t>(total, 0xffffffffull);
            } else {
                mass = total = 0;
            }
            if (records) records[v] = rec;
            const uint64_t w = v - win_offsets[i];
            if (w == 0 || rec.call != seg.call) {
                if (w && segments) segments[win_offsets[i] + segs - 1] = seg;
                seg = epik_amd_window_segment{rec.call, (uint32_t)w, 0, 0, 0, 0};
                ++segs;
            }
            ++seg.num_windows, seg.call_mass += mass, seg.total += total;
        }
        if (segs && segments) segments[win_offsets[i] + segs - 1] = seg;
        if (n_segments) n_segments[i] = segs;
    }
    return EPIK_AMD_OK;
}

}  // namespace

extern "C" {

int epik_amd_placer_window_workspace_bytes(const epik_amd_placer *p, uint64_t n, uint64_t num_windows, uint64_t window_bytes,
                                           uint32_t mode, uint64_t *bytes)
{
    if (!bytes) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    *bytes = 0;
    if (const int rc = check_handle(p, mode); rc != EPIK_AMD_OK) return rc;
    if (n == 0) return EPIK_AMD_OK;
    WorkspaceLayout l;
    if (const int rc = layout_of(p, n, num_windows, window_bytes, mode, l); rc != EPIK_AMD_OK) return rc;
    *bytes = l.end;
    return EPIK_AMD_OK;
}

int epik_amd_placer_place_windows_device(epik_amd_placer *p, const void *d_seqs, const void *d_seq_offsets, uint64_t n,
                                         uint32_t window, uint32_t step, uint32_t mode, uint64_t num_windows,
                                         uint64_t window_bytes, void *d_workspace, uint64_t workspace_bytes, void *d_rows,
                                         void *d_n_rows, void *d_kmer_counts, void *d_strand, void *d_win_offsets, void *stream)
{
    return place_windows_device_impl(p, d_seqs, d_seq_offsets, n, window, step, mode, num_windows, window_bytes, d_workspace,
                                     workspace_bytes, d_rows, d_n_rows, d_kmer_counts, d_strand, d_win_offsets,
                                     static_cast<hipStream_t>(stream));
}

int epik_amd_placer_place_windows(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n, uint32_t window,
                                  uint32_t step, uint32_t mode, epik_amd_placement *rows, uint32_t *n_rows,
                                  uint32_t *kmer_counts, uint8_t *strand, uint64_t *win_offsets)
{
    try {  // std::vector: nothing may leave through the C ABI
        return place_windows_impl(p, seqs, seq_offsets, n, window, step, mode, rows, n_rows, kmer_counts, strand, win_offsets);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("place_windows: ") + e.what());
    }
}

int epik_amd_windows_paint_device(int device, const void *d_rows, const void *d_n_rows, const void *d_kmer_counts,
                                  const void *d_win_offsets, uint64_t n, uint64_t num_windows, uint32_t keep, const void *d_group,
                                  uint32_t num_branches, uint32_t tau_q, void *d_records, void *d_segments, void *d_n_segments,
                                  void *stream)
{
    if (const int rc = check_tau(tau_q); rc != EPIK_AMD_OK) return rc;
    if (n == 0) return EPIK_AMD_OK;
    if (!d_rows || !d_n_rows || !d_kmer_counts || !d_win_offsets || !d_group) return fail_with(EPIK_AMD_ERR_INVALID, "null device buffer");
    if (keep == 0) return fail_with(EPIK_AMD_ERR_INVALID, "keep is 0");
    HIP_TRY(hipSetDevice(device));
    launch_paint(d_rows, d_n_rows, d_kmer_counts, d_win_offsets, n, num_windows, keep, d_group, num_branches, tau_q, d_records,
                 d_segments, d_n_segments, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

int epik_amd_placer_paint_windows(epik_amd_placer *p, const char *seqs, const uint64_t *seq_offsets, uint64_t n, uint32_t window,
                                  uint32_t step, uint32_t mode, const uint32_t *group, uint32_t tau_q, epik_amd_placement *rows,
                                  uint32_t *n_rows, uint32_t *kmer_counts, uint8_t *strand, uint64_t *win_offsets,
                                  epik_amd_window_record *records, epik_amd_window_segment *segments, uint32_t *n_segments)
{
    try {  // (place_windows with every chunk's windows painted on the device from the rows left there)
        const PaintRequest paint{group, tau_q, records, segments, n_segments};
        return place_windows_impl(p, seqs, seq_offsets, n, window, step, mode, rows, n_rows, kmer_counts, strand, win_offsets, &paint);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("paint_windows: ") + e.what());
    }
}

int epik_amd_windows_paint_host(const epik_amd_placement *rows, const uint32_t *n_rows, const uint32_t *kmer_counts,
                                const uint64_t *win_offsets, uint64_t n, uint32_t keep, const uint32_t *group, uint32_t num_branches,
                                uint32_t tau_q, epik_amd_window_record *records, epik_amd_window_segment *segments,
                                uint32_t *n_segments)
{
    try {
        return paint_host_impl(rows, n_rows, kmer_counts, win_offsets, n, keep, group, num_branches, tau_q, records, segments,
                               n_segments);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("windows_paint_host: ") + e.what());
    }
}

}  // extern "C"
