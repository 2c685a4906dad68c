// cohort_place.hip -- a cohort of samples on the device: the per-branch profile of every sample, summed from the rows
// the placement kernels write, and the Kantorovich-Rubinstein distance between every two samples: epik_amd_cohort_*
// and epik_amd_placer_cohort_reads (include/epik_amd.h); cohort_host_chunked, the host side the strand, frame and mates
// variants share (host_entry.hpp).
//
// No reference counterpart: the reference writes a jplace per sample and leaves sums and distances to a second tool.
//
// The rule is stated once, in include/epik_amd.h (epik_amd/host/cohort.cpp is the same rule on the CPU).
// Every cell is a uint64 that wraps and integer adds commute -- no float atomic may appear in this file -- and the sum
// over the branches of one pair of samples is strictly sequential, so that the distances are the same bits here, on the
// host and in the tests' numpy.
//
// cohort_add_kernel: profile_kernel (profile_place.hip) with a row of cells per sample.  S * N cells do not fit LDS, and
// same-address global 64-bit atomics serialise (22 ms against 0.04 ms), so a workgroup takes a CONTIGUOUS
// range of row-slot tiles and keeps mass[N] | best[N] of ONE current sample in LDS: the sample of the first read of the
// tile at hand.  Lanes whose read is of that sample add into LDS, lanes of any other sample straight into the matrix;
// when the next tile begins in another sample the workgroup adds its non-zero LDS cells and the five totals (kept per
// lane, reduced over the wave and the workgroup) to the current sample's row and switches.  Grouped input -- what the
// drivers produce -- flushes once a sample and workgroup; interleaved input is still correct and pays a flush a tile.
// With LDS = false (trees beyond kLdsLimit, EPIK_AMD_PROFILE_LDS=0) every cell add goes to global memory; the totals of
// the current sample are still reduced first.  A read whose sample is >= S adds 1 to bad_samples and touches no row.
//
// cohort_normalise_kernel: a workgroup a sample: the uint64 inclusive prefix sum over the branches in chunks of a
// workgroup (wave scans, the waves' sums through LDS, a carry), written to a workspace; then T_s, and C_s[b], B_s[b] as
// doubles into planes [b][Sp] (Sp = S rounded up to the tile, the padding zero), sample fastest: what the distance
// kernel stages is then 256 contiguous bytes per branch and tile.
//
// cohort_kr_kernel: shaped like a GEMM with |a - b| for a * b.  A workgroup owns a tile of 32 x 32 pairs on or above
// the diagonal, lane (ty, tx) of 16 x 16 the pairs (ty | ty + 16) x (tx | tx + 16): four accumulators in registers.  A
// chunk of kChunk branches of C and B of the tile's row and column samples is staged in LDS as [branch][32 samples];
// for one branch a half-wave then reads two row addresses (ty: broadcasts) and sixteen consecutive doubles of the
// column samples (tx: banks 0..31 of ds_read_b64's 64) -- no conflict -- and walks the chunk in ascending order.
// Nothing is fused (__dsub_rn / __dadd_rn / __dmul_rn; the file is built with -ffp-contract=off as well).  The
// diagonal and the pairs with an empty sample are written by rule, the tile mirrored on the way out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kLwrBits = EPIK_AMD_PROFILE_LWR_BITS;
constexpr uint32_t kTotals = 5;                    // placed, no_hit, too_short, too_narrow, bad_rows: epik_amd_profile_totals
constexpr uint64_t kLdsBudget = 48u << 10;         // as profile_place.hip: three workgroups a CU up to 3072 branches
constexpr uint64_t kLdsLimit = (160u << 10) - 64;  // ... and one up to 10 236
constexpr uint64_t kMaxBlocks = 1024;
constexpr uint32_t kNoSample = 0xffffffffu;
constexpr uint32_t kTile = kCohortTile;  // samples a side of a tile of pairs
constexpr uint32_t kChunk = 32;   // branches staged at a time: 4 * 32 * 32 * 8 = 32 KB of LDS
constexpr uint64_t kKrBlocks = 65536;

static_assert(sizeof(epik_amd_profile_totals) == kTotals * sizeof(uint64_t));
static_assert(sizeof(epik_amd_placement) == 16);
static_assert(kBlock == 256 && kTile == 32, "a lane owns 2 x 2 pairs of a 32 x 32 tile");

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

template <bool LDS>
__global__ __launch_bounds__(kBlock) void cohort_add_kernel(const u32x4 *__restrict__ rows, const uint32_t *__restrict__ n_rows,
                                                            const uint32_t *__restrict__ kmer_counts,
                                                            const uint32_t *__restrict__ weights,
                                                            const uint32_t *__restrict__ samples, uint64_t n, uint32_t keep,
                                                            uint32_t num_branches, uint32_t num_samples,
                                                            uint64_t *__restrict__ g_cells)
{
    extern __shared__ uint64_t lds_cells[];  // LDS: mass[N] | best[N] of the current sample
    __shared__ uint64_t block_totals[kTotals + 1];  // ... its totals, and the workgroup's bad_samples
    const uint32_t cells = 2 * num_branches;
    const uint64_t stride = (uint64_t)cells + kTotals;
    if (LDS)
        for (uint32_t c = threadIdx.x; c < cells; c += kBlock) lds_cells[c] = 0;
    if (threadIdx.x <= kTotals) block_totals[threadIdx.x] = 0;
    __syncthreads();

    uint64_t tot[kTotals] = {0, 0, 0, 0, 0};  // of the current sample: placed, no_hit, too_short, too_narrow, bad_rows
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

    const uint64_t slots = n * keep, tiles = (slots + kBlock - 1) / kBlock;
    const uint64_t per = (tiles + gridDim.x - 1) / gridDim.x, t_begin = blockIdx.x * per, t_end = t_begin + per < tiles ? t_begin + per : tiles;
    for (uint64_t t = t_begin; t < t_end; ++t) {
        const uint64_t first = t * kBlock, read0 = first / keep;  // (read0 < n: first < slots)
        const uint32_t lead = __builtin_amdgcn_readfirstlane(samples[read0]);  // (one address: the branch below is uniform)
        if (lead < num_samples && lead != cur) {
            flush();
            cur = lead;
        }
        const uint32_t at = (uint32_t)(first - read0 * keep) + threadIdx.x, dr = at / keep, j = at - dr * keep;
        const uint64_t i = read0 + dr;
        if (i >= n) continue;
        const uint32_t smp = samples[i];
        if (smp >= num_samples) {
            if (j == 0) ++bad_samples;
            continue;
        }
        const u32x4 row = rows[i * keep + j];
        const uint32_t nr = n_rows[i], hits = kmer_counts[i * keep], w = weights ? weights[i] : 1u;
        const bool own = smp == cur, placed = nr != EPIK_AMD_ROWS_COUNTS_TOO_NARROW && nr != 0 && hits != 0;
        uint64_t *g_row = g_cells + smp * stride;
        if (j == 0) {
            const uint32_t k = nr == EPIK_AMD_ROWS_COUNTS_TOO_NARROW ? 3u : nr == 0 ? 2u : hits == 0 ? 1u : 0u;
            if (own) {
                tot[0] += k == 0 ? w : 0u, tot[1] += k == 1 ? w : 0u, tot[2] += k == 2 ? w : 0u, tot[3] += k == 3 ? w : 0u;
            } else if (w) {
                add64(&g_row[cells + k], w);
            }
        }
        if (!placed || j >= nr) continue;
        const uint32_t branch = row.x;
        if (branch >= num_branches) {
            if (own)
                ++tot[4];
            else
                add64(&g_row[cells + 4], 1);
            continue;
        }
        if (w == 0) continue;
        const double lwr = __hiloint2double((int)row.w, (int)row.z);
        const uint64_t q = (uint64_t)__double2ll_rn(lwr * (double)(1u << kLwrBits));
        if (LDS && own) {  // (ds_add_u64)
            add64(&lds_cells[branch], (uint64_t)w * q);
            if (j == 0) add64(&lds_cells[num_branches + branch], w);
        } else {
            add64(&g_row[branch], (uint64_t)w * q);
            if (j == 0) add64(&g_row[num_branches + branch], w);
        }
    }
    flush();
    const uint64_t bad = wave_sum(bad_samples);
    if (threadIdx.x % kWave == 0 && bad) add64(&block_totals[kTotals], bad);
    __syncthreads();
    if (threadIdx.x == 0 && block_totals[kTotals]) add64(&g_cells[num_samples * stride], block_totals[kTotals]);
}

// dst[c] += src[c]: the cells of another device's cohort, uploaded (add_cells)
__global__ __launch_bounds__(kBlock) void cohort_merge_kernel(uint64_t *__restrict__ dst, const uint64_t *__restrict__ src, uint64_t count)
{
    for (uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x; c < count; c += (uint64_t)gridDim.x * kBlock) dst[c] += src[c];
}

__global__ __launch_bounds__(kBlock) void cohort_normalise_kernel(const uint64_t *__restrict__ g_cells, const uint32_t *__restrict__ first,
                                                                  uint32_t num_samples, uint32_t num_branches, uint32_t padded,
                                                                  uint64_t *__restrict__ prefix, uint64_t *__restrict__ total,
                                                                  double *__restrict__ planes)
{
    __shared__ uint64_t wave_sums[kBlockWaves];
    const uint64_t stride = 2ull * num_branches + kTotals;
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    double *C = planes, *B = planes + (uint64_t)num_branches * padded;
    for (uint32_t s = blockIdx.x; s < num_samples; s += gridDim.x) {
        const uint64_t *mass = g_cells + s * stride;
        uint64_t *P = prefix + (uint64_t)s * num_branches;
        uint64_t carry = 0;  // (the same in every lane)
        for (uint32_t base = 0; base < num_branches; base += kBlock) {
            const uint32_t b = base + threadIdx.x;
            uint64_t v = b < num_branches ? mass[b] : 0;
#pragma unroll
            for (uint32_t d = 1; d < kWave; d <<= 1) {
                const uint64_t up = __shfl_up((unsigned long long)v, d);
                if (lane >= d) v += up;
            }
            if (lane == kWave - 1) wave_sums[wave] = v;
            __syncthreads();
            uint64_t before = carry, all = carry;
#pragma unroll
            for (uint32_t k = 0; k < kBlockWaves; ++k) {
                if (k < wave) before += wave_sums[k];
                all += wave_sums[k];
            }
            if (b < num_branches) P[b] = before + v;
            carry = all;
            __syncthreads();  // (wave_sums is written again; the last round: P is the workgroup's to read)
        }
        if (threadIdx.x == 0) total[s] = carry;
        const double T = __ull2double_rn(carry);
        for (uint32_t b = threadIdx.x; b < num_branches; b += kBlock) {
            const uint32_t f = first[b];
            const uint64_t clade = P[b] - (f ? P[f - 1] : 0), below = clade - mass[b];
            C[(uint64_t)b * padded + s] = __ddiv_rn(__ull2double_rn(clade), T);
            B[(uint64_t)b * padded + s] = __ddiv_rn(__ull2double_rn(below), T);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void cohort_kr_kernel(const double *__restrict__ planes, const double *__restrict__ half,
                                                           const uint64_t *__restrict__ total, uint32_t num_samples,
                                                           uint32_t num_branches, uint32_t padded, double *__restrict__ out)
{
    __shared__ double c_row[kChunk][kTile], b_row[kChunk][kTile], c_col[kChunk][kTile], b_col[kChunk][kTile];
    __shared__ double half_of[kChunk];
    const double *C = planes, *B = planes + (uint64_t)num_branches * padded;
    const uint32_t side = padded / kTile, tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    const uint64_t tiles = (uint64_t)side * (side + 1) / 2;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        // tile (ti, tj), ti <= tj, counted along the rows of the upper triangle
        uint32_t ti = 0;
        uint64_t rem = tile;
        while (rem >= side - ti) rem -= side - ti, ++ti;
        const uint32_t tj = ti + (uint32_t)rem;
        double acc00 = 0.0, acc01 = 0.0, acc10 = 0.0, acc11 = 0.0;
        for (uint32_t b0 = 0; b0 < num_branches; b0 += kChunk) {
            const uint32_t kc = num_branches - b0 < kChunk ? num_branches - b0 : kChunk;
            for (uint32_t e = threadIdx.x; e < kc * kTile; e += kBlock) {
                const uint32_t k = e / kTile, x = e % kTile;
                const uint64_t at = (uint64_t)(b0 + k) * padded;
                c_row[k][x] = C[at + ti * kTile + x], b_row[k][x] = B[at + ti * kTile + x];
                c_col[k][x] = C[at + tj * kTile + x], b_col[k][x] = B[at + tj * kTile + x];
            }
            if (threadIdx.x < kc) half_of[threadIdx.x] = half[b0 + threadIdx.x];
            __syncthreads();
            for (uint32_t k = 0; k < kc; ++k) {  // ascending, one branch after the other: the rule's order
                const double h = half_of[k];
                const double cr0 = c_row[k][ty], cr1 = c_row[k][ty + 16], br0 = b_row[k][ty], br1 = b_row[k][ty + 16];
                const double cc0 = c_col[k][tx], cc1 = c_col[k][tx + 16], bc0 = b_col[k][tx], bc1 = b_col[k][tx + 16];
                acc00 = __dadd_rn(acc00, __dmul_rn(h, __dadd_rn(fabs(__dsub_rn(cr0, cc0)), fabs(__dsub_rn(br0, bc0)))));
                acc01 = __dadd_rn(acc01, __dmul_rn(h, __dadd_rn(fabs(__dsub_rn(cr0, cc1)), fabs(__dsub_rn(br0, bc1)))));
                acc10 = __dadd_rn(acc10, __dmul_rn(h, __dadd_rn(fabs(__dsub_rn(cr1, cc0)), fabs(__dsub_rn(br1, bc0)))));
                acc11 = __dadd_rn(acc11, __dmul_rn(h, __dadd_rn(fabs(__dsub_rn(cr1, cc1)), fabs(__dsub_rn(br1, bc1)))));
            }
            __syncthreads();
        }
        const double acc[2][2] = {{acc00, acc01}, {acc10, acc11}};
#pragma unroll
        for (uint32_t u = 0; u < 2; ++u)
#pragma unroll
            for (uint32_t v = 0; v < 2; ++v) {
                const uint32_t r = ti * kTile + ty + 16 * u, c = tj * kTile + tx + 16 * v;
                if (r >= num_samples || c >= num_samples || r > c) continue;  // (a diagonal tile: its upper half, mirrored)
                const double d = r == c ? 0.0 : (total[r] == 0 || total[c] == 0) ? -1.0 : acc[u][v];
                out[(uint64_t)r * num_samples + c] = d;
                out[(uint64_t)c * num_samples + r] = d;
            }
    }
}

uint64_t row_stride(const epik_amd_cohort *cohort) { return 2ull * cohort->num_branches + kTotals; }
uint64_t cell_count(const epik_amd_cohort *cohort) { return cohort->num_samples * row_stride(cohort) + 1; }
uint32_t padded_samples(const epik_amd_cohort *cohort) { return cohort_padded_samples(cohort); }

// a cohort made for another device, tree or keep_at_most than the placer's would be summed wrongly, silently
int check_pair(const epik_amd_placer *p, const epik_amd_cohort *cohort)
{
    if (!p) return fail_with(EPIK_AMD_ERR_INVALID, "null placer");
    COHORT_TRY(check_cohort(cohort));
    if (cohort->device != p->device || cohort->num_branches != p->params.num_branches || cohort->keep != p->params.keep_at_most)
        return fail_with(EPIK_AMD_ERR_INVALID, "the cohort was created for another placer (device, num_branches or keep_at_most differ)");
    return EPIK_AMD_OK;
}

int add_device_impl(epik_amd_cohort *cohort, const void *d_rows, const void *d_n_rows, const void *d_kmer_counts,
                    const void *d_weights, const void *d_samples, uint64_t n, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    if (n == 0) return EPIK_AMD_OK;
    if (!d_rows || !d_n_rows || !d_kmer_counts)
        return fail_with(EPIK_AMD_ERR_INVALID, "null device buffer (the k-mer counts are required: they tell a read without hits)");
    if (!d_samples) return fail_with(EPIK_AMD_ERR_INVALID, "null device buffer (the samples are required: they name each read's row)");
    if (n > 0xffffffffull) return fail_with(EPIK_AMD_ERR_INVALID, "a batch of 2^32 reads or more");
    HIP_TRY(hipSetDevice(cohort->device));
    const uint64_t tiles = (n * cohort->keep + kBlock - 1) / kBlock;
    const dim3 grid = cohort_grid(cohort, tiles, cohort->lds ? cohort->lds_blocks : kMaxBlocks);
    const auto *rows = static_cast<const u32x4 *>(d_rows);
    const auto *n_rows = static_cast<const uint32_t *>(d_n_rows), *counts = static_cast<const uint32_t *>(d_kmer_counts);
    const auto *weights = static_cast<const uint32_t *>(d_weights), *samples = static_cast<const uint32_t *>(d_samples);
    if (cohort->lds)
        hipLaunchKernelGGL(cohort_add_kernel<true>, grid, dim3(kBlock), 2 * sizeof(uint64_t) * cohort->num_branches, stream, rows,
                           n_rows, counts, weights, samples, n, cohort->keep, cohort->num_branches, cohort->num_samples,
                           cohort->d_cells);
    else
        hipLaunchKernelGGL(cohort_add_kernel<false>, grid, dim3(kBlock), 0, stream, rows, n_rows, counts, weights, samples, n,
                           cohort->keep, cohort->num_branches, cohort->num_samples, cohort->d_cells);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

// the tree of a distance or of anything else that starts from the planes: on the cohort's device, of its N; its first[]
int check_tree(const epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t **d_first)
{
    COHORT_TRY(check_cohort(cohort));
    int tree_device = 0;
    uint32_t tree_branches = 0;
    COHORT_TRY(tree_first_device(tree, &tree_device, &tree_branches, d_first));
    if (tree_device != cohort->device || tree_branches != cohort->num_branches)
        return fail_with(EPIK_AMD_ERR_INVALID, "the tree does not fit the cohort (device or num_branches differ)");
    return EPIK_AMD_OK;
}

// the device drained, the workspace of the planes, then cohort_normalise_kernel on `stream`
int normalise_launch(epik_amd_cohort *cohort, const uint32_t *d_first, hipStream_t stream)
{
    const uint32_t N = cohort->num_branches, S = cohort->num_samples, padded = padded_samples(cohort);
    HIP_TRY(hipSetDevice(cohort->device));
    HIP_TRY(hipDeviceSynchronize());  // (the adds enqueued so far, and a distance still reading the lengths)
    if (!cohort->d_planes) {
        const size_t plane_bytes = 2ull * N * padded * sizeof(double);
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&cohort->d_prefix), (size_t)S * N * sizeof(uint64_t)));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&cohort->d_total), (size_t)S * sizeof(uint64_t)));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&cohort->d_half), (size_t)N * sizeof(double)));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&cohort->d_planes), plane_bytes));
        HIP_TRY(hipMemset(cohort->d_planes, 0, plane_bytes));  // (the padding samples of the last tile stay zero)
    }
    hipLaunchKernelGGL(cohort_normalise_kernel, cohort_grid(cohort, S, kMaxBlocks), dim3(kBlock), 0, stream, cohort->d_cells, d_first, S, N,
                       padded, cohort->d_prefix, cohort->d_total, cohort->d_planes);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

int kr_device_impl(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, void *d_out, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(check_present(branch_length, d_out));
    const uint32_t *d_first = nullptr;
    COHORT_TRY(check_tree(cohort, tree, &d_first));
    const uint32_t N = cohort->num_branches, S = cohort->num_samples, padded = padded_samples(cohort);
    std::vector<double> half;
    COHORT_TRY(half_branch_lengths(branch_length, N, half));
    COHORT_TRY(normalise_launch(cohort, d_first, stream));
    HIP_TRY(hipMemcpy(cohort->d_half, half.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice));
    const uint64_t side = padded / kTile, tiles = side * (side + 1) / 2;
    hipLaunchKernelGGL(cohort_kr_kernel, cohort_grid(cohort, tiles, kKrBlocks), dim3(kBlock), 0, stream, cohort->d_planes, cohort->d_half,
                       cohort->d_total, S, N, padded, static_cast<double *>(d_out));
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

// what the sink of a cohort placement carries from chunk to chunk
struct CohortSink {
    epik_amd_cohort *cohort;
    const uint32_t *d_weights;  // [n] of the whole batch, or null
    const uint32_t *d_samples;  // [n] of the whole batch
};

int cohort_chunk(void *ctx, const epik_amd_placement *d_rows, const uint32_t *d_n_rows, const uint32_t *d_counts, uint64_t first,
                 uint64_t count, hipStream_t stream)
{
    const auto *sink = static_cast<const CohortSink *>(ctx);
    return add_device_impl(sink->cohort, d_rows, d_n_rows, d_counts, sink->d_weights ? sink->d_weights + first : nullptr,
                           sink->d_samples + first, count, stream);
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

constexpr HostVariant kForwardHost{.chunk_reads = 1u << 18, .chunk_bytes = 64u << 20, .chunk_reads_env = "EPIK_AMD_PROFILE_CHUNK_READS",
                                   .workspace_bytes = no_workspace, .zeroed_bytes = nullptr, .place_device = place_forward};

// the used samples (T_s > 0) in ascending s: used[j], jof[s] (kCohortNoIndex for a sample without mass) and L into *count
__global__ __launch_bounds__(kBlock) void used_index_kernel(const uint64_t *__restrict__ total, uint32_t num_samples,
                                                            uint32_t *__restrict__ used, uint32_t *__restrict__ jof,
                                                            uint32_t *__restrict__ count)
{
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < num_samples; s += gridDim.x * kBlock) {
        uint32_t j = 0;
        for (uint32_t t = 0; t < s; ++t) j += total[t] != 0 ? 1u : 0u;
        const bool mine = total[s] != 0;
        jof[s] = mine ? j : kCohortNoIndex;
        if (mine) used[j] = s;  // (j < the number of used samples <= num_samples)
        if (s == num_samples - 1) *count = j + (mine ? 1u : 0u);
    }
}

void free_cohort(epik_amd_cohort *cohort)
{
    (void)hipFree(cohort->d_cells), (void)hipFree(cohort->d_prefix), (void)hipFree(cohort->d_total);
    (void)hipFree(cohort->d_planes), (void)hipFree(cohort->d_half);
    for (CohortSpace &space : cohort->space) (void)hipFree(space.d);
}

}  // namespace

namespace epik_amd {

int cohort_normalise_enqueue(epik_amd_cohort *cohort, const epik_amd_tree *tree, hipStream_t stream, const uint32_t **d_first)
{
    COHORT_TRY(check_tree(cohort, tree, d_first));
    return normalise_launch(cohort, *d_first, stream);
}

int cohort_kr_enqueue(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, void *d_out, hipStream_t stream)
{
    return kr_device_impl(cohort, tree, branch_length, d_out, stream);
}

int cohort_used_index_enqueue(const epik_amd_cohort *cohort, uint32_t *used, uint32_t *jof, uint32_t *count, hipStream_t stream)
{
    hipLaunchKernelGGL(used_index_kernel, cohort_grid_per(cohort, cohort->num_samples, kBlock, 1024), dim3(kBlock), 0, stream, cohort->d_total,
                       cohort->num_samples, used, jof, count);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

int cohort_host_chunked(epik_amd_placer *p, epik_amd_cohort *cohort, const char *seqs, const uint64_t *seq_offsets,
                        const uint32_t *weights, const uint32_t *samples, uint64_t n, uint32_t mode, uint64_t longest_placed,
                        const HostVariant &v, uint8_t *label)
{
    COHORT_TRY(check_pair(p, cohort));
    if (!samples) return fail_with(EPIK_AMD_ERR_INVALID, "null samples (a cohort placement names the sample of every read)");
    HIP_TRY(hipSetDevice(p->device));
    struct DeviceArrays {  // (freed however the call ends; place_host_chunked has drained the stream by then, or never used it)
        void *weights = nullptr, *samples = nullptr;
        hipStream_t stream = nullptr;
        ~DeviceArrays()
        {
            if (weights || samples) (void)hipStreamSynchronize(stream);
            if (weights) (void)hipFree(weights);
            if (samples) (void)hipFree(samples);
        }
    } d;
    d.stream = p->stream;
    HIP_TRY(hipMalloc(&d.samples, n * sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(d.samples, samples, n * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    if (weights) {
        HIP_TRY(hipMalloc(&d.weights, n * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(d.weights, weights, n * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    }
    CohortSink ctx{cohort, static_cast<const uint32_t *>(d.weights), static_cast<const uint32_t *>(d.samples)};
    const ChunkSink sink{cohort_chunk, &ctx};
    return place_host_chunked(p, seqs, seq_offsets, n, mode, longest_placed, v, nullptr, nullptr, nullptr, label, &sink);
}

}  // namespace epik_amd

extern "C" {

int epik_amd_cohort_create(const epik_amd_placer *p, uint32_t num_samples, epik_amd_cohort **out)
{
    if (!out) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!p) return fail_with(EPIK_AMD_ERR_INVALID, "null placer");
    COHORT_TRY(check_host_samples(num_samples));
    if (p->plan.shard_count > 1)
        return fail_with(EPIK_AMD_ERR_INVALID, "a cohort needs a whole database, not a k-mer-space shard");
    auto *cohort = new (std::nothrow) epik_amd_cohort;
    if (!cohort) return fail_with(EPIK_AMD_ERR_INVALID, "out of memory");
    cohort->device = p->device;
    cohort->num_samples = num_samples;
    cohort->num_branches = p->params.num_branches;
    cohort->keep = p->params.keep_at_most;
    cohort->max_blocks_cap = p->max_blocks_cap;
    const uint64_t lds_bytes = 2 * sizeof(uint64_t) * (uint64_t)cohort->num_branches;
    cohort->lds = lds_bytes <= kLdsLimit;
    // EPIK_AMD_PROFILE_LDS=0|1 (tests), as for a profile: the global or the LDS path whatever the tree
    if (const char *e = std::getenv("EPIK_AMD_PROFILE_LDS")) {
        if (std::strcmp(e, "0") == 0)
            cohort->lds = false;
        else if (std::strcmp(e, "1") == 0 && !cohort->lds) {
            delete cohort;
            return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "EPIK_AMD_PROFILE_LDS=1: the accumulators of this tree do not fit the LDS path");
        }
    }
    const size_t bytes = cell_count(cohort) * sizeof(uint64_t);
    hipError_t e = hipSetDevice(cohort->device);
    cohort->lds_blocks = kMaxBlocks;
    if (e == hipSuccess && cohort->lds && lds_bytes > kLdsBudget) {
        int cus = 0;
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cohort->device);
        cohort->lds_blocks = (uint32_t)std::max(1, cus);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(&cohort_add_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(kLdsLimit));
    }
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&cohort->d_cells), bytes);
    if (e == hipSuccess) e = hipMemset(cohort->d_cells, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        free_cohort(cohort);
        delete cohort;
        return fail_with(EPIK_AMD_ERR_HIP, std::string("epik_amd_cohort_create: ") + hipGetErrorString(e));
    }
    *out = cohort;
    return EPIK_AMD_OK;
}

void epik_amd_cohort_destroy(epik_amd_cohort *cohort)
{
    if (!cohort) return;
    if (hipSetDevice(cohort->device) == hipSuccess) {
        (void)hipDeviceSynchronize();
        free_cohort(cohort);
    }
    delete cohort;
}

int epik_amd_cohort_reset(epik_amd_cohort *cohort)
{
    COHORT_TRY(check_cohort(cohort));
    HIP_TRY(hipSetDevice(cohort->device));
    HIP_TRY(hipDeviceSynchronize());  // (the adds enqueued so far, on whatever stream)
    HIP_TRY(hipMemset(cohort->d_cells, 0, cell_count(cohort) * sizeof(uint64_t)));
    HIP_TRY(hipDeviceSynchronize());
    return EPIK_AMD_OK;
}

int epik_amd_cohort_info(const epik_amd_cohort *cohort, uint32_t *num_samples, uint32_t *num_branches, uint32_t *lds_path)
{
    COHORT_TRY(check_cohort(cohort));
    if (num_samples) *num_samples = cohort->num_samples;
    if (num_branches) *num_branches = cohort->num_branches;
    if (lds_path) *lds_path = cohort->lds ? 1 : 0;
    return EPIK_AMD_OK;
}

int epik_amd_cohort_read(epik_amd_cohort *cohort, uint64_t *mass, uint64_t *best, epik_amd_profile_totals *totals,
                         uint64_t *bad_samples)
{
    COHORT_TRY(check_cohort(cohort));
    HIP_TRY(hipSetDevice(cohort->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = cohort->num_branches, S = cohort->num_samples, pitch = row_stride(cohort) * sizeof(uint64_t);
    const size_t row = n * sizeof(uint64_t);
    if (mass) HIP_TRY(hipMemcpy2D(mass, row, cohort->d_cells, pitch, row, S, hipMemcpyDeviceToHost));
    if (best) HIP_TRY(hipMemcpy2D(best, row, cohort->d_cells + n, pitch, row, S, hipMemcpyDeviceToHost));
    if (totals) HIP_TRY(hipMemcpy2D(totals, sizeof *totals, cohort->d_cells + 2 * n, pitch, sizeof *totals, S, hipMemcpyDeviceToHost));
    if (bad_samples) HIP_TRY(hipMemcpy(bad_samples, cohort->d_cells + S * row_stride(cohort), sizeof *bad_samples, hipMemcpyDeviceToHost));
    return EPIK_AMD_OK;
}

int epik_amd_cohort_add_cells(epik_amd_cohort *cohort, const uint64_t *mass, const uint64_t *best,
                              const epik_amd_profile_totals *totals)
{
    return guarded("cohort_add_cells", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        const size_t n = cohort->num_branches, S = cohort->num_samples, stride = row_stride(cohort);
        std::vector<uint64_t> cells(S * stride, 0);
        for (size_t s = 0; s < S; ++s) {
            if (mass) std::memcpy(&cells[s * stride], mass + s * n, n * sizeof(uint64_t));
            if (best) std::memcpy(&cells[s * stride + n], best + s * n, n * sizeof(uint64_t));
            if (totals) std::memcpy(&cells[s * stride + 2 * n], totals + s, sizeof *totals);
        }
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult up;
        COHORT_TRY(up.alloc(cells.size() * sizeof(uint64_t)));
        HIP_TRY(hipMemcpy(up.d, cells.data(), cells.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIP_TRY(hipDeviceSynchronize());  // (the adds enqueued so far: this one is no atomic)
        const uint64_t blocks = std::min<uint64_t>((cells.size() + kBlock - 1) / kBlock, cohort->max_blocks_cap ? cohort->max_blocks_cap : kMaxBlocks);
        hipLaunchKernelGGL(cohort_merge_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, nullptr, cohort->d_cells,
                           static_cast<const uint64_t *>(up.d), (uint64_t)cells.size());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        return EPIK_AMD_OK;
    });
}

int epik_amd_cohort_add_device(epik_amd_cohort *cohort, const void *d_rows, const void *d_n_rows, const void *d_kmer_counts,
                               const void *d_weights, const void *d_samples, uint64_t n, void *stream)
{
    return add_device_impl(cohort, d_rows, d_n_rows, d_kmer_counts, d_weights, d_samples, n, static_cast<hipStream_t>(stream));
}

int epik_amd_cohort_kr_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, void *d_out,
                              void *stream)
{
    return guarded("cohort_kr_device", [&]() -> int { return kr_device_impl(cohort, tree, branch_length, d_out, static_cast<hipStream_t>(stream)); });
}

int epik_amd_cohort_kr(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, double *out)
{
    return guarded("cohort_kr", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(check_present(out));
        const size_t bytes = (size_t)cohort->num_samples * cohort->num_samples * sizeof(double);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult m;
        COHORT_TRY(m.alloc(bytes));
        COHORT_TRY(kr_device_impl(cohort, tree, branch_length, m.d, nullptr));
        return m.copy_to(out, bytes);
    });
}

int epik_amd_cohort_kr_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                            const double *branch_length, double *out)
{
    return guarded("cohort_kr_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(check_present(mass, first, branch_length, out));
        std::string err;
        return rule_result(kr_matrix(mass, num_samples, num_branches, first, branch_length, out, err), err);
    });
}

int epik_amd_placer_cohort_reads(epik_amd_placer *p, epik_amd_cohort *cohort, const char *seqs, const uint64_t *seq_offsets,
                                 const uint32_t *weights, const uint32_t *samples, uint64_t n)
{
    return guarded("cohort_reads", [&]() -> int {
        COHORT_TRY(check_pair(p, cohort));
        if (n == 0) return EPIK_AMD_OK;
        uint64_t longest = 0;
        COHORT_TRY(check_host_reads(seqs, seq_offsets, n, longest));
        return cohort_host_chunked(p, cohort, seqs, seq_offsets, weights, samples, n, 0, longest, kForwardHost, nullptr);
    });
}

}  // extern "C"
