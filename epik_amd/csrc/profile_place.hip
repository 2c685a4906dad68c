// profile_place.hip -- the abundance profile of a sample, summed on the device from the rows the placement kernels
// write: epik_amd_profile_create / _destroy / _reset / _read / _add_device and epik_amd_placer_profile_reads
// (include/epik_amd.h); profile_host_chunked, the host side the strand and frame variants share (host_entry.hpp).
//
// No reference counterpart: the reference writes a jplace and leaves the sums to a second tool.
//
// The rule (epik_amd/host/profile.cpp is the same rule on the CPU).  q(x) = llrint(x * 2^30), round half
// to even.  For read i with weight w, tested in this order:
//   n_rows[i] == EPIK_AMD_ROWS_COUNTS_TOO_NARROW   totals.too_narrow += w
//   n_rows[i] == 0                                 totals.too_short  += w
//   kmer_counts[i * keep] == 0                     totals.no_hit     += w   (rows fabricated for a read without hits)
//   otherwise                                      totals.placed     += w; best[rows[i * keep].branch] += w;
//                                                  mass[rows[i * keep + j].branch] += w * q(lwr) for j < n_rows[i]
// A row of a placed read whose branch is >= num_branches writes nothing and adds 1 to totals.bad_rows.  Every
// accumulator is a uint64 that wraps; integer adds commute, so the sums are the same bits whatever the order -- no
// float atomic may appear in this file.
//
// profile_kernel: lane l of a workgroup takes row slot 256 t + l of [n][keep] for the tiles t of its grid stride -- 16
// bytes a lane, consecutive -- and the read's n_rows, first count and weight (a few lanes share each).  With LDS = true
// the workgroup adds into mass[N] | best[N] in LDS (ds_add_u64) and at its end adds its non-zero cells to the global
// arrays; with LDS = false (16 N bytes beyond kLdsLimit, or EPIK_AMD_PROFILE_LDS=0) every add goes to global memory.
// Up to kLdsBudget (N <= 3 072) several workgroups share a CU and the grid is kMaxBlocks; beyond it, up to what one
// workgroup may have of a CU's LDS (N <= 10 236), a workgroup per CU -- the adds at the end of a workgroup are then at
// most as many as the rows it read.  Measured: a million reads on the same seven branches take the
// global path 22 ms, the LDS path 0.04 ms; that, and not the spread case, is what the LDS path is for.
// The five totals are kept per lane, reduced over the wave, then over the workgroup in LDS: five global adds a workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "host_entry.hpp"

struct epik_amd_profile {
    int device = 0;
    uint32_t num_branches = 0, keep = 0;
    bool lds = false;             // latched at create(): the LDS path
    uint32_t lds_blocks = 0;      // ... and its grid: kMaxBlocks, or a workgroup per CU for the trees beyond kLdsBudget
    uint32_t max_blocks_cap = 0;  // the placer's EPIK_AMD_MAX_BLOCKS
    uint64_t *d_cells = nullptr;  // mass[N] | best[N] | totals[kTotals]
};

namespace {

using namespace epik_amd;

constexpr uint32_t kLwrBits = EPIK_AMD_PROFILE_LWR_BITS;
constexpr uint32_t kTotals = 5;             // placed, no_hit, too_short, too_narrow, bad_rows: epik_amd_profile_totals
constexpr uint64_t kLdsBudget = 48u << 10;  // mass + best of trees of up to 3072 branches: three workgroups a CU, no limit raised
constexpr uint64_t kLdsLimit = (160u << 10) - 64;  // ... of up to 10 236: the LDS of a CU, less the workgroup's totals
constexpr uint64_t kMaxBlocks = 1024;       // four workgroups a CU: their end-of-kernel adds stay few

static_assert(sizeof(epik_amd_profile_totals) == kTotals * sizeof(uint64_t));
static_assert(sizeof(epik_amd_placement) == 16);

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
__global__ __launch_bounds__(kBlock) void profile_kernel(const u32x4 *__restrict__ rows, const uint32_t *__restrict__ n_rows,
                                                         const uint32_t *__restrict__ kmer_counts,
                                                         const uint32_t *__restrict__ weights, uint64_t n, uint32_t keep,
                                                         uint32_t num_branches, uint64_t *__restrict__ g_cells)
{
    extern __shared__ uint64_t lds_cells[];  // LDS: mass[N] | best[N]
    __shared__ uint64_t block_totals[kTotals];
    const uint32_t cells = 2 * num_branches;
    if (LDS)
        for (uint32_t c = threadIdx.x; c < cells; c += kBlock) lds_cells[c] = 0;
    if (threadIdx.x < kTotals) block_totals[threadIdx.x] = 0;
    __syncthreads();
    uint64_t *mass = LDS ? lds_cells : g_cells, *best = mass + num_branches;

    uint64_t t_placed = 0, t_no_hit = 0, t_short = 0, t_narrow = 0, t_bad = 0;
    const uint64_t slots = n * keep, tiles = (slots + kBlock - 1) / kBlock;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        // (one 64-bit division a tile, the lane's own in 32 bits)
        const uint64_t first = t * kBlock, read0 = first / keep;
        const uint32_t at = (uint32_t)(first - read0 * keep) + threadIdx.x, dr = at / keep, j = at - dr * keep;
        const uint64_t i = read0 + dr;
        if (i >= n) continue;
        const u32x4 row = rows[i * keep + j];
        const uint32_t nr = n_rows[i], hits = kmer_counts[i * keep], w = weights ? weights[i] : 1u;
        const bool placed = nr != EPIK_AMD_ROWS_COUNTS_TOO_NARROW && nr != 0 && hits != 0;
        if (j == 0) {
            if (nr == EPIK_AMD_ROWS_COUNTS_TOO_NARROW)
                t_narrow += w;
            else if (nr == 0)
                t_short += w;
            else if (hits == 0)
                t_no_hit += w;
            else
                t_placed += w;
        }
        if (!placed || j >= nr) continue;
        const uint32_t branch = row.x;
        if (branch >= num_branches) {
            ++t_bad;
            continue;
        }
        if (w == 0) continue;
        const double lwr = __hiloint2double((int)row.w, (int)row.z);
        const uint64_t q = (uint64_t)__double2ll_rn(lwr * (double)(1u << kLwrBits));
        add64(&mass[branch], (uint64_t)w * q);
        if (j == 0) add64(&best[branch], w);
    }

    const uint64_t sums[kTotals] = {wave_sum(t_placed), wave_sum(t_no_hit), wave_sum(t_short), wave_sum(t_narrow), wave_sum(t_bad)};
    if (threadIdx.x % kWave == 0)
#pragma unroll
        for (uint32_t k = 0; k < kTotals; ++k)
            if (sums[k]) add64(&block_totals[k], sums[k]);
    __syncthreads();
    if (LDS)
        for (uint32_t c = threadIdx.x; c < cells; c += kBlock)
            if (const uint64_t v = lds_cells[c]) add64(&g_cells[c], v);
    if (threadIdx.x < kTotals && block_totals[threadIdx.x]) add64(&g_cells[cells + threadIdx.x], block_totals[threadIdx.x]);
}

uint64_t cell_count(const epik_amd_profile *profile) { return 2ull * profile->num_branches + kTotals; }

// a profile made for another device, tree or keep_at_most than the placer's would be summed wrongly, silently
int check_pair(const epik_amd_placer *p, const epik_amd_profile *profile)
{
    if (!p) return fail_with(EPIK_AMD_ERR_INVALID, "null placer");
    if (!profile) return fail_with(EPIK_AMD_ERR_INVALID, "null profile");
    if (profile->device != p->device || profile->num_branches != p->params.num_branches || profile->keep != p->params.keep_at_most)
        return fail_with(EPIK_AMD_ERR_INVALID, "the profile was created for another placer (device, num_branches or keep_at_most differ)");
    return EPIK_AMD_OK;
}

int add_device_impl(epik_amd_profile *profile, const void *d_rows, const void *d_n_rows, const void *d_kmer_counts,
                    const void *d_weights, uint64_t n, hipStream_t stream)
{
    if (!profile) return fail_with(EPIK_AMD_ERR_INVALID, "null profile");
    if (n == 0) return EPIK_AMD_OK;
    if (!d_rows || !d_n_rows || !d_kmer_counts)
        return fail_with(EPIK_AMD_ERR_INVALID, "null device buffer (the k-mer counts are required: they tell a read without hits)");
    if (n > 0xffffffffull) return fail_with(EPIK_AMD_ERR_INVALID, "a batch of 2^32 reads or more");
    HIP_TRY(hipSetDevice(profile->device));
    const uint64_t tiles = (n * profile->keep + kBlock - 1) / kBlock;
    const uint64_t own_blocks = profile->lds ? profile->lds_blocks : kMaxBlocks;
    const uint64_t max_blocks = profile->max_blocks_cap ? std::min<uint64_t>(own_blocks, profile->max_blocks_cap) : own_blocks;
    const dim3 grid((uint32_t)std::max<uint64_t>(1, std::min(tiles, max_blocks)));
    const auto *rows = static_cast<const u32x4 *>(d_rows);
    const auto *n_rows = static_cast<const uint32_t *>(d_n_rows), *counts = static_cast<const uint32_t *>(d_kmer_counts);
    const auto *weights = static_cast<const uint32_t *>(d_weights);
    if (profile->lds)
        hipLaunchKernelGGL(profile_kernel<true>, grid, dim3(kBlock), 2 * sizeof(uint64_t) * profile->num_branches, stream, rows,
                           n_rows, counts, weights, n, profile->keep, profile->num_branches, profile->d_cells);
    else
        hipLaunchKernelGGL(profile_kernel<false>, grid, dim3(kBlock), 0, stream, rows, n_rows, counts, weights, n, profile->keep,
                           profile->num_branches, profile->d_cells);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

// what the sink of a profile-only placement carries from chunk to chunk
struct ProfileSink {
    epik_amd_profile *profile;
    const uint32_t *d_weights;  // [n] of the whole batch, or null
};

int profile_chunk(void *ctx, const epik_amd_placement *d_rows, const uint32_t *d_n_rows, const uint32_t *d_counts,
                  uint64_t first, uint64_t count, hipStream_t stream)
{
    const auto *sink = static_cast<const ProfileSink *>(ctx);
    return add_device_impl(sink->profile, d_rows, d_n_rows, d_counts, sink->d_weights ? sink->d_weights + first : nullptr, count, stream);
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

}  // namespace

namespace epik_amd {

int check_profile_pair(const epik_amd_placer *p, const epik_amd_profile *profile) { return check_pair(p, profile); }

int profile_host_chunked(epik_amd_placer *p, epik_amd_profile *profile, const char *seqs, const uint64_t *seq_offsets,
                         const uint32_t *weights, uint64_t n, uint32_t mode, uint64_t longest_placed, const HostVariant &v,
                         uint8_t *label)
{
    if (const int rc = check_pair(p, profile); rc != EPIK_AMD_OK) return rc;
    HIP_TRY(hipSetDevice(p->device));
    struct Weights {  // (freed however the call ends; place_host_chunked has drained the stream by then, or never used it)
        void *d = nullptr;
        hipStream_t stream = nullptr;
        ~Weights()
        {
            if (d) (void)hipStreamSynchronize(stream), (void)hipFree(d);
        }
    } w;
    w.stream = p->stream;
    if (weights) {
        HIP_TRY(hipMalloc(&w.d, n * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(w.d, weights, n * sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    }
    ProfileSink ctx{profile, static_cast<const uint32_t *>(w.d)};
    const ChunkSink sink{profile_chunk, &ctx};
    return place_host_chunked(p, seqs, seq_offsets, n, mode, longest_placed, v, nullptr, nullptr, nullptr, label, &sink);
}

}  // namespace epik_amd

extern "C" {

int epik_amd_profile_create(const epik_amd_placer *p, epik_amd_profile **out)
{
    if (!out) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!p) return fail_with(EPIK_AMD_ERR_INVALID, "null placer");
    auto *profile = new (std::nothrow) epik_amd_profile;
    if (!profile) return fail_with(EPIK_AMD_ERR_INVALID, "out of memory");
    profile->device = p->device;
    profile->num_branches = p->params.num_branches;
    profile->keep = p->params.keep_at_most;
    profile->max_blocks_cap = p->max_blocks_cap;
    const uint64_t lds_bytes = 2 * sizeof(uint64_t) * (uint64_t)profile->num_branches;
    profile->lds = lds_bytes <= kLdsLimit;
    // EPIK_AMD_PROFILE_LDS=0|1 (tests): the global or the LDS path whatever the tree (1: only where LDS holds the cells)
    if (const char *e = std::getenv("EPIK_AMD_PROFILE_LDS")) {
        if (std::strcmp(e, "0") == 0)
            profile->lds = false;
        else if (std::strcmp(e, "1") == 0 && !profile->lds) {
            delete profile;
            return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "EPIK_AMD_PROFILE_LDS=1: the accumulators of this tree do not fit the LDS path");
        }
    }
    const size_t bytes = cell_count(profile) * sizeof(uint64_t);
    hipError_t e = hipSetDevice(profile->device);
    profile->lds_blocks = kMaxBlocks;
    if (e == hipSuccess && profile->lds && lds_bytes > kLdsBudget) {
        int cus = 0;
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, profile->device);
        profile->lds_blocks = (uint32_t)std::max(1, cus);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(&profile_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(kLdsLimit));
    }
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&profile->d_cells), bytes);
    if (e == hipSuccess) e = hipMemset(profile->d_cells, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        if (profile->d_cells) (void)hipFree(profile->d_cells);
        delete profile;
        return fail_with(EPIK_AMD_ERR_HIP, std::string("epik_amd_profile_create: ") + hipGetErrorString(e));
    }
    *out = profile;
    return EPIK_AMD_OK;
}

void epik_amd_profile_destroy(epik_amd_profile *profile)
{
    if (!profile) return;
    if (hipSetDevice(profile->device) == hipSuccess) {
        (void)hipDeviceSynchronize();
        (void)hipFree(profile->d_cells);
    }
    delete profile;
}

int epik_amd_profile_reset(epik_amd_profile *profile)
{
    if (!profile) return fail_with(EPIK_AMD_ERR_INVALID, "null profile");
    HIP_TRY(hipSetDevice(profile->device));
    HIP_TRY(hipDeviceSynchronize());  // (the adds enqueued so far, on whatever stream)
    HIP_TRY(hipMemset(profile->d_cells, 0, cell_count(profile) * sizeof(uint64_t)));
    HIP_TRY(hipDeviceSynchronize());
    return EPIK_AMD_OK;
}

int epik_amd_profile_read(epik_amd_profile *profile, uint64_t *mass, uint64_t *best, epik_amd_profile_totals *totals)
{
    if (!profile) return fail_with(EPIK_AMD_ERR_INVALID, "null profile");
    HIP_TRY(hipSetDevice(profile->device));
    HIP_TRY(hipDeviceSynchronize());
    const size_t n = profile->num_branches;
    if (mass) HIP_TRY(hipMemcpy(mass, profile->d_cells, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (best) HIP_TRY(hipMemcpy(best, profile->d_cells + n, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (totals) HIP_TRY(hipMemcpy(totals, profile->d_cells + 2 * n, sizeof *totals, hipMemcpyDeviceToHost));
    return EPIK_AMD_OK;
}

int epik_amd_profile_info(const epik_amd_profile *profile, uint32_t *num_branches, uint32_t *lds_path)
{
    if (!profile) return fail_with(EPIK_AMD_ERR_INVALID, "null profile");
    if (num_branches) *num_branches = profile->num_branches;
    if (lds_path) *lds_path = profile->lds ? 1 : 0;
    return EPIK_AMD_OK;
}

int epik_amd_profile_add_device(epik_amd_profile *profile, const void *d_rows, const void *d_n_rows, const void *d_kmer_counts,
                                const void *d_weights, uint64_t n, void *stream)
{
    return add_device_impl(profile, d_rows, d_n_rows, d_kmer_counts, d_weights, n, static_cast<hipStream_t>(stream));
}

int epik_amd_placer_profile_reads(epik_amd_placer *p, epik_amd_profile *profile, const char *seqs, const uint64_t *seq_offsets,
                                  const uint32_t *weights, uint64_t n)
{
    try {  // std::vector: nothing may leave through the C ABI
        if (const int rc = check_pair(p, profile); rc != EPIK_AMD_OK) return rc;
        if (p->plan.shard_count > 1)
            return fail_with(EPIK_AMD_ERR_UNSUPPORTED, "a profile needs a whole database, not a k-mer-space shard");
        if (n == 0) return EPIK_AMD_OK;
        uint64_t longest = 0;
        if (const int rc = check_host_reads(seqs, seq_offsets, n, longest); rc != EPIK_AMD_OK) return rc;
        return profile_host_chunked(p, profile, seqs, seq_offsets, weights, n, 0, longest, kForwardHost, nullptr);
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("profile_reads: ") + e.what());
    }
}

}  // extern "C"
