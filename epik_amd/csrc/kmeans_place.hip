// kmeans_place.hip -- phylogenetic k-means (Czech et al. 2019) of a cohort's samples on the device:
// epik_amd_cohort_kmeans_device / _kmeans / _kmeans_host (include/epik_amd.h).
//
// No reference counterpart.  The rule is stated once, in include/epik_amd.h beside the KR, squash and epca rules
// (epik_amd/host/cohort.cpp: kmeans_clusters is the same rule on the CPU).  A centroid is a mass
// distribution of its own -- the average of the planes of its members -- and every distance to it is the KR rule's strictly
// sequential sum over the branches, so every output is the same bits here, on the host and in the tests' numpy.  Nothing
// is fused (__dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn; the file is built with -ffp-contract=off as well).
//
// Start-up: cohort_normalise_kernel (cohort_place.hip) leaves T_s and the planes C, B [b][Sp].  Then
//
//   kmeans_init_kernel     one workgroup: the used samples compacted in ascending s (used[j] = s, L, K' = min(K, L)),
//                          assign = "none", no centre yet.
//   kmeans_average_kernel  work shared over (b, k), k fastest: a lane walks the members of cluster k in ascending j and
//                          divides once.  With the list of all used samples as the one cluster it is the grand mean (into
//                          the column buffer), in the iterations it is the update (into the centroid planes [b][64]).
//   kmeans_column_kernel   a lane a used sample j: KR(column, j) with b ascending, the column (the grand mean, then the
//                          centre just picked) and half staged in LDS 32 branches at a time and read back as broadcasts,
//                          the 32 branches of the lane's own sample loaded ahead of the dependent add chain.
//   kmeans_pick_kernel     every workgroup reduces the L values by (value, j) -- the first smallest KR(M, j) for centre 0,
//                          the first largest mind[j] among the samples not yet centres after it --, then the copy of the
//                          centre's planes into centroid k and into the column buffer is shared out over the branches.
//
// Pass p of the seeding is column(p), pick(p); all K of them are enqueued up front and return uniformly when p >= K', so
// the host does not need L.  Then an iteration is
//
//   kmeans_dist_kernel     cohort_kr_kernel's tile made rectangular: 16 used samples x 16 centroids a workgroup, a pair a
//                          lane, the branches staged in LDS in ascending chunks of 32.  (DESIGN.md 3.11 for the tile.)
//   kmeans_argmin_kernel   a lane a used sample, k ascending, strict <; `changed` counted with an atomic add of each
//                          lane's own flag on one uint32.
//   kmeans_members_kernel  a workgroup a cluster: the stable compaction of its members in ascending j.
//
// and the host reads `changed` (4 bytes, one stream synchronisation), then either stops or enqueues the update.
//   kmeans_finish_kernel   writes every record: samples, clusters (a lane a cluster walking its members in order),
//                          centroids and info.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kNone = EPIK_AMD_KMEANS_NONE;
constexpr uint32_t kMaxK = EPIK_AMD_KMEANS_MAX_CLUSTERS;  // the pitch of the centroid planes and of D
constexpr uint32_t kUnit = 32;         // branches staged at a time
constexpr uint32_t kTileS = 16, kTileK = 16;  // used samples x centroids of a workgroup of the distance kernel
constexpr uint64_t kManyBlocks = 1024;

static_assert(sizeof(epik_amd_kmeans_info) == 16 && sizeof(epik_amd_kmeans_sample) == 16 && sizeof(epik_amd_kmeans_cluster) == 24);
static_assert(kTileS * kTileK == kBlock && kUnit <= kWave);

struct KmeansControl {
    uint32_t used, clusters;  // L, K'
    uint32_t changed, pad;
    uint32_t centre[kMaxK];   // the j of centre k
    uint32_t seed[kMaxK];     // ... and its s
    uint32_t size[kMaxK];
};

// the workspace, one allocation: what the kernels take
struct KmeansSpace {
    double *cent;      // C[N][64] | B[N][64]: the centroid planes, centroid fastest
    double *column;    // C[N] | B[N]: the grand mean, then the centre just picked
    double *D;         // [S][64]
    double *mind;      // [S]: KR(M, j) in pass 0, then the distance to the nearest centre
    double *dist;      // [S]: D[j][assign[j]]
    KmeansControl *ctl;
    uint32_t *used;    // [S]: the s of j
    uint32_t *all;     // [S]: 0 .. S - 1, the member list of the grand mean
    uint32_t *assign;  // [S]
    uint32_t *is_centre;  // [S]
    uint32_t *members; // [64][S]: the j of cluster k's members, ascending
};

size_t kmeans_space(void *base, uint32_t S, uint32_t N, KmeansSpace *sp)
{
    Carver c(base);
    const KmeansSpace parts{.cent = c.take<double>(2 * (size_t)N * kMaxK),
                            .column = c.take<double>(2 * (size_t)N),
                            .D = c.take<double>((size_t)S * kMaxK),
                            .mind = c.take<double>(S),
                            .dist = c.take<double>(S),
                            .ctl = c.take<KmeansControl>(1),
                            .used = c.take<uint32_t>(S),
                            .all = c.take<uint32_t>(S),
                            .assign = c.take<uint32_t>(S),
                            .is_centre = c.take<uint32_t>(S),
                            .members = c.take<uint32_t>((size_t)kMaxK * S)};
    if (sp) *sp = parts;
    return c.bytes();
}

// the i < count with pred(i), in ascending order, into out[]; their number.  One workgroup of kBlock, every lane calls.
template <class Pred>
__device__ inline uint32_t block_compact(uint32_t count, Pred pred, uint32_t *__restrict__ out, uint32_t *wave_sums)
{
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    uint32_t carry = 0;  // (the same in every lane)
    for (uint32_t base = 0; base < count; base += kBlock) {
        const uint32_t i = base + threadIdx.x;
        const bool flag = i < count && pred(i);
        const unsigned long long mask = __ballot(flag);
        if (lane == 0) wave_sums[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = carry, all = carry;
#pragma unroll
        for (uint32_t k = 0; k < kBlockWaves; ++k) {
            if (k < wave) before += wave_sums[k];
            all += wave_sums[k];
        }
        if (flag) out[before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = i;
        carry = all;
        __syncthreads();  // (wave_sums is written again)
    }
    return carry;
}

__global__ __launch_bounds__(kBlock) void kmeans_init_kernel(const uint64_t *__restrict__ total, uint32_t num_samples,
                                                             uint32_t num_clusters, KmeansControl *__restrict__ ctl,
                                                             uint32_t *__restrict__ used, uint32_t *__restrict__ all,
                                                             uint32_t *__restrict__ assign, uint32_t *__restrict__ is_centre)
{
    __shared__ uint32_t wave_sums[kBlockWaves];
    if (blockIdx.x != 0) return;
    for (uint32_t s = threadIdx.x; s < num_samples; s += kBlock) all[s] = s, assign[s] = kNone, is_centre[s] = 0u;
    for (uint32_t k = threadIdx.x; k < kMaxK; k += kBlock) ctl->centre[k] = kNone, ctl->seed[k] = kNone, ctl->size[k] = 0u;
    const uint32_t L = block_compact(num_samples, [&](uint32_t s) { return total[s] != 0; }, used, wave_sums);
    if (threadIdx.x == 0) ctl->used = L, ctl->clusters = L < num_clusters ? L : num_clusters, ctl->changed = 0u, ctl->pad = 0u;
}

// for every b and every cluster k < clusters with members: out[b * pitch + k] = (the sum of the planes of its members, in
// the list's order, from +0.0) / size.  clusters, size[] and the list are the device's: `whole` takes the one list of all
// used samples (the grand mean), else cluster k's list is members + k * num_samples and the count ctl->clusters.
__global__ __launch_bounds__(kBlock) void kmeans_average_kernel(const double *__restrict__ planes, uint32_t num_branches,
                                                                uint32_t padded, uint32_t num_samples,
                                                                const KmeansControl *__restrict__ ctl,
                                                                const uint32_t *__restrict__ used,
                                                                const uint32_t *__restrict__ members, bool whole,
                                                                double *__restrict__ out_c, double *__restrict__ out_b,
                                                                uint32_t pitch)
{
    const uint32_t clusters = whole ? 1u : ctl->clusters;
    if (clusters == 0) return;
    const double *C = planes, *B = planes + (uint64_t)num_branches * padded;
    const uint64_t cells = (uint64_t)num_branches * clusters;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock) {
        const uint32_t k = (uint32_t)(e % clusters), b = (uint32_t)(e / clusters);
        const uint32_t size = whole ? ctl->used : ctl->size[k];
        if (size == 0) continue;  // (a cluster without members keeps the planes it has)
        const uint32_t *list = members + (uint64_t)k * num_samples;
        const uint64_t at = (uint64_t)b * padded;
        double acc_c = 0.0, acc_b = 0.0;
        for (uint32_t i = 0; i < size; ++i) {  // ascending j, one member after the other: the rule's order
            const uint32_t s = used[list[i]];
            acc_c = __dadd_rn(acc_c, C[at + s]);
            acc_b = __dadd_rn(acc_b, B[at + s]);
        }
        out_c[(uint64_t)b * pitch + k] = __ddiv_rn(acc_c, (double)size);
        out_b[(uint64_t)b * pitch + k] = __ddiv_rn(acc_b, (double)size);
    }
}

__device__ inline double kr_step(double acc, double h, double cm, double bm, double cx, double bx)
{
    return __dadd_rn(acc, __dmul_rn(h, __dadd_rn(fabs(__dsub_rn(cm, cx)), fabs(__dsub_rn(bm, bx)))));
}

// pass 0: mind[j] = KR(grand mean, j).  Pass p >= 1, run only when another centre follows (p < K'): the distance to
// centre p - 1, mind[j] = that for p = 1 and min(mind[j], that) after; the lane of the centre marks it.
__global__ __launch_bounds__(kWave) void kmeans_column_kernel(const double *__restrict__ planes, uint32_t num_branches,
                                                              uint32_t padded, const double *__restrict__ half,
                                                              const double *__restrict__ column,
                                                              const KmeansControl *__restrict__ ctl,
                                                              const uint32_t *__restrict__ used, uint32_t pass,
                                                              double *__restrict__ mind, uint32_t *__restrict__ is_centre)
{
    __shared__ double s_cm[kUnit], s_bm[kUnit], s_half[kUnit];
    const uint32_t L = ctl->used;
    if (L == 0 || pass >= ctl->clusters) return;  // (uniform)
    const uint32_t lane = threadIdx.x;
    const double *Cm = column, *Bm = column + num_branches;
    const uint32_t full = num_branches / kUnit * kUnit;
    // a workgroup is one wave of 64 used samples; every lane walks the branches (the barriers), a lane without a sample
    // walks the last one's column and writes nothing
    for (uint32_t j0 = blockIdx.x * kWave; j0 < L; j0 += gridDim.x * kWave) {
        const uint32_t j = j0 + lane < L ? j0 + lane : L - 1;
        const double *Cx = planes + used[j], *Bx = planes + (uint64_t)num_branches * padded + used[j];
        double acc = 0.0;
        for (uint32_t b0 = 0; b0 < full; b0 += kUnit) {
            __syncthreads();  // (the reads of the unit before are done)
            if (lane < kUnit) s_cm[lane] = Cm[b0 + lane], s_bm[lane] = Bm[b0 + lane], s_half[lane] = half[b0 + lane];
            double c[kUnit], b[kUnit];
            const double *pc = Cx + (uint64_t)b0 * padded, *pb = Bx + (uint64_t)b0 * padded;
#pragma unroll
            for (uint32_t k = 0; k < kUnit; ++k, pc += padded, pb += padded) c[k] = *pc, b[k] = *pb;  // all in flight at once
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < kUnit; ++k)  // ascending, one branch after the other: the rule's order
                acc = kr_step(acc, s_half[k], s_cm[k], s_bm[k], c[k], b[k]);
        }
        for (uint32_t b = full; b < num_branches; ++b)  // the last N % kUnit branches: uniform loads
            acc = kr_step(acc, half[b], Cm[b], Bm[b], Cx[(uint64_t)b * padded], Bx[(uint64_t)b * padded]);
        if (j0 + lane >= L) continue;
        if (pass <= 1) {
            mind[j] = acc;
        } else {
            const double m = mind[j];
            mind[j] = acc < m ? acc : m;
        }
        if (pass >= 1 && j == ctl->centre[pass - 1]) is_centre[j] = 1u;
    }
}

// whether (v, j) comes before (best_v, best_j): the smaller value (the larger with `largest`), then the smaller index;
// kNone is no candidate
__device__ inline bool comes_first(bool largest, double v, uint32_t j, double best_v, uint32_t best_j)
{
    if (j == kNone) return false;
    if (best_j == kNone) return true;
    return (largest ? v > best_v : v < best_v) || (v == best_v && j < best_j);
}

__global__ __launch_bounds__(kBlock) void kmeans_pick_kernel(const double *__restrict__ planes, uint32_t num_branches, uint32_t padded,
                                                             KmeansControl *__restrict__ ctl, const uint32_t *__restrict__ used,
                                                             uint32_t pass, const double *__restrict__ mind,
                                                             const uint32_t *__restrict__ is_centre, double *__restrict__ cent,
                                                             double *__restrict__ column)
{
    __shared__ double wave_val[kBlockWaves];
    __shared__ uint32_t wave_at[kBlockWaves];
    const uint32_t L = ctl->used;
    if (pass >= ctl->clusters) return;  // (uniform)
    const bool largest = pass != 0;
    double val = 0.0;
    uint32_t at = kNone;
    for (uint32_t j = threadIdx.x; j < L; j += kBlock) {  // (ascending in a lane: a strict comparison keeps the first)
        if (largest && is_centre[j]) continue;
        const double v = mind[j];
        if (at == kNone || (largest ? v > val : v < val)) val = v, at = j;
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const double ov = __shfl_down(val, d);
        const uint32_t oj = __shfl_down(at, d);
        if (comes_first(largest, ov, oj, val, at)) val = ov, at = oj;
    }
    if (threadIdx.x % kWave == 0) wave_val[threadIdx.x / kWave] = val, wave_at[threadIdx.x / kWave] = at;
    __syncthreads();
    val = wave_val[0], at = wave_at[0];
#pragma unroll
    for (uint32_t k = 1; k < kBlockWaves; ++k)
        if (comes_first(largest, wave_val[k], wave_at[k], val, at)) val = wave_val[k], at = wave_at[k];
    // (the same in every lane of every workgroup from here; pass < K' <= L: there is a sample that is no centre yet)
    if (at == kNone) return;
    const uint32_t s = used[at];
    const double *C = planes, *B = planes + (uint64_t)num_branches * padded;
    double *cent_c = cent, *cent_b = cent + (uint64_t)num_branches * kMaxK;
    for (uint32_t b = blockIdx.x * kBlock + threadIdx.x; b < num_branches; b += gridDim.x * kBlock) {
        const double c = C[(uint64_t)b * padded + s], bb = B[(uint64_t)b * padded + s];
        cent_c[(uint64_t)b * kMaxK + pass] = c, cent_b[(uint64_t)b * kMaxK + pass] = bb;
        column[b] = c, column[num_branches + b] = bb;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->centre[pass] = at, ctl->seed[pass] = s;
}

// D[j][k] = KR(j, centroid k): a workgroup a tile of 16 used samples x 16 centroids, a pair a lane
__global__ __launch_bounds__(kBlock) void kmeans_dist_kernel(const double *__restrict__ planes, const double *__restrict__ half,
                                                             uint32_t num_branches, uint32_t padded,
                                                             const double *__restrict__ cent, KmeansControl *__restrict__ ctl,
                                                             const uint32_t *__restrict__ used, double *__restrict__ D)
{
    __shared__ double c_row[kUnit][kTileS], b_row[kUnit][kTileS], c_col[kUnit][kTileK], b_col[kUnit][kTileK];
    __shared__ double half_of[kUnit];
    const uint32_t L = ctl->used, Kc = ctl->clusters;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->changed = 0u;  // (the host has read the count of the iteration before)
    if (L == 0) return;
    const double *C = planes, *B = planes + (uint64_t)num_branches * padded;
    const double *cent_c = cent, *cent_b = cent + (uint64_t)num_branches * kMaxK;
    const uint32_t tiles_k = (Kc + kTileK - 1) / kTileK;
    const uint64_t tiles = (uint64_t)((L + kTileS - 1) / kTileS) * tiles_k;
    const uint32_t tx = threadIdx.x % kTileK, ty = threadIdx.x / kTileK;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t j0 = (uint32_t)(tile / tiles_k) * kTileS, k0 = (uint32_t)(tile % tiles_k) * kTileK;
        // what this lane stages of every chunk: sample j0 + tx (the last used one beyond L) and centroid k0 + tx (the
        // planes are 64 wide, so a centroid beyond K' is read, zeros or stale values, and never written out)
        const uint32_t my_s = used[j0 + tx < L ? j0 + tx : L - 1];
        double acc = 0.0;
        for (uint32_t b0 = 0; b0 < num_branches; b0 += kUnit) {
            const uint32_t kc = num_branches - b0 < kUnit ? num_branches - b0 : kUnit;
            for (uint32_t k = ty; k < kc; k += kBlock / kTileK) {
                const uint64_t b = b0 + k;
                c_row[k][tx] = C[b * padded + my_s], b_row[k][tx] = B[b * padded + my_s];
                c_col[k][tx] = cent_c[b * kMaxK + k0 + tx], b_col[k][tx] = cent_b[b * kMaxK + k0 + tx];
            }
            if (threadIdx.x < kc) half_of[threadIdx.x] = half[b0 + threadIdx.x];
            __syncthreads();
            for (uint32_t k = 0; k < kc; ++k)  // ascending, one branch after the other: the rule's order
                acc = kr_step(acc, half_of[k], c_row[k][ty], b_row[k][ty], c_col[k][tx], b_col[k][tx]);
            __syncthreads();
        }
        const uint32_t j = j0 + ty, k = k0 + tx;
        if (j < L && k < Kc) D[(uint64_t)j * kMaxK + k] = acc;
    }
}

__global__ __launch_bounds__(kBlock) void kmeans_argmin_kernel(const double *__restrict__ D, KmeansControl *__restrict__ ctl,
                                                               uint32_t *__restrict__ assign, double *__restrict__ dist)
{
    const uint32_t L = ctl->used, Kc = ctl->clusters;
    for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < L; j += gridDim.x * kBlock) {
        const double *row = D + (uint64_t)j * kMaxK;
        double best = row[0];
        uint32_t at = 0;
        for (uint32_t k = 1; k < Kc; ++k)  // ascending, strict <: the first smallest
            if (row[k] < best) best = row[k], at = k;
        if (assign[j] != at) atomicAdd(&ctl->changed, 1u);
        assign[j] = at, dist[j] = best;
    }
}

__global__ __launch_bounds__(kBlock) void kmeans_members_kernel(KmeansControl *__restrict__ ctl, const uint32_t *__restrict__ assign,
                                                                uint32_t num_samples, uint32_t *__restrict__ members)
{
    __shared__ uint32_t wave_sums[kBlockWaves];
    const uint32_t L = ctl->used, Kc = ctl->clusters;
    for (uint32_t k = blockIdx.x; k < Kc; k += gridDim.x) {
        const uint32_t size = block_compact(L, [&](uint32_t j) { return assign[j] == k; }, members + (uint64_t)k * num_samples, wave_sums);
        if (threadIdx.x == 0) ctl->size[k] = size;
    }
}

__global__ __launch_bounds__(kBlock) void kmeans_finish_kernel(const KmeansControl *__restrict__ ctl, const uint64_t *__restrict__ total,
                                                               const uint32_t *__restrict__ used, const uint32_t *__restrict__ assign,
                                                               const double *__restrict__ dist, const uint32_t *__restrict__ members,
                                                               const double *__restrict__ cent, uint32_t num_samples,
                                                               uint32_t num_branches, uint32_t num_clusters, uint32_t iterations,
                                                               uint32_t converged, epik_amd_kmeans_sample *__restrict__ samples,
                                                               epik_amd_kmeans_cluster *__restrict__ clusters,
                                                               double *__restrict__ centroids, epik_amd_kmeans_info *__restrict__ info)
{
    const uint32_t L = ctl->used, Kc = ctl->clusters;
    const uint32_t tid = blockIdx.x * kBlock + threadIdx.x, threads = gridDim.x * kBlock;
    for (uint32_t s = tid; s < num_samples; s += threads)
        if (total[s] == 0) samples[s] = epik_amd_kmeans_sample{kNone, 0u, -1.0};
    for (uint32_t j = tid; j < L; j += threads) samples[used[j]] = epik_amd_kmeans_sample{assign[j], 0u, dist[j]};
    for (uint32_t k = tid; k < num_clusters; k += threads) {
        if (k >= Kc) {
            clusters[k] = epik_amd_kmeans_cluster{0u, kNone, 0.0, 0.0};
            continue;
        }
        const uint32_t size = ctl->size[k], *list = members + (uint64_t)k * num_samples;
        double sum = 0.0, sq = 0.0;
        for (uint32_t i = 0; i < size; ++i) {  // ascending j
            const double d = dist[list[i]];
            sum = __dadd_rn(sum, d), sq = __dadd_rn(sq, __dmul_rn(d, d));
        }
        clusters[k] = epik_amd_kmeans_cluster{size, ctl->seed[k], sum, sq};
    }
    const double *cent_c = cent, *cent_b = cent + (uint64_t)num_branches * kMaxK;
    const uint64_t cells = (uint64_t)num_clusters * num_branches;
    for (uint64_t e = tid; e < cells; e += threads) {
        const uint32_t k = (uint32_t)(e / num_branches), b = (uint32_t)(e % num_branches);
        centroids[e] = k < Kc ? __dsub_rn(cent_c[(uint64_t)b * kMaxK + k], cent_b[(uint64_t)b * kMaxK + k]) : 0.0;
    }
    if (tid == 0) *info = L ? epik_amd_kmeans_info{L, Kc, iterations, converged} : epik_amd_kmeans_info{0u, 0u, 0u, 1u};
}

int check_counts(uint32_t K, uint32_t max_iterations)
{
    if (K < 1 || K > EPIK_AMD_KMEANS_MAX_CLUSTERS)
        return fail_with(EPIK_AMD_ERR_INVALID, "num_clusters = " + std::to_string(K) + " is outside [1, 64]");
    if (max_iterations < 1 || max_iterations > EPIK_AMD_KMEANS_MAX_ITERATIONS)
        return fail_with(EPIK_AMD_ERR_INVALID, "max_iterations = " + std::to_string(max_iterations) + " is outside [1, 1000]");
    return EPIK_AMD_OK;
}

int kmeans_device_impl(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t K,
                       uint32_t max_iterations, void *d_samples, void *d_clusters, void *d_centroids, void *d_info,
                       hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(check_present(branch_length, d_samples, d_clusters, d_centroids, d_info));
    COHORT_TRY(check_counts(K, max_iterations));
    const uint32_t N = cohort->num_branches, S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    std::vector<double> half;
    COHORT_TRY(half_branch_lengths(branch_length, N, half));
    // the checks of the tree, the device drained, then T_s and the planes
    const uint32_t *d_first = nullptr;
    COHORT_TRY(cohort_normalise_enqueue(cohort, tree, stream, &d_first));
    HIP_TRY(hipMemcpy(cohort->d_half, half.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice));
    const size_t bytes = kmeans_space(nullptr, S, N, nullptr);
    bool fresh = false;
    COHORT_TRY(cohort_space_ensure(cohort, kSpaceKmeans, bytes, &fresh));
    KmeansSpace sp;
    kmeans_space(cohort->space[kSpaceKmeans].d, S, N, &sp);
    if (fresh) HIP_TRY(hipMemset(cohort->space[kSpaceKmeans].d, 0, bytes));  // (the centroid planes beyond K' are read by the distance tiles)
    double *cent_c = sp.cent, *cent_b = sp.cent + (uint64_t)N * kMaxK;
    hipLaunchKernelGGL(kmeans_init_kernel, dim3(1), dim3(kBlock), 0, stream, cohort->d_total, S, K, sp.ctl, sp.used, sp.all, sp.assign,
                       sp.is_centre);
    hipLaunchKernelGGL(kmeans_average_kernel, cohort_grid_per(cohort, N, kBlock, kManyBlocks), dim3(kBlock), 0, stream, cohort->d_planes, N, padded, S, sp.ctl, sp.used,
                       sp.all, true, sp.column, sp.column + N, 1u);
    HIP_TRY(hipGetLastError());
    const dim3 column_grid = cohort_grid_per(cohort, S, kWave, kManyBlocks), pick_grid = cohort_grid_per(cohort, N, kBlock, kManyBlocks);
    for (uint32_t pass = 0; pass < K; ++pass) {
        hipLaunchKernelGGL(kmeans_column_kernel, column_grid, dim3(kWave), 0, stream, cohort->d_planes, N, padded, cohort->d_half,
                           sp.column, sp.ctl, sp.used, pass, sp.mind, sp.is_centre);
        hipLaunchKernelGGL(kmeans_pick_kernel, pick_grid, dim3(kBlock), 0, stream, cohort->d_planes, N, padded, sp.ctl, sp.used, pass,
                           sp.mind, sp.is_centre, sp.cent, sp.column);
        HIP_TRY(hipGetLastError());
    }
    const uint64_t tiles = (uint64_t)((S + kTileS - 1) / kTileS) * ((K + kTileK - 1) / kTileK);
    const dim3 dist_grid = cohort_grid(cohort, tiles, kManyBlocks), sample_grid = cohort_grid_per(cohort, S, kBlock, kManyBlocks);
    const dim3 member_grid = cohort_grid(cohort, K, kManyBlocks);
    const dim3 update_grid = cohort_grid_per(cohort, (uint64_t)N * K, kBlock, kManyBlocks);
    uint32_t iterations = 0, converged = 0;
    for (;;) {
        ++iterations;
        hipLaunchKernelGGL(kmeans_dist_kernel, dist_grid, dim3(kBlock), 0, stream, cohort->d_planes, cohort->d_half, N, padded, sp.cent,
                           sp.ctl, sp.used, sp.D);
        hipLaunchKernelGGL(kmeans_argmin_kernel, sample_grid, dim3(kBlock), 0, stream, sp.D, sp.ctl, sp.assign, sp.dist);
        hipLaunchKernelGGL(kmeans_members_kernel, member_grid, dim3(kBlock), 0, stream, sp.ctl, sp.assign, S, sp.members);
        HIP_TRY(hipGetLastError());
        uint32_t changed = 0;  // the one readback of an iteration
        HIP_TRY(hipMemcpyAsync(&changed, &sp.ctl->changed, sizeof changed, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (changed > S) return fail_with(EPIK_AMD_ERR_HIP, "cohort_kmeans: the device counted more changes than there are samples");
        if (changed == 0) {
            converged = 1;
            break;
        }
        if (iterations == max_iterations) break;
        hipLaunchKernelGGL(kmeans_average_kernel, update_grid, dim3(kBlock), 0, stream, cohort->d_planes, N, padded, S, sp.ctl, sp.used,
                           sp.members, false, cent_c, cent_b, kMaxK);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(kmeans_finish_kernel, cohort_grid_per(cohort, std::max<uint64_t>(S, (uint64_t)K * N), kBlock, kManyBlocks), dim3(kBlock), 0, stream, sp.ctl,
                       cohort->d_total, sp.used, sp.assign, sp.dist, sp.members, sp.cent, S, N, K, iterations, converged,
                       static_cast<epik_amd_kmeans_sample *>(d_samples), static_cast<epik_amd_kmeans_cluster *>(d_clusters),
                       static_cast<double *>(d_centroids), static_cast<epik_amd_kmeans_info *>(d_info));
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

}  // namespace

extern "C" {

int epik_amd_cohort_kmeans_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                                  uint32_t num_clusters, uint32_t max_iterations, void *d_samples, void *d_clusters,
                                  void *d_centroids, void *d_info, void *stream)
{
    return guarded("cohort_kmeans_device", [&]() -> int {
        return kmeans_device_impl(cohort, tree, branch_length, num_clusters, max_iterations, d_samples, d_clusters, d_centroids, d_info,
                                  static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_kmeans(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                           uint32_t num_clusters, uint32_t max_iterations, epik_amd_kmeans_sample *samples,
                           epik_amd_kmeans_cluster *clusters, double *centroids, epik_amd_kmeans_info *info)
{
    return guarded("cohort_kmeans", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(check_present(samples, clusters, centroids, info));
        COHORT_TRY(check_counts(num_clusters, max_iterations));
        const size_t S = cohort->num_samples, N = cohort->num_branches, K = num_clusters;
        const size_t sample_bytes = S * sizeof(epik_amd_kmeans_sample), cluster_bytes = K * sizeof(epik_amd_kmeans_cluster);
        const size_t centroid_bytes = K * N * sizeof(double);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult r;
        // the centroids, the samples, the clusters, then the info block: every part begins on a multiple of 8
        const size_t samples_at = centroid_bytes, clusters_at = samples_at + sample_bytes, info_at = clusters_at + cluster_bytes;
        COHORT_TRY(r.alloc(info_at + sizeof(epik_amd_kmeans_info)));
        COHORT_TRY(kmeans_device_impl(cohort, tree, branch_length, num_clusters, max_iterations, r.at(samples_at), r.at(clusters_at), r.d,
                                      r.at(info_at), nullptr));
        COHORT_TRY(r.copy_to(centroids, centroid_bytes));
        COHORT_TRY(r.copy_to(samples, sample_bytes, samples_at));
        COHORT_TRY(r.copy_to(clusters, cluster_bytes, clusters_at));
        return r.copy_to(info, sizeof(epik_amd_kmeans_info), info_at);
    });
}

int epik_amd_cohort_kmeans_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                const double *branch_length, uint32_t num_clusters, uint32_t max_iterations,
                                epik_amd_kmeans_sample *samples, epik_amd_kmeans_cluster *clusters, double *centroids,
                                epik_amd_kmeans_info *info)
{
    return guarded("cohort_kmeans_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(check_present(mass, first, branch_length, samples, clusters, centroids, info));
        std::string err;
        return rule_result(kmeans_clusters(mass, num_samples, num_branches, first, branch_length, num_clusters, max_iterations, samples,
                                           clusters, centroids, info, err),
                           err);
    });
}

}  // extern "C"
