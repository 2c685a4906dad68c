// cohort_device.hpp -- what the cohort analyses share of a device cohort.  For the host: the object itself with its workspace
// slots, and the enqueue calls that one analysis offers the others (the normalise and distance kernels, the mass plane, the
// index of the used samples).  For the kernels (under __HIPCC__): NA, the Gower centring of a distance matrix, a branch's
// vectors and midranks, the permutation key and rank, the strata rule's tables and arrangement, and a column's list and
// groups.  The host code around the kernels is in cohort_entry.hpp.
#ifndef EPIK_AMD_COHORT_DEVICE_HPP
#define EPIK_AMD_COHORT_DEVICE_HPP

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "epik_amd.h"
#include "host_entry.hpp"

// a workspace of one analysis on the cohort's device
struct CohortSpace {
    void *d = nullptr;
    size_t bytes = 0;
};

// one entry a workspace (kSpaceRarefy: the curve's partials, beside the counts and the alpha partials of kSpaceDiversity)
enum CohortSpaceId : uint32_t {
    kSpaceSquash,
    kSpaceEpca,
    kSpacePcoa,
    kSpaceKmeans,
    kSpaceDiversity,
    kSpaceRarefy,
    kSpaceCorrelation,
    kSpacePermanova,
    kSpaceEdgetest,
    kSpacePermdisp,
    kSpaceModel,
    kSpaceMantel,
    kSpaceEdgemodel,
    kCohortSpaces
};

struct epik_amd_cohort {
    int device = 0;
    uint32_t num_samples = 0, num_branches = 0, keep = 0;
    bool lds = false;             // latched at create(): the LDS path
    uint32_t lds_blocks = 0;      // ... and its grid: kMaxBlocks, or a workgroup per CU for the trees beyond kLdsBudget
    uint32_t max_blocks_cap = 0;  // the placer's EPIK_AMD_MAX_BLOCKS
    uint64_t *d_cells = nullptr;  // [S] x (mass[N] | best[N] | totals[kTotals]) | bad_samples
    // the workspace of the KR distance, allocated by the first kr_device:
    uint64_t *d_prefix = nullptr;  // [S][N]: inclusive prefix sums of mass
    uint64_t *d_total = nullptr;   // [S]: T_s
    double *d_planes = nullptr;    // C[N][Sp] | B[N][Sp]
    double *d_half = nullptr;      // [N]: 0.5 * branch_length
    // the workspaces of the analyses, each allocated by its first call and grown by a call that needs more
    // (cohort_entry.hpp: cohort_space_ensure)
    CohortSpace space[kCohortSpaces];
};

namespace epik_amd {

constexpr uint32_t kCohortTile = 32;  // samples a side of a tile of pairs: the planes' sample pitch is a multiple of it
inline uint32_t cohort_padded_samples(const epik_amd_cohort *cohort)
{
    return (cohort->num_samples + kCohortTile - 1) / kCohortTile * kCohortTile;
}

// the checks of the cohort and the tree (device, N), the device drained, the workspace of the planes, then the normalise
// kernel on `stream`: T_s in d_total, C and B in d_planes; *d_first: the tree's first[] on the device
int cohort_normalise_enqueue(epik_amd_cohort *cohort, const epik_amd_tree *tree, hipStream_t stream, const uint32_t **d_first);

// epik_amd_cohort_kr_device: the checks, the workspace, the lengths, then the normalise and distance kernels on `stream`
int cohort_kr_enqueue(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, void *d_out,
                      hipStream_t stream);

// unifrac_place.hip: the matrix of distance `metric` (EPIK_AMD_DISTANCE_*) into d_out on `stream`: cohort_kr_enqueue for KR,
// epik_amd_cohort_unifrac_device for the UniFrac distances; any other metric is refused with a message that names it
int cohort_distance_enqueue(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                            void *d_out, hipStream_t stream);

// correlation_place.hip: the checks of epca_device, the device drained, T_s and the planes C and B, the workspace of the
// correlation, then xm as a plane [N][Sp], sample-fastest, on `stream`: *d_first the tree's first[], *d_X the plane
int cohort_mass_plane_enqueue(epik_amd_cohort *cohort, const epik_amd_tree *tree, hipStream_t stream, const uint32_t **d_first,
                              const double **d_X);

// The used samples (T_s > 0 in d_total, which the normalise kernel left) in ascending s, enqueued on `stream`: used[j], jof[s]
// (kCohortNoIndex for a sample without mass) and L into *count, all uint32 in device memory.  What the edge principal
// components and the principal coordinates start from (cohort_place.hip).
constexpr uint32_t kCohortNoIndex = 0xffffffffu;
int cohort_used_index_enqueue(const epik_amd_cohort *cohort, uint32_t *used, uint32_t *jof, uint32_t *count, hipStream_t stream);

constexpr uint32_t kCohortLdsSamples = 1024;   // the most samples whose four vectors stay in LDS (32 KiB)
constexpr uint32_t kCohortCountSamples = 128;  // up to here the LDS path counts its ranks; beyond, it sorts
constexpr uint32_t kCohortKeyTile = 1024;      // the keys a workgroup ranks a labelling against at a time (permutation_rank)
static_assert(kBlock == 256 && kCohortLdsSamples % kBlock == 0 && 2 * kCohortCountSamples <= kCohortLdsSamples);

#ifdef __HIPCC__
// NA is stored as its bit pattern and never computed
__device__ inline double na_value() { return __longlong_as_double((long long)EPIK_AMD_NA_BITS); }

// The Gower centring of the distances kr[S][S] among the L samples used[0 .. L), as pcoa_place.hip and model_place.hip form
// it; every sum is a sequential chain in the rule's order.
// B[i][j], i <= j, from the distance and the means
__device__ inline double gower_centred(double d, double ri, double rj, double g)
{
    return __dmul_rn(-0.5, __dadd_rn(__dsub_rn(__dsub_rn(__dmul_rn(d, d), ri), rj), g));
}

// r_i: the mean of the squared distances of row i
__device__ inline double gower_row_mean(const double *__restrict__ kr, const uint32_t *__restrict__ used, uint32_t num_samples,
                                        uint32_t L, uint32_t i)
{
    const double *column = kr + used[i];  // KR[u_j][u_i] = KR[u_i][u_j]
    double acc = 0.0;
#pragma unroll 4  // (the reads of four values are in flight ahead of the dependent adds)
    for (uint32_t j = 0; j < L; ++j) {  // ascending: the rule's order
        const double d = column[(uint64_t)used[j] * num_samples];
        acc = __dadd_rn(acc, __dmul_rn(d, d));
    }
    return __ddiv_rn(acc, (double)L);
}

// g: the mean of r[0 .. L) (0.0 of no sample); one lane's work
__device__ inline double gower_mean_of_means(const double *__restrict__ r, uint32_t L)
{
    double g = 0.0;
    for (uint32_t i = 0; i < L; ++i) g = __dadd_rn(g, r[i]);  // ascending: the rule's order
    if (L) g = __ddiv_rn(g, (double)L);
    return g;
}

// B[L][L], a grid of workgroups of kBlock lanes striding over the cells
__device__ inline void gower_centre_cells(const double *__restrict__ kr, const uint32_t *__restrict__ used, uint32_t num_samples,
                                          uint32_t L, const double *__restrict__ r, double g, double *__restrict__ B)
{
    const uint64_t cells = (uint64_t)L * L;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock) {
        const uint32_t i = (uint32_t)(e / L), j = (uint32_t)(e - (uint64_t)i * L), lo = i < j ? i : j, hi = i < j ? j : i;
        B[e] = gower_centred(kr[(uint64_t)used[lo] * num_samples + used[hi]], r[lo], r[hi], g);
    }
}

// the midrank of x_j among x[0 .. L): the rule's two counts
__device__ inline double midrank(const double *x, uint32_t L, double xj)
{
    uint32_t less = 0, equal = 0;
#pragma unroll 4
    for (uint32_t i = 0; i < L; ++i) {
        const double v = x[i];  // a broadcast
        less += v < xj, equal += v == xj;
    }
    return __dadd_rn((double)less, __dmul_rn(0.5, (double)(equal + 1)));
}

// the midrank of xj among the finite values of sorted[0 .. P), ascending (the padding is +inf): two binary searches, the
// number of values below xj and of those not above it -- the rule's two counts, found in another way
__device__ inline double midrank_sorted(const double *sorted, uint32_t P, double xj)
{
    uint32_t lo = 0, hi = P;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (sorted[mid] < xj) lo = mid + 1; else hi = mid;
    }
    const uint32_t less = lo;
    hi = P;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (sorted[mid] <= xj) lo = mid + 1; else hi = mid;
    }
    return __dadd_rn((double)less, __dmul_rn(0.5, (double)(lo - less + 1)));
}

// d[0 .. L) becomes d - mean(d); returns the sequential sum of the squares: one lane's work
__device__ inline double centre(double *d, uint32_t L, double *mean_out = nullptr)
{
    double acc = 0.0;
    for (uint32_t j = 0; j < L; ++j) acc = __dadd_rn(acc, d[j]);
    const double mean = __ddiv_rn(acc, (double)L);
    if (mean_out) *mean_out = mean;
    double ss = 0.0;
    for (uint32_t j = 0; j < L; ++j) {
        const double dev = __dsub_rn(d[j], mean);
        d[j] = dev;
        ss = __dadd_rn(ss, __dmul_rn(dev, dev));
    }
    return ss;
}

// A workgroup of kBlock lanes: xm and xi of a branch over the L samples of `list` into vec[0 .. L) and vec[pitch ..], and
// with kRanks their midranks into vec[2 pitch ..] and vec[3 pitch ..] (xi and its ranks are 0.0 unless `inner`).  xrow, crow
// and brow are the branch's rows of the planes.  kLds: vec is LDS with pitch = kCohortLdsSamples, and beyond
// kCohortCountSamples samples the values are sorted in the ranks' place (a bitonic network over the next power of two, the
// padding +inf), every lane's ranks found in the sorted copy and kept in registers, then stored over it; else a lane ranks
// its j against broadcasts of all i.  The ranks are exact either way.  Every condition around a barrier is uniform; the
// vectors are complete when it returns.
template <bool kLds, bool kRanks>
__device__ inline void branch_vectors(const double *__restrict__ xrow, const double *__restrict__ crow, const double *__restrict__ brow,
                                      const uint32_t *__restrict__ list, uint32_t L, bool inner, double *vec, uint32_t pitch)
{
    for (uint32_t j = threadIdx.x; j < L; j += kBlock) {
        const uint32_t s = list[j];
        vec[j] = xrow[s];
        vec[pitch + j] = inner ? __dsub_rn(__dadd_rn(brow[s], crow[s]), 1.0) : 0.0;
    }
    __syncthreads();
    if (kRanks && kLds && L > kCohortCountSamples) {
        double *sm = vec + 2 * pitch, *si = vec + 3 * pitch;
        uint32_t P = 2 * kCohortCountSamples;
        while (P < L) P <<= 1;  // (<= kCohortLdsSamples)
        for (uint32_t j = threadIdx.x; j < P; j += kBlock) {
            sm[j] = j < L ? vec[j] : HUGE_VAL;
            si[j] = j < L ? vec[pitch + j] : HUGE_VAL;
        }
        __syncthreads();
        for (uint32_t k = 2; k <= P; k <<= 1)
            for (uint32_t step = k >> 1; step > 0; step >>= 1) {
                for (uint32_t e = threadIdx.x; e < P / 2; e += kBlock) {
                    const uint32_t i = 2 * e - (e & (step - 1)), l = i + step;  // (l < P)
                    const bool up = (i & k) == 0;
                    const double a = sm[i], c = sm[l];
                    if ((a > c) == up) sm[i] = c, sm[l] = a;
                    if (inner) {
                        const double ai = si[i], ci = si[l];
                        if ((ai > ci) == up) si[i] = ci, si[l] = ai;
                    }
                }
                __syncthreads();
            }
        double rank_m[kCohortLdsSamples / kBlock], rank_i[kCohortLdsSamples / kBlock];
#pragma unroll
        for (uint32_t q = 0; q < kCohortLdsSamples / kBlock; ++q) {
            const uint32_t j = q * kBlock + threadIdx.x;
            rank_m[q] = j < L ? midrank_sorted(sm, P, vec[j]) : 0.0;
            rank_i[q] = j < L && inner ? midrank_sorted(si, P, vec[pitch + j]) : 0.0;
        }
        __syncthreads();  // (every search is done: the sorted copies become the ranks)
#pragma unroll
        for (uint32_t q = 0; q < kCohortLdsSamples / kBlock; ++q) {
            const uint32_t j = q * kBlock + threadIdx.x;
            if (j < L) sm[j] = rank_m[q], si[j] = rank_i[q];
        }
        __syncthreads();
    } else if (kRanks) {
        for (uint32_t j = threadIdx.x; j < L; j += kBlock) {
            vec[2 * pitch + j] = midrank(vec, L, vec[j]);
            vec[3 * pitch + j] = inner ? midrank(vec + pitch, L, vec[pitch + j]) : 0.0;
        }
        __syncthreads();
    }
}

// the PERMANOVA rule's key of position i in permutation p: the splitmix64 finaliser of a counter
__device__ inline uint64_t permutation_key(uint64_t seed, uint32_t p, uint32_t i)
{
    uint64_t z = seed + (((uint64_t)p << 32) | i) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// A workgroup of kBlock lanes, every lane calling it (it has barriers; L and p are uniform): rank_p(i) of the PERMANOVA rule
// among the L positions, counted against tiles of keys in tile[kCohortKeyTile] (LDS).  Permutation 0 is the identity.  A
// lane whose i is not below L gets a number that means nothing.
__device__ inline uint32_t permutation_rank(uint64_t seed, uint32_t p, uint32_t i, uint32_t L, uint64_t *tile)
{
    if (p == 0) return i;  // (uniform)
    const uint64_t mine = permutation_key(seed, p, i);
    uint32_t rank = 0;
    for (uint32_t j0 = 0; j0 < L; j0 += kCohortKeyTile) {
        const uint32_t nt = min(kCohortKeyTile, L - j0);
        __syncthreads();  // (the tile is written again)
        for (uint32_t j = threadIdx.x; j < nt; j += kBlock) tile[j] = permutation_key(seed, p, j0 + j);
        __syncthreads();
#pragma unroll 4
        for (uint32_t j = 0; j < nt; ++j) {
            const uint64_t other = tile[j];  // a broadcast
            rank += other < mine || (other == mine && j0 + j < i);
        }
    }
    return rank;
}

// The strata rule's tables of one list of n positions, which do not depend on p.  A workgroup of any size, every lane calling
// it (it has barriers; n is uniform): hs[i] = the stratum of position i, from the strata by sample and sample_of(i), and
// home[], the positions by (stratum, position): home[base_i + index rank of i in its stratum] = i, base_i the positions in
// strata with a smaller id.  hs and home are the list's, in global memory or LDS.
template <class SampleOf>
__device__ inline void strata_tables(const uint32_t *__restrict__ strata, SampleOf sample_of, uint32_t n, uint32_t *hs, uint32_t *home)
{
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) hs[i] = strata[sample_of(i)];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t mine = hs[i];
        uint32_t slot = 0;
#pragma unroll 4
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t other = hs[j];  // a broadcast
            slot += other < mine || (other == mine && j < i);
        }
        home[slot] = i;  // (a bijection: slot < n)
    }
    __syncthreads();
}

// whether (stratum, key, position) of j comes before that of i: what places i among the positions of its own stratum, behind
// every stratum with a smaller id.  Only equality of strata decides sigma_p: home[] is in the same order of the ids.
__device__ inline bool strata_before(uint32_t hj, uint64_t kj, uint32_t j, uint32_t hi, uint64_t ki, uint32_t i)
{
    return hj < hi || (hj == hi && (kj < ki || (kj == ki && j < i)));
}

// permutation_rank's stratified sibling, called the same way: sigma_p(i) = home[base_i + w_p(i)] of the strata rule, with hs and
// home from strata_tables.  The tile carries the strata beside the keys (htile[kCohortKeyTile], LDS), and the count runs on
// over the tiles, so a stratum may straddle them.  Permutation 0 is the identity.
__device__ inline uint32_t permutation_arrangement(uint64_t seed, uint32_t p, uint32_t i, uint32_t L, uint64_t *tile, uint32_t *htile,
                                                   const uint32_t *__restrict__ hs, const uint32_t *__restrict__ home)
{
    if (p == 0) return i;  // (uniform)
    const uint64_t mine = permutation_key(seed, p, i);
    const uint32_t stratum = i < L ? hs[i] : 0;
    uint32_t slot = 0;
    for (uint32_t j0 = 0; j0 < L; j0 += kCohortKeyTile) {
        const uint32_t nt = min(kCohortKeyTile, L - j0);
        __syncthreads();  // (the tile is written again)
        for (uint32_t j = threadIdx.x; j < nt; j += kBlock) tile[j] = permutation_key(seed, p, j0 + j), htile[j] = hs[j0 + j];
        __syncthreads();
#pragma unroll 4
        for (uint32_t j = 0; j < nt; ++j) slot += strata_before(htile[j], tile[j], j0 + j, stratum, mine, i);  // broadcasts
    }
    return i < L ? home[slot] : 0;  // (slot < L)
}

// the lanes of a wave whose `flag` is set append (sample, group) to the list in the order of the lanes; returns how many did
__device__ inline uint32_t append_in_order(bool flag, uint32_t at, uint32_t sample, uint32_t group, uint32_t *__restrict__ idx,
                                           uint8_t *__restrict__ lam)
{
    const unsigned long long mask = __ballot(flag);
    if (flag) {
        const uint32_t pos = at + __popcll(mask & ((1ull << threadIdx.x) - 1));
        idx[pos] = sample, lam[pos] = (uint8_t)group;
    }
    return __popcll(mask);
}

// One wave (a workgroup of kWave lanes): the PERMANOVA rule's U_c of a column in list order into idx and lam, its groups
// numbered by first appearance (ballots keep the order) and their sizes.  lab: the column's labels by sample, each below
// kGroups (a power of two) or `missing`; group_of[kGroups] and size[kGroups] are the workgroup's, in LDS.  L and G are uniform.
template <uint32_t kGroups>
__device__ inline void column_list(const uint64_t *__restrict__ total, const uint32_t *__restrict__ lab, uint32_t num_samples,
                                   uint32_t missing, uint32_t *group_of, uint32_t *size, uint32_t *__restrict__ idx,
                                   uint8_t *__restrict__ lam, uint32_t &L, uint32_t &G)
{
    for (uint32_t g = threadIdx.x; g < kGroups; g += kWave) group_of[g] = missing, size[g] = 0;
    __syncthreads();
    L = 0, G = 0;
    for (uint32_t base = 0; base < num_samples; base += kWave) {
        const uint32_t s = base + threadIdx.x;
        const uint32_t v = s < num_samples ? lab[s] : missing;
        const bool flag = s < num_samples && total[s] != 0 && v != missing;  // (v < kGroups: the host has checked)
        for (;;) {  // the labels not seen before take the next numbers, the first lane first
            const unsigned long long fresh = __ballot(flag && group_of[v & (kGroups - 1)] == missing);
            if (!fresh) break;
            if (threadIdx.x == (uint32_t)__ffsll((long long)fresh) - 1) group_of[v] = G;
            ++G;
            __syncthreads();
        }
        const uint32_t g = flag ? group_of[v] : 0;
        if (flag) atomicAdd(&size[g], 1u);
        L += append_in_order(flag, L, s, g, idx, lam);
    }
    __syncthreads();
}
#endif

}  // namespace epik_amd
#endif
