// edgetest_place.hip -- the edge test of a cohort's samples on the device: on which branches do the groups of a factor column
// differ?  A one-way ANOVA and a Kruskal-Wallis test per branch, of its mass and of its imbalance, by permutation, with the
// single-step max-statistic adjustment (Westfall & Young 1993).  epik_amd_cohort_edgetest_device / _edgetest / _edgetest_host
// (include/epik_amd.h).
//
// No reference counterpart.  The rule is stated once, in include/epik_amd.h after the PERMANOVA rule (DESIGN.md 3.16;
// epik_amd/host/cohort.cpp: edgetest_records is the same rule on the CPU).  Every sum is a sequential chain from +0.0 in one
// lane (__dadd_rn / __dsub_rn / __dmul_rn / __ddiv_rn; the file is built with -ffp-contract=off as well); ranks and counts
// are integers; a maximum of doubles that are >= +0.0 is a maximum of their bit patterns.  NA is stored as its bit pattern
// and never computed.
//
// cohort_mass_plane_enqueue (correlation_place.hip) leaves T_s, the planes C and B, and xm as a plane [b][Sp].  Then
//
//   edgetest_columns_kernel     a wave a column: U_c in list order and the groups by first appearance (column_list,
//                               cohort_device.hpp: PERMANOVA's).
//   and, one column after another in the same workspace,
//   edgetest_observed_kernel    a workgroup a branch: xm, xi and their midranks over U_c (branch_vectors, cohort_device.hpp:
//                               the correlation's), in LDS or, beyond kLdsPositions samples, in the workgroup's slice of global
//                               memory; a lane a family centres its vector (mx, d, sxx); the deviations go to the plane
//                               D[b][f][Sp]; a lane a (family, group) sums lambda's S_g; a lane a family writes the record's
//                               observed half.  A branch with a defined family joins the list of the branches to permute.
//   edgetest_labellings_kernel  a workgroup a labelling of the chunk (kChunk labellings, p = p0 ..): the keys ranked by
//                               counting against tiles of keys in LDS; mu as a byte a position, four positions of a labelling
//                               in a word, the labellings of a word-row side by side: MU[i / 4][k] -- neighbouring lanes read
//                               neighbouring labellings.
//   edgetest_chains_kernel      a workgroup a (listed branch, blockDim.x labellings), a lane a labelling: it walks the
//                               positions in ascending order and adds d_i into the accumulator of mu_i, two families at a
//                               time from one read of mu.  kG = 2 or 4: the accumulators of G <= kG groups in registers (a
//                               chain never holds -0.0, so adding +0.0 to the other groups' leaves their bits: no branch);
//                               kG = 0: in LDS, [g][lane], one family at a time.  The two deviation vectors in LDS, or read
//                               from D beyond kLdsPositions samples.  eta into stat; the count of eta >= eta2 by a ballot and
//                               one vector atomic add a wave; the maximum over a workgroup's branches in a register, then a
//                               vector atomic max on the bit patterns.
//   edgetest_finish_kernel      max_at_least, p and p_adj of every defined family; NA into stat where undefined; max.
//   edgetest_strata_kernel      with strata only (the strata rule): the tables of every column's list, once a
//                               call; edgetest_labellings_kernel<true> then takes sigma_p (permutation_arrangement) for the rank.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kColumns = EPIK_AMD_EDGETEST_MAX_COLUMNS;
constexpr uint32_t kGroups = EPIK_AMD_EDGETEST_MAX_GROUPS;
constexpr uint32_t kFamilies = EPIK_AMD_EDGETEST_FAMILIES;
constexpr uint32_t kMissing = EPIK_AMD_EDGETEST_MISSING;
constexpr uint32_t kLdsPositions = kCohortLdsSamples;  // the most samples whose vectors stay in LDS
constexpr uint32_t kRegisterGroups = 4;                // up to here the accumulators of a lane are registers (2 or 4 a family)
constexpr uint32_t kChunk = 1024;                      // the labellings made at a time
constexpr uint32_t kLdsLanes = 128;                    // the lanes of a workgroup whose accumulators are in LDS (32 KiB at G = 32)
constexpr uint32_t kKeyTile = kCohortKeyTile;          // the keys a workgroup ranks against at a time
constexpr uint32_t kGeneralBlocks = 256;               // workgroups of the observed kernel's general path: each has a slice
constexpr uint64_t kManyBlocks = 65536;

static_assert(sizeof(epik_amd_edgetest_family) == 48 && sizeof(epik_amd_edgetest) == 208, "the record is 208 bytes");
static_assert(offsetof(epik_amd_edgetest, family) == 8 && offsetof(epik_amd_edgetest, top_mass) == 200);
static_assert(kFamilies == 4 && kBlock == 256 && kWave == 64 && kChunk % kBlock == 0 && kChunk % kLdsLanes == 0);
static_assert((kGroups & (kGroups - 1)) == 0 && kFamilies * kGroups <= kBlock);

struct EdgeColumn {
    uint32_t used, groups;
    uint32_t size[kGroups];
};

struct EdgeSpace {
    double *D;         // [N][4][Sp]: the deviations of the column at hand
    double *scratch;   // [kGeneralBlocks][4][Sp]
    double *sxx;       // [N][4]
    uint64_t *mmax;    // [4][P + 1]: the bit patterns of Mmax
    uint32_t *MU;      // [Sp / 4][kChunk]: four positions of a labelling a word
    uint32_t *lab;     // [M][Sp]: the labels by sample
    uint32_t *idx;     // [M][Sp]: the samples of the positions
    uint32_t *defined; // [N]: bit f: family f of the branch is defined
    uint32_t *active;  // [N] the branches to permute, then their number, then the defined branches of the four families
    EdgeColumn *cols;  // [M]
    uint8_t *lam;      // [M][Sp]: the groups of the positions
    uint32_t *strata;  // with strata only: [Sp], the strata by sample
    uint32_t *hs, *home;  // ... and [M][Sp]: the strata of the positions, and the positions by (stratum, position)
};

size_t edgetest_space(void *base, uint32_t N, uint32_t padded, uint32_t M, uint32_t P, bool strata, EdgeSpace *sp)
{
    Carver c(base);
    const EdgeSpace parts{.D = c.take<double>((size_t)N * kFamilies * padded),
                          .scratch = c.take<double>((size_t)kGeneralBlocks * kFamilies * padded),
                          .sxx = c.take<double>((size_t)N * kFamilies),
                          .mmax = c.take<uint64_t>((size_t)kFamilies * ((size_t)P + 1)),
                          .MU = c.take<uint32_t>((size_t)padded * kChunk / 4),
                          .lab = c.take<uint32_t>((size_t)M * padded),
                          .idx = c.take<uint32_t>((size_t)M * padded),
                          .defined = c.take<uint32_t>(N),
                          .active = c.take<uint32_t>((size_t)N + 1 + kFamilies),
                          .cols = c.take<EdgeColumn>(M),
                          .lam = c.take<uint8_t>((size_t)M * padded),
                          .strata = c.take<uint32_t>(strata ? padded : 0),
                          .hs = c.take<uint32_t>(strata ? (size_t)M * padded : 0),
                          .home = c.take<uint32_t>(strata ? (size_t)M * padded : 0)};
    if (sp) *sp = parts;
    return c.bytes();
}

__global__ __launch_bounds__(kWave) void edgetest_columns_kernel(const uint64_t *__restrict__ total, const uint32_t *__restrict__ lab,
                                                                 uint32_t num_samples, uint32_t padded, uint32_t num_columns,
                                                                 uint32_t *__restrict__ idx, uint8_t *__restrict__ lam,
                                                                 EdgeColumn *__restrict__ cols)
{
    __shared__ uint32_t group_of[kGroups], size[kGroups];
    for (uint32_t c = blockIdx.x; c < num_columns; c += gridDim.x) {
        const uint64_t offset = (uint64_t)c * padded;
        uint32_t L, G;  // (uniform)
        column_list<kGroups>(total, lab + offset, num_samples, kMissing, group_of, size, idx + offset, lam + offset, L, G);
        for (uint32_t g = threadIdx.x; g < kGroups; g += kWave) cols[c].size[g] = size[g];
        if (threadIdx.x == 0) cols[c].used = L, cols[c].groups = G;
        __syncthreads();  // (the tables are written again)
    }
}

__device__ inline uint32_t vector_of(uint32_t family) { return (family & 1u) * 2 + (family >> 1); }

struct EdgeArgs {
    const double *X, *planes;
    const uint32_t *first;
    EdgeSpace sp;
    epik_amd_edgetest *out;  // the column's records
    double *stat;            // the column's [4][N][P + 1], or null
    double *max;             // the column's [4][P + 1], or null
    uint64_t seed;
    uint32_t column, num_branches, padded, num_permutations;
    uint32_t p0, np;         // the chunk: the labellings p0 .. p0 + np - 1
};

template <bool kLds>
__global__ __launch_bounds__(kBlock) void edgetest_observed_kernel(const EdgeArgs a)
{
    __shared__ double lds_vec[kLds ? kFamilies * kLdsPositions : 1];
    __shared__ double sxx_of[kFamilies], sum_of[kFamilies * kGroups];
    const uint32_t tid = threadIdx.x, N = a.num_branches, padded = a.padded, c = a.column;
    const uint32_t pitch = kLds ? kLdsPositions : padded;
    double *vec = kLds ? lds_vec : a.sp.scratch + (uint64_t)blockIdx.x * kFamilies * padded;
    const double *C = a.planes, *B = a.planes + (uint64_t)N * padded;
    const EdgeColumn *col = a.sp.cols + c;
    const uint32_t L = col->used, G = col->groups;
    const uint32_t *list = a.sp.idx + (uint64_t)c * padded;
    const uint8_t *lam = a.sp.lam + (uint64_t)c * padded;
    const bool column_defined = G >= 2 && L >= G + 1;  // (uniform, as is every condition around a barrier below)
    for (uint32_t b = blockIdx.x; b < N; b += gridDim.x) {
        const bool inner = a.first[b] < b;
        const uint32_t nf = inner ? kFamilies : 2;
        epik_amd_edgetest *r = a.out + b;
        if (column_defined) {
            branch_vectors<kLds, true>(a.X + (uint64_t)b * padded, C + (uint64_t)b * padded, B + (uint64_t)b * padded, list, L, inner,
                                       vec, pitch);
            // (family f is the vector (f & 1) * 2 + (f >> 1) of branch_vectors: xm, xi, rank(xm), rank(xi))
            if (tid % kWave == 0 && tid / kWave < nf) sxx_of[tid / kWave] = centre(vec + vector_of(tid / kWave) * pitch, L);  // a wave a family
            __syncthreads();
            for (uint32_t f = 0; f < nf; ++f) {
                double *row = a.sp.D + ((uint64_t)b * kFamilies + f) * padded;
                for (uint32_t i = tid; i < L; i += kBlock) row[i] = vec[vector_of(f) * pitch + i];
            }
            if (tid < nf * G) {
                const uint32_t f = tid / G, g = tid % G;
                const double *d = vec + vector_of(f) * pitch;
                double acc = 0.0;
#pragma unroll 4
                for (uint32_t i = 0; i < L; ++i)
                    if (lam[i] == g) acc = __dadd_rn(acc, d[i]);
                sum_of[f * kGroups + g] = acc;
            }
            __syncthreads();
        }
        if (tid < kFamilies) {
            const uint32_t f = tid;
            epik_amd_edgetest_family fam{na_value(), na_value(), na_value(), na_value(), 0, 0};
            uint32_t top = kMissing;
            const double sxx = column_defined && f < nf ? sxx_of[f] : 0.0;
            const bool defined = sxx > 0.0;
            if (defined) {
                double among = 0.0;
                for (uint32_t g = 0; g < G; ++g)
                    among = __dadd_rn(among, __ddiv_rn(__dmul_rn(sum_of[f * kGroups + g], sum_of[f * kGroups + g]), (double)col->size[g]));
                fam.eta2 = __ddiv_rn(among, sxx);
                if (f % 2 == 0) {
                    const double ssw = __dsub_rn(sxx, among);
                    if (ssw > 0.0) fam.stat = __ddiv_rn(__ddiv_rn(among, (double)(G - 1)), __ddiv_rn(ssw, (double)(L - G)));
                    top = 0;
                    double best = __ddiv_rn(sum_of[f * kGroups], (double)col->size[0]);
                    for (uint32_t g = 1; g < G; ++g) {
                        const double mean = __ddiv_rn(sum_of[f * kGroups + g], (double)col->size[g]);
                        if (mean > best) best = mean, top = g;
                    }
                } else {
                    fam.stat = __dmul_rn((double)(L - 1), fam.eta2);
                }
                atomicAdd(a.sp.active + N + 1 + f, 1u);
            }
            r->family[f] = fam;
            a.sp.sxx[(uint64_t)b * kFamilies + f] = sxx;
            if (f == 0) r->used = L, r->groups = G, r->top_mass = top;
            if (f == 2) r->top_imbalance = top;
            const uint32_t mask = (uint32_t)__ballot(defined) & 0xfu;  // (the four lanes are the first of wave 0)
            if (f == 0) {
                a.sp.defined[b] = mask;
                if (mask) a.sp.active[atomicAdd(a.sp.active + N, 1u)] = b;
            }
        }
        __syncthreads();  // (the vectors and the sums are written again)
    }
}

// the strata rule's tables of every column's list: a workgroup a column
__global__ __launch_bounds__(kBlock) void edgetest_strata_kernel(const EdgeSpace sp, uint32_t num_columns, uint32_t padded)
{
    for (uint32_t c = blockIdx.x; c < num_columns; c += gridDim.x) {  // (uniform)
        const uint64_t at = (uint64_t)c * padded;
        const uint32_t *idx = sp.idx + at;
        strata_tables(sp.strata, [&](uint32_t i) { return idx[i]; }, sp.cols[c].used, sp.hs + at, sp.home + at);
    }
}

template <bool kStrata>
__global__ __launch_bounds__(kBlock) void edgetest_labellings_kernel(const EdgeArgs a)
{
    __shared__ uint64_t tile[kKeyTile];
    const uint32_t tid = threadIdx.x, c = a.column;
    const uint32_t L = a.sp.cols[c].used;
    const uint8_t *lam = a.sp.lam + (uint64_t)c * a.padded;
    uint8_t *mu8 = reinterpret_cast<uint8_t *>(a.sp.MU);
    if (a.sp.active[a.num_branches] == 0) return;  // (uniform: no branch to permute)
    for (uint32_t k = blockIdx.x; k < a.np; k += gridDim.x) {
        const uint32_t p = a.p0 + k;
        for (uint32_t base = 0; base < L; base += kBlock) {
            const uint32_t i = base + tid;
            uint32_t rank;  // (permutation 0 is the identity)
            if constexpr (kStrata) {
                __shared__ uint32_t htile[kKeyTile];
                rank = permutation_arrangement(a.seed, p, i, L, tile, htile, a.sp.hs + (uint64_t)c * a.padded, a.sp.home + (uint64_t)c * a.padded);
            } else {
                rank = permutation_rank(a.seed, p, i, L, tile);
            }
            if (i < L) mu8[((uint64_t)(i / 4) * kChunk + k) * 4 + i % 4] = lam[rank];  // (rank < L)
        }
    }
}

// a lane's labelling: the chains S_g of kF vectors d[q * pitch + i] over the positions, then A(mu) / sxx of each.
// kG != 0: G <= kG, the accumulators in registers; else in acc[g * lanes + lane] (LDS), kF = 1.
template <uint32_t kG, uint32_t kF>
__device__ inline void lane_chains(const double *d, uint32_t pitch, const uint32_t *__restrict__ mu, uint32_t L, uint32_t G,
                                   const uint32_t *size, const double *sxx, double *acc, uint32_t lanes, double *eta)
{
    constexpr uint32_t kAcc = kG ? kG : 1;
    double reg[kF][kAcc];
    if (kG) {
#pragma unroll
        for (uint32_t q = 0; q < kF; ++q)
#pragma unroll
            for (uint32_t g = 0; g < kAcc; ++g) reg[q][g] = 0.0;
    } else {
        for (uint32_t g = 0; g < G; ++g) acc[g * lanes] = 0.0;
    }
    const auto step = [&](uint32_t i, uint32_t m) {
        if (kG) {
#pragma unroll
            for (uint32_t q = 0; q < kF; ++q) {
                const double v = d[q * pitch + i];  // a broadcast
#pragma unroll
                for (uint32_t g = 0; g < kAcc; ++g) reg[q][g] = __dadd_rn(reg[q][g], m == g ? v : 0.0);  // (+0.0: the same bits)
            }
        } else {
            acc[m * lanes] = __dadd_rn(acc[m * lanes], d[i]);
        }
    };
    const uint32_t words = L / 4;
#pragma unroll 2
    for (uint32_t w = 0; w < words; ++w) {
        const uint32_t four = mu[(uint64_t)w * kChunk];
        step(4 * w, four & 0xffu), step(4 * w + 1, (four >> 8) & 0xffu), step(4 * w + 2, (four >> 16) & 0xffu), step(4 * w + 3, four >> 24);
    }
    if (L % 4) {
        const uint32_t four = mu[(uint64_t)words * kChunk];
        for (uint32_t i = 4 * words; i < L; ++i) step(i, (four >> (8 * (i % 4))) & 0xffu);
    }
#pragma unroll
    for (uint32_t q = 0; q < kF; ++q) {
        double among = 0.0;
        if (kG) {
#pragma unroll
            for (uint32_t g = 0; g < kAcc; ++g)
                if (g < G) among = __dadd_rn(among, __ddiv_rn(__dmul_rn(reg[q][g], reg[q][g]), (double)size[g]));
        } else {
            for (uint32_t g = 0; g < G; ++g) {
                const double s = acc[g * lanes];
                among = __dadd_rn(among, __ddiv_rn(__dmul_rn(s, s), (double)size[g]));
            }
        }
        eta[q] = __ddiv_rn(among, sxx[q]);
    }
}

template <uint32_t kG, bool kLds>
__global__ __launch_bounds__(kBlock) void edgetest_chains_kernel(const EdgeArgs a)
{
    extern __shared__ __align__(16) unsigned char dynamic_lds[];
    __shared__ uint32_t size[kGroups];
    const uint32_t tid = threadIdx.x, lanes = blockDim.x, N = a.num_branches, padded = a.padded, c = a.column;
    const uint32_t P = a.num_permutations;
    const uint64_t row = (uint64_t)P + 1;
    double *lds_d = reinterpret_cast<double *>(dynamic_lds);                   // kLds: [2][padded]
    double *lds_acc = lds_d + (kLds ? 2 * padded : 0);                          // kG == 0: [G][lanes]
    const EdgeColumn *col = a.sp.cols + c;
    const uint32_t L = col->used, G = col->groups, listed = a.sp.active[N];
    if (listed == 0) return;  // (uniform)
    if (tid < kGroups) size[tid] = col->size[tid];
    __syncthreads();
    // the workgroups as `across` groups of labellings times `down` workers a group, so that a workgroup's branches share
    // its labellings and their maximum stays in a register
    const uint32_t subs = (a.np + lanes - 1) / lanes, across = min(gridDim.x, subs), down = max(1u, gridDim.x / subs);
    if (blockIdx.x >= across * down) return;  // (uniform)
    for (uint32_t sub = blockIdx.x % across; sub < subs; sub += across) {
        const uint32_t k = sub * lanes + tid, p = a.p0 + k;
        const bool live = k < a.np;
        const uint32_t *mu = a.sp.MU + (live ? k : 0);
        uint64_t most[kFamilies] = {0, 0, 0, 0};
        for (uint32_t at = blockIdx.x / across; at < listed; at += down) {
            const uint32_t b = a.sp.active[at], mask = a.sp.defined[b];
            for (uint32_t pair = 0; pair < 2; ++pair) {
                if (!((mask >> (2 * pair)) & 3u)) continue;  // (uniform)
                const double *d = a.sp.D + ((uint64_t)b * kFamilies + 2 * pair) * padded;
                const double *sxx = a.sp.sxx + (uint64_t)b * kFamilies + 2 * pair;
                if (kLds) {
                    __syncthreads();  // (the vectors are written again)
                    for (uint32_t i = tid; i < L; i += lanes) lds_d[i] = d[i], lds_d[padded + i] = d[padded + i];
                    __syncthreads();
                    d = lds_d;
                }
                double eta[2];
                if (kG) {
                    lane_chains<kG, 2>(d, padded, mu, L, G, size, sxx, nullptr, 0, eta);
                } else {
                    lane_chains<0, 1>(d, padded, mu, L, G, size, sxx, lds_acc + tid, lanes, eta);
                    lane_chains<0, 1>(d + padded, padded, mu, L, G, size, sxx + 1, lds_acc + tid, lanes, eta + 1);
                }
                for (uint32_t q = 0; q < 2; ++q) {
                    const uint32_t f = 2 * pair + q;
                    if (!((mask >> f) & 1u)) continue;  // (uniform)
                    epik_amd_edgetest_family *fam = &a.out[b].family[f];
                    const double value = eta[q];
                    const unsigned long long bits = (unsigned long long)__double_as_longlong(value);
                    if (live) {
                        if (a.stat) a.stat[((uint64_t)f * N + b) * row + p] = value;
                        if (bits > most[f]) most[f] = bits;
                    }
                    const unsigned long long count = __popcll(__ballot(live && p >= 1 && value >= fam->eta2));
                    if (tid % kWave == 0 && count) atomicAdd(reinterpret_cast<unsigned long long *>(&fam->at_least), count);
                }
            }
        }
        if (live)
            for (uint32_t f = 0; f < kFamilies; ++f)
                if (most[f]) atomicMax(reinterpret_cast<unsigned long long *>(a.sp.mmax + f * row + p), (unsigned long long)most[f]);
    }
}

__global__ __launch_bounds__(kBlock) void edgetest_finish_kernel(const EdgeArgs a)
{
    const uint32_t N = a.num_branches, P = a.num_permutations;
    const uint64_t row = (uint64_t)P + 1, units = (uint64_t)N * kFamilies;
    const uint64_t start = (uint64_t)blockIdx.x * kBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kBlock;
    const double *mmax = reinterpret_cast<const double *>(a.sp.mmax);
    for (uint64_t e = start; e < units; e += stride) {
        const uint32_t b = (uint32_t)(e / kFamilies), f = (uint32_t)(e % kFamilies);
        if (!((a.sp.defined[b] >> f) & 1u)) continue;
        epik_amd_edgetest_family *fam = &a.out[b].family[f];
        const double eta2 = fam->eta2;
        const double *m = mmax + f * row;
        uint64_t count = 0;
#pragma unroll 4
        for (uint32_t p = 1; p <= P; ++p) count += m[p] >= eta2;
        fam->max_at_least = count;
        fam->p = __ddiv_rn((double)(1 + fam->at_least), (double)(P + 1));
        fam->p_adj = __ddiv_rn((double)(1 + count), (double)(P + 1));
    }
    if (a.max)
        for (uint64_t e = start; e < kFamilies * row; e += stride) a.max[e] = a.sp.active[N + 1 + e / row] ? mmax[e] : na_value();
    if (a.stat)
        for (uint64_t e = start; e < units * row; e += stride) {
            const uint64_t fb = e / row;  // f * N + b
            if (!((a.sp.defined[fb % N] >> (fb / N)) & 1u)) a.stat[e] = na_value();
        }
}

template <uint32_t kG>
void chains_launch(bool lds, dim3 grid, uint32_t lanes, size_t dynamic, hipStream_t stream, const EdgeArgs &args)
{
    if (lds)
        hipLaunchKernelGGL((edgetest_chains_kernel<kG, true>), grid, dim3(lanes), dynamic, stream, args);
    else
        hipLaunchKernelGGL((edgetest_chains_kernel<kG, false>), grid, dim3(lanes), dynamic, stream, args);
}

int check_arguments(const uint32_t *labels, uint32_t S, uint32_t M, uint32_t P)
{
    std::string err;
    return rule_result(edgetest_arguments_valid(labels, S, M, P, err), err);
}

int edgetest_device_impl(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *labels, const uint32_t *strata, uint32_t M,
                         uint32_t P, uint64_t seed, void *d_out, void *d_stat, void *d_max, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(check_columns(M));
    COHORT_TRY(check_present(tree, labels, d_out));
    const uint32_t S = cohort->num_samples, N = cohort->num_branches, padded = cohort_padded_samples(cohort);
    COHORT_TRY(check_arguments(labels, S, M, P));
    // the largest G of a column decides where the accumulators are: the distinct labels bound it
    const uint32_t most_groups = most_distinct_labels(labels, S, M, kMissing);
    const uint32_t *d_first = nullptr;
    const double *d_X = nullptr;
    // (the checks of the tree; the device drained of every call before: nothing reads the workspace)
    COHORT_TRY(cohort_mass_plane_enqueue(cohort, tree, stream, &d_first, &d_X));
    COHORT_TRY(cohort_space_ensure(cohort, kSpaceEdgetest, edgetest_space(nullptr, N, padded, M, P, strata != nullptr, nullptr)));
    EdgeSpace sp;
    edgetest_space(cohort->space[kSpaceEdgetest].d, N, padded, M, P, strata != nullptr, &sp);
    COHORT_TRY(upload_labels_by_column(labels, S, M, padded, kMissing, sp.lab));
    if (strata) COHORT_TRY(upload_strata(strata, S, padded, sp.strata));
    hipLaunchKernelGGL(edgetest_columns_kernel, cohort_grid(cohort, M, kColumns), dim3(kWave), 0, stream, cohort->d_total, sp.lab, S, padded, M,
                       sp.idx, sp.lam, sp.cols);
    if (strata) hipLaunchKernelGGL(edgetest_strata_kernel, cohort_grid(cohort, M, kColumns), dim3(kBlock), 0, stream, sp, M, padded);
    const bool lds = lds_switch("EPIK_AMD_EDGETEST_LDS", S, kLdsPositions);  // (=0, tests: the general path whatever S)
    const uint32_t lanes = most_groups <= kRegisterGroups ? kBlock : kLdsLanes;
    const size_t dynamic = (lds ? (size_t)2 * padded * 8 : 0) + (most_groups <= kRegisterGroups ? 0 : (size_t)most_groups * lanes * 8);
    const uint64_t row = (uint64_t)P + 1;
    for (uint32_t c = 0; c < M; ++c) {
        EdgeArgs args{d_X, cohort->d_planes, d_first, sp, static_cast<epik_amd_edgetest *>(d_out) + (size_t)c * N,
                      d_stat ? static_cast<double *>(d_stat) + (size_t)c * kFamilies * N * row : nullptr,
                      d_max ? static_cast<double *>(d_max) + (size_t)c * kFamilies * row : nullptr, seed, c, N, padded, P, 0, 0};
        HIP_TRY(hipMemsetAsync(sp.active + N, 0, (1 + kFamilies) * sizeof(uint32_t), stream));
        HIP_TRY(hipMemsetAsync(sp.mmax, 0, kFamilies * row * sizeof(uint64_t), stream));
        if (lds)
            hipLaunchKernelGGL((edgetest_observed_kernel<true>), cohort_grid(cohort, N, kManyBlocks), dim3(kBlock), 0, stream, args);
        else
            hipLaunchKernelGGL((edgetest_observed_kernel<false>), cohort_grid(cohort, N, kGeneralBlocks), dim3(kBlock), 0, stream, args);
        for (uint64_t p0 = 0; p0 < row; p0 += kChunk) {
            args.p0 = (uint32_t)p0, args.np = (uint32_t)std::min<uint64_t>(kChunk, row - p0);
            const dim3 labellings = cohort_grid(cohort, args.np, kManyBlocks);
            if (strata) hipLaunchKernelGGL(edgetest_labellings_kernel<true>, labellings, dim3(kBlock), 0, stream, args);
            else hipLaunchKernelGGL(edgetest_labellings_kernel<false>, labellings, dim3(kBlock), 0, stream, args);
            const uint64_t subs = (args.np + lanes - 1) / lanes;
            const dim3 grid = cohort_grid(cohort, (uint64_t)N * subs, kManyBlocks);
            if (most_groups <= 2)
                chains_launch<2>(lds, grid, lanes, dynamic, stream, args);
            else if (most_groups <= kRegisterGroups)
                chains_launch<kRegisterGroups>(lds, grid, lanes, dynamic, stream, args);
            else
                chains_launch<0>(lds, grid, lanes, dynamic, stream, args);
        }
        const uint64_t finish = d_stat ? (uint64_t)N * kFamilies * row : std::max<uint64_t>((uint64_t)N * kFamilies, d_max ? kFamilies * row : 0);
        hipLaunchKernelGGL(edgetest_finish_kernel, cohort_grid(cohort, (finish + kBlock - 1) / kBlock, kManyBlocks), dim3(kBlock), 0, stream, args);
    }
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

}  // namespace

extern "C" {

int epik_amd_cohort_edgetest_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *labels, uint32_t num_columns,
                                    uint32_t num_permutations, uint64_t seed, void *d_out, void *d_stat, void *d_max, void *stream)
{
    return epik_amd_cohort_edgetest_strata_device(cohort, tree, labels, num_columns, num_permutations, seed, d_out, d_stat, d_max, stream,
                                                  nullptr);
}

int epik_amd_cohort_edgetest_strata_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *labels,
                                           uint32_t num_columns, uint32_t num_permutations, uint64_t seed, void *d_out, void *d_stat,
                                           void *d_max, void *stream, const uint32_t *strata)
{
    return guarded("cohort_edgetest_device", [&]() -> int {
        return edgetest_device_impl(cohort, tree, labels, strata, num_columns, num_permutations, seed, d_out, d_stat, d_max,
                                    static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_edgetest(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *labels, uint32_t num_columns,
                             uint32_t num_permutations, uint64_t seed, epik_amd_edgetest *out, double *stat, double *max)
{
    return epik_amd_cohort_edgetest_strata(cohort, tree, labels, num_columns, num_permutations, seed, out, stat, max, nullptr);
}

int epik_amd_cohort_edgetest_strata(epik_amd_cohort *cohort, const epik_amd_tree *tree, const uint32_t *labels, uint32_t num_columns,
                                    uint32_t num_permutations, uint64_t seed, epik_amd_edgetest *out, double *stat, double *max,
                                    const uint32_t *strata)
{
    return guarded("cohort_edgetest", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(check_columns(num_columns));
        COHORT_TRY(check_present(tree, labels, out));
        COHORT_TRY(check_arguments(labels, cohort->num_samples, num_columns, num_permutations));
        const size_t row = (size_t)num_permutations + 1, N = cohort->num_branches;
        const size_t out_bytes = (size_t)num_columns * N * sizeof(epik_amd_edgetest);
        const size_t stat_bytes = (size_t)num_columns * kFamilies * N * row * sizeof(double);
        const size_t max_bytes = (size_t)num_columns * kFamilies * row * sizeof(double);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult r, s, m;
        COHORT_TRY(r.alloc(out_bytes));
        COHORT_TRY(s.alloc(stat_bytes, stat != nullptr));
        COHORT_TRY(m.alloc(max_bytes, max != nullptr));
        COHORT_TRY(edgetest_device_impl(cohort, tree, labels, strata, num_columns, num_permutations, seed, r.d, s.d, m.d, nullptr));
        COHORT_TRY(r.copy_to(out, out_bytes));
        COHORT_TRY(s.copy_to(stat, stat_bytes));
        return m.copy_to(max, max_bytes);
    });
}

int epik_amd_cohort_edgetest_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                  const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed,
                                  epik_amd_edgetest *out, double *stat, double *max)
{
    return epik_amd_cohort_edgetest_strata_host(mass, num_samples, num_branches, first, labels, num_columns, num_permutations, seed, out,
                                                stat, max, nullptr);
}

int epik_amd_cohort_edgetest_strata_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                         const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed,
                                         epik_amd_edgetest *out, double *stat, double *max, const uint32_t *strata)
{
    return guarded("cohort_edgetest_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(check_present(mass, first, labels, out));
        std::string err;
        return rule_result(edgetest_records(mass, num_samples, num_branches, first, labels, num_columns, num_permutations, seed, out, stat,
                                            max, err, strata),
                           err);
    });
}

}  // extern "C"
