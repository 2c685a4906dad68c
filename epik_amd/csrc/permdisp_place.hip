// permdisp_place.hip -- PERMDISP (Anderson 2006; betadisper + permutest, centroids) of a cohort's samples over their KR
// distances on the device: do the groups of a factor column differ in spread?  epik_amd_cohort_permdisp_device / _permdisp /
// _permdisp_host / _permdisp_kr_host (include/epik_amd.h).
//
// No reference counterpart.  The rule is stated once, in include/epik_amd.h after the edge-test rule (DESIGN.md 3.19;
// epik_amd/host/cohort.cpp: permdisp_records_of_kr is the same rule on the CPU).  Every sum is a sequential chain from +0.0 in
// one lane (__dadd_rn / __dsub_rn / __dmul_rn / __ddiv_rn / __dsqrt_rn; the file is built with -ffp-contract=off as well);
// ranks and counts are integers.  NA is stored as its bit pattern and never computed.  No MFMA: nothing here is a matrix
// product, and a chain may not be split (epca_place.hip gives the longer reason).
//
//   permdisp_columns_kernel     a wave a column: U_c in list order and the groups by first appearance (column_list,
//                               cohort_device.hpp: PERMANOVA's); NA into the column's z and group means.
//   permdisp_distance_kernel    a workgroup a column, a lane a position i: one walk over the positions j of its group, reading
//                               KR[u_j][u_i] (the lanes of a wave read neighbouring cells of a row: the matrix is symmetric, as
//                               permanova_ssw_kernel reads it) and squaring it, feeds both the PERMANOVA row sum t_i (j > i) and
//                               m_i's sum (every j).  Then a lane a group: W_g and c_g; a lane a position: z2, z, clipped; a
//                               lane a group: the mean; a lane a position: r.
//   permdisp_tests_kernel       a wave a (column, slot): the list of the test (the column, or the positions of a pair's two
//                               groups, appended in order by ballots), then one lane the observed sums of z and the centred
//                               residuals, and the record.  A test with something to permute joins its column's list.
//   and, one column after another, the permutations 1 .. P in chunks of kChunk labellings:
//   permdisp_labellings_kernel  a workgroup a (listed test, labelling): the ranks by counting (permutation_rank,
//                               cohort_device.hpp: the edge test's), mu as a byte a position, the labellings of a position side by
//                               side: MU[position][k] -- neighbouring lanes read neighbouring labellings.
//   permdisp_chains_kernel      a workgroup a (listed test, blockDim.x labellings), a lane a labelling: it walks the positions
//                               and adds the residual into the accumulator of mu_i.  kG = 4: the accumulators of G <= 4 groups
//                               in registers (a chain never holds -0.0, so adding +0.0 to the other groups' leaves their bits:
//                               no branch); kG = 0: in LDS, [g][lane].  eta_r into stat; the count of eta_r >= eta2 by a ballot
//                               and one vector atomic add a wave.
//   permdisp_finish_kernel      p of every defined test; eta2 and NA into the stat of the tests that did not permute.
//   permdisp_strata_kernel      with strata only (the strata rule): the tables of every test's list, once a call;
//                               permdisp_labellings_kernel<true> then takes sigma_p (permutation_arrangement) for the rank.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kColumns = EPIK_AMD_PERMDISP_MAX_COLUMNS;
constexpr uint32_t kGroups = EPIK_AMD_PERMDISP_MAX_GROUPS;
constexpr uint32_t kPairSlots = EPIK_AMD_PERMDISP_PAIR_SLOTS;
constexpr uint32_t kMissing = EPIK_AMD_PERMDISP_MISSING;
constexpr uint32_t kRegisterGroups = 4;  // up to here the accumulators of a lane are registers
constexpr uint32_t kChunk = 1024;        // the labellings made at a time
constexpr uint32_t kLdsLanes = 128;      // the lanes of a workgroup whose accumulators are in LDS (32 KiB at G = 32)
constexpr uint64_t kManyBlocks = 65536;

static_assert(sizeof(epik_amd_permdisp) == 48, "the record is 48 bytes");
static_assert(kPairSlots == kGroups * (kGroups - 1) / 2 && kBlock == 256 && kWave == 64 && kGroups <= kWave);
static_assert(kChunk % kBlock == 0 && kChunk % kLdsLanes == 0 && (kGroups & (kGroups - 1)) == 0);

struct DispColumn {
    uint32_t used, groups;
    uint32_t size[kGroups];
};

enum : uint32_t { kUndefined = 0, kTied = 1, kPermuted = 2 };  // a test: NA; sxx_r is not > 0.0; its labellings run

struct DispTest {
    uint64_t offset;   // of its list in the pools
    uint32_t n, groups, state, pad;
    uint32_t size[2];  // of a pair's two groups (the whole column's are in its DispColumn)
    double eta2, sxx_r;
};

struct DispSpace {
    double *t, *m, *z, *r;  // [M][Sp] by position: PERMANOVA's row sums, m, z and the residuals
    double *dr;             // [M][lists * Sp]: the centred residuals of a test's positions
    uint32_t *lab;          // [M][Sp]: the labels by sample
    uint32_t *idx;          // [M][Sp]: the samples of the positions
    uint32_t *pos;          // [M][lists * Sp]: the column's positions of a test's; a column's pairs follow its whole list
    uint32_t *active;       // [M][slots]: the slots to permute
    uint32_t *count;        // [M]: how many
    DispColumn *cols;       // [M]
    DispTest *tests;        // [M][slots]
    uint8_t *lam, *clip;    // [M][Sp]: the groups of the positions, and whether z2 < 0
    uint8_t *two;           // as pos: the groups of a test's positions
    uint8_t *MU;            // [lists * Sp][kChunk]: the chunk of labellings of the column at hand
    uint32_t *strata;       // with strata only: [Sp], the strata by sample
    uint32_t *hs, *home;    // ... and as pos: the strata of a test's positions, and its positions by (stratum, position)
};

size_t permdisp_space(void *base, uint32_t padded, uint32_t M, bool pairwise, bool strata, DispSpace *sp)
{
    const size_t slots = 1 + (pairwise ? kPairSlots : 0), lists = pairwise ? kGroups : 1;
    const size_t column = (size_t)M * padded, pool = (size_t)M * lists * padded;
    Carver c(base);
    const DispSpace parts{.t = c.take<double>(column),
                          .m = c.take<double>(column),
                          .z = c.take<double>(column),
                          .r = c.take<double>(column),
                          .dr = c.take<double>(pool),
                          .lab = c.take<uint32_t>(column),
                          .idx = c.take<uint32_t>(column),
                          .pos = c.take<uint32_t>(pool),
                          .active = c.take<uint32_t>(M * slots),
                          .count = c.take<uint32_t>(M),
                          .cols = c.take<DispColumn>(M),
                          .tests = c.take<DispTest>(M * slots),
                          .lam = c.take<uint8_t>(column),
                          .clip = c.take<uint8_t>(column),
                          .two = c.take<uint8_t>(pool),
                          .MU = c.take<uint8_t>(lists * padded * kChunk),
                          .strata = c.take<uint32_t>(strata ? padded : 0),
                          .hs = c.take<uint32_t>(strata ? pool : 0),
                          .home = c.take<uint32_t>(strata ? pool : 0)};
    if (sp) *sp = parts;
    return c.bytes();
}

struct DispArgs {
    const double *kr;
    DispSpace sp;
    epik_amd_permdisp *out;       // [M][slots]
    double *stat;                 // [M][slots][P + 1], or null
    double *group_mean, *z;       // [M][32], [M][S]
    uint64_t seed;
    uint32_t num_samples, padded, num_columns, slots, lists, num_permutations;
    uint32_t column, p0, np;      // the column at hand and its chunk: the labellings p0 .. p0 + np - 1 (p0 >= 1)
};

__global__ __launch_bounds__(kWave) void permdisp_columns_kernel(const uint64_t *__restrict__ total, const DispArgs a)
{
    __shared__ uint32_t group_of[kGroups], size[kGroups];
    const uint32_t S = a.num_samples;
    for (uint32_t c = blockIdx.x; c < a.num_columns; c += gridDim.x) {
        for (uint32_t s = threadIdx.x; s < S; s += kWave) a.z[(uint64_t)c * S + s] = na_value();
        if (threadIdx.x < kGroups) a.group_mean[(uint64_t)c * kGroups + threadIdx.x] = na_value();
        const uint64_t offset = (uint64_t)c * a.padded;
        uint32_t L, G;  // (uniform)
        column_list<kGroups>(total, a.sp.lab + offset, S, kMissing, group_of, size, a.sp.idx + offset, a.sp.lam + offset, L, G);
        for (uint32_t g = threadIdx.x; g < kGroups; g += kWave) a.sp.cols[c].size[g] = size[g];
        if (threadIdx.x == 0) a.sp.cols[c].used = L, a.sp.cols[c].groups = G, a.sp.count[c] = 0;
        __syncthreads();  // (the tables are written again)
    }
}

__global__ __launch_bounds__(kBlock) void permdisp_distance_kernel(const DispArgs a)
{
    __shared__ double centre_of[kGroups], mean_of[kGroups];
    const uint32_t tid = threadIdx.x;
    const uint64_t S = a.num_samples;
    for (uint32_t c = blockIdx.x; c < a.num_columns; c += gridDim.x) {
        const DispColumn *col = a.sp.cols + c;
        const uint32_t L = col->used, G = col->groups;  // (uniform)
        const uint64_t at = (uint64_t)c * a.padded;
        const uint32_t *idx = a.sp.idx + at;
        const uint8_t *lam = a.sp.lam + at;
        double *t = a.sp.t + at, *m = a.sp.m + at, *z = a.sp.z + at, *r = a.sp.r + at;
        uint8_t *clip = a.sp.clip + at;
        for (uint32_t i = tid; i < L; i += kBlock) {
            const uint32_t g = lam[i];
            const double *column = a.kr + idx[i];  // (idx < S: KR[u_j][u_i] is inside the matrix)
            double above = 0.0, all = 0.0;
#pragma unroll 4
            for (uint32_t j = 0; j < L; ++j) {
                if (lam[j] != g) continue;
                const double d = column[(uint64_t)idx[j] * S];
                const double sq = __dmul_rn(d, d);
                all = __dadd_rn(all, sq);
                if (j > i) above = __dadd_rn(above, sq);
            }
            t[i] = above;
            m[i] = __ddiv_rn(all, (double)col->size[g]);
        }
        __syncthreads();
        if (tid < G) {
            double w = 0.0;
            for (uint32_t i = 0; i < L; ++i)
                if (lam[i] == tid) w = __dadd_rn(w, t[i]);
            const double n = (double)col->size[tid];
            centre_of[tid] = __ddiv_rn(__ddiv_rn(w, n), n);
        }
        __syncthreads();
        for (uint32_t i = tid; i < L; i += kBlock) {
            const double z2 = __dsub_rn(m[i], centre_of[lam[i]]);
            const double zi = z2 > 0.0 ? __dsqrt_rn(z2) : 0.0;
            clip[i] = z2 < 0.0;
            z[i] = zi;
            a.z[(uint64_t)c * S + idx[i]] = zi;
        }
        __syncthreads();
        if (tid < G) {
            double acc = 0.0;
            for (uint32_t i = 0; i < L; ++i)
                if (lam[i] == tid) acc = __dadd_rn(acc, z[i]);
            const double mean = __ddiv_rn(acc, (double)col->size[tid]);
            mean_of[tid] = mean;
            a.group_mean[(uint64_t)c * kGroups + tid] = mean;
        }
        __syncthreads();
        for (uint32_t i = tid; i < L; i += kBlock) r[i] = __dsub_rn(z[i], mean_of[lam[i]]);
        __syncthreads();  // (the tables are written again)
    }
}

__global__ __launch_bounds__(kWave) void permdisp_tests_kernel(const DispArgs a)
{
    __shared__ double sums[kGroups];
    const uint32_t slots = a.slots, padded = a.padded, P = a.num_permutations;
    for (uint32_t unit = blockIdx.x; unit < a.num_columns * slots; unit += gridDim.x) {
        const uint32_t c = unit / slots, slot = unit % slots;
        const DispColumn *col = a.sp.cols + c;
        const uint32_t L = col->used, G = col->groups;
        const uint64_t column_at = (uint64_t)c * padded, pool_at = (uint64_t)c * a.lists * padded;
        const uint8_t *lam = a.sp.lam + column_at;
        uint64_t offset = pool_at;
        uint32_t n = 0, groups = 0, size0 = 0, size1 = 0;  // (uniform)
        if (slot == 0) {
            for (uint32_t i = threadIdx.x; i < L; i += kWave) a.sp.pos[offset + i] = i, a.sp.two[offset + i] = lam[i];
            n = L, groups = G;
        } else {
            const uint32_t pair = slot - 1;
            uint32_t h = 1;
            while ((h + 1) * h / 2 <= pair) ++h;
            const uint32_t g = pair - h * (h - 1) / 2;
            if (h < G) {
                // the pairs' lists follow the whole column's, in slot order
                offset += padded;
                for (uint32_t hh = 1; hh <= h; ++hh)
                    for (uint32_t gg = 0; gg < (hh < h ? hh : g); ++gg) offset += col->size[gg] + col->size[hh];
                for (uint32_t base = 0; base < L; base += kWave) {
                    const uint32_t i = base + threadIdx.x;
                    const uint32_t group = i < L ? lam[i] : kMissing;
                    n += append_in_order(group == g || group == h, n, i, group == h, a.sp.pos + offset, a.sp.two + offset);
                }
                groups = 2, size0 = col->size[g], size1 = col->size[h];
            }
        }
        __syncthreads();  // (the list is written: one lane reads all of it)
        if (threadIdx.x == 0) {
            const uint32_t *pos = a.sp.pos + offset;
            const uint8_t *two = a.sp.two + offset;
            const double *z = a.sp.z + column_at, *r = a.sp.r + column_at;
            double *dr = a.sp.dr + offset;
            epik_amd_permdisp rec{n, groups, 0, 0, 0, na_value(), na_value(), na_value()};
            DispTest test{offset, n, groups, kUndefined, 0, {size0, size1}, 0.0, 0.0};
            for (uint32_t i = 0; i < n; ++i) rec.clipped += a.sp.clip[column_at + pos[i]];
            if (groups >= 2 && n >= groups + 1) {
                double acc = 0.0;
                for (uint32_t i = 0; i < n; ++i) acc = __dadd_rn(acc, z[pos[i]]);
                const double mx = __ddiv_rn(acc, (double)n);
                for (uint32_t g = 0; g < groups; ++g) sums[g] = 0.0;
                double sxx = 0.0;
                for (uint32_t i = 0; i < n; ++i) {
                    const double d = __dsub_rn(z[pos[i]], mx);
                    sxx = __dadd_rn(sxx, __dmul_rn(d, d));
                    sums[two[i]] = __dadd_rn(sums[two[i]], d);
                }
                if (sxx > 0.0) {
                    double among = 0.0;
                    for (uint32_t g = 0; g < groups; ++g) {
                        const uint32_t size = slot == 0 ? col->size[g] : g ? size1 : size0;
                        among = __dadd_rn(among, __ddiv_rn(__dmul_rn(sums[g], sums[g]), (double)size));
                    }
                    rec.eta2 = __ddiv_rn(among, sxx);
                    const double ssw = __dsub_rn(sxx, among);
                    if (ssw > 0.0) rec.f = __ddiv_rn(__ddiv_rn(among, (double)(groups - 1)), __ddiv_rn(ssw, (double)(n - groups)));
                    acc = 0.0;
                    for (uint32_t i = 0; i < n; ++i) acc = __dadd_rn(acc, r[pos[i]]);
                    const double mr = __ddiv_rn(acc, (double)n);
                    double sxx_r = 0.0;
                    for (uint32_t i = 0; i < n; ++i) {
                        const double d = __dsub_rn(r[pos[i]], mr);
                        dr[i] = d;
                        sxx_r = __dadd_rn(sxx_r, __dmul_rn(d, d));
                    }
                    test.eta2 = rec.eta2, test.sxx_r = sxx_r;
                    test.state = sxx_r > 0.0 ? kPermuted : kTied;
                    if (test.state == kTied) rec.at_least = P;  // nothing to permute: every permuted statistic is a tie
                    if (test.state == kPermuted) a.sp.active[(uint64_t)c * slots + atomicAdd(a.sp.count + c, 1u)] = slot;
                }
            }
            a.out[unit] = rec;
            a.sp.tests[unit] = test;
        }
        __syncthreads();  // (the sums are written again)
    }
}

// the strata rule's tables of every test with a list: a workgroup a (column, slot)
__global__ __launch_bounds__(kBlock) void permdisp_strata_kernel(const DispArgs a)
{
    for (uint32_t unit = blockIdx.x; unit < a.num_columns * a.slots; unit += gridDim.x) {  // (uniform)
        const DispTest *test = a.sp.tests + unit;
        const uint32_t *idx = a.sp.idx + (uint64_t)(unit / a.slots) * a.padded, *pos = a.sp.pos + test->offset;
        strata_tables(a.sp.strata, [&](uint32_t i) { return idx[pos[i]]; }, test->n, a.sp.hs + test->offset, a.sp.home + test->offset);
    }
}

template <bool kStrata>
__global__ __launch_bounds__(kBlock) void permdisp_labellings_kernel(const DispArgs a)
{
    __shared__ uint64_t tile[kCohortKeyTile];
    const uint32_t c = a.column, slots = a.slots;
    const uint64_t pool_at = (uint64_t)c * a.lists * a.padded, units = (uint64_t)a.sp.count[c] * a.np;
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {  // (uniform)
        const uint32_t slot = a.sp.active[(uint64_t)c * slots + unit / a.np], k = (uint32_t)(unit % a.np);
        const DispTest *test = a.sp.tests + (uint64_t)c * slots + slot;
        const uint32_t n = test->n;
        const uint8_t *two = a.sp.two + test->offset;
        uint8_t *mu = a.sp.MU + (test->offset - pool_at) * kChunk + k;  // (offset - pool_at + i < lists * Sp)
        for (uint32_t base = 0; base < n; base += kBlock) {
            const uint32_t i = base + threadIdx.x;
            uint32_t rank;
            if constexpr (kStrata) {
                __shared__ uint32_t htile[kCohortKeyTile];
                rank = permutation_arrangement(a.seed, a.p0 + k, i, n, tile, htile, a.sp.hs + test->offset, a.sp.home + test->offset);
            } else {
                rank = permutation_rank(a.seed, a.p0 + k, i, n, tile);
            }
            if (i < n) mu[(uint64_t)i * kChunk] = two[rank];  // (rank < n)
        }
    }
}

template <uint32_t kG>
__global__ __launch_bounds__(kBlock) void permdisp_chains_kernel(const DispArgs a)
{
    extern __shared__ __align__(16) unsigned char dynamic_lds[];
    const uint32_t tid = threadIdx.x, lanes = blockDim.x, c = a.column, slots = a.slots, P = a.num_permutations;
    double *acc = reinterpret_cast<double *>(dynamic_lds) + tid;  // kG == 0: [G][lanes]
    const uint64_t pool_at = (uint64_t)c * a.lists * a.padded;
    const uint32_t subs = (a.np + lanes - 1) / lanes;
    const uint64_t units = (uint64_t)a.sp.count[c] * subs;
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {  // (uniform)
        const uint32_t slot = a.sp.active[(uint64_t)c * slots + unit / subs], k = (uint32_t)(unit % subs) * lanes + tid;
        const uint64_t at = (uint64_t)c * slots + slot;
        const DispTest test = a.sp.tests[at];
        const uint32_t n = test.n, G = test.groups;
        const bool live = k < a.np;
        const uint8_t *mu = a.sp.MU + (test.offset - pool_at) * kChunk + (live ? k : 0);
        const double *d = a.sp.dr + test.offset;
        double reg[kG ? kG : 1];
        if (kG) {
#pragma unroll
            for (uint32_t g = 0; g < kG; ++g) reg[g] = 0.0;
        } else {
            for (uint32_t g = 0; g < G; ++g) acc[g * lanes] = 0.0;
        }
#pragma unroll 4
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t m = mu[(uint64_t)i * kChunk];
            const double v = d[i];  // a broadcast
            if (kG) {
#pragma unroll
                for (uint32_t g = 0; g < kG; ++g) reg[g] = __dadd_rn(reg[g], m == g ? v : 0.0);  // (+0.0: the same bits)
            } else {
                acc[m * lanes] = __dadd_rn(acc[m * lanes], v);
            }
        }
        double among = 0.0;
        for (uint32_t g = 0; g < G; ++g) {
            const uint32_t size = slot == 0 ? a.sp.cols[c].size[g] : test.size[g ? 1 : 0];
            double s = 0.0;
            if (kG) {
#pragma unroll
                for (uint32_t q = 0; q < kG; ++q)
                    if (q == g) s = reg[q];
            } else {
                s = acc[g * lanes];
            }
            among = __dadd_rn(among, __ddiv_rn(__dmul_rn(s, s), (double)size));
        }
        const double eta = __ddiv_rn(among, test.sxx_r);
        if (live && a.stat) a.stat[at * ((uint64_t)P + 1) + a.p0 + k] = eta;
        const unsigned long long count = __popcll(__ballot(live && eta >= test.eta2));
        if (tid % kWave == 0 && count) atomicAdd(reinterpret_cast<unsigned long long *>(&a.out[at].at_least), count);
    }
}

__global__ __launch_bounds__(kBlock) void permdisp_finish_kernel(const DispArgs a)
{
    const uint64_t tests = (uint64_t)a.num_columns * a.slots, row = (uint64_t)a.num_permutations + 1;
    const uint64_t first = (uint64_t)blockIdx.x * kBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t test = first; test < tests; test += stride)
        if (a.sp.tests[test].state != kUndefined)
            a.out[test].p = __ddiv_rn((double)(1 + a.out[test].at_least), (double)row);
    if (!a.stat) return;
    for (uint64_t e = first; e < tests * row; e += stride) {
        const DispTest *test = a.sp.tests + e / row;
        if (test->state == kUndefined)
            a.stat[e] = na_value();
        else if (test->state == kTied || e % row == 0)
            a.stat[e] = test->eta2;
    }
}

int check_arguments(const uint32_t *labels, uint32_t S, uint32_t M, uint32_t P)
{
    std::string err;
    return rule_result(permdisp_arguments_valid(labels, S, M, P, err), err);
}

int permdisp_device_impl(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *labels, const uint32_t *strata, uint32_t M,
                         uint32_t P, uint64_t seed, bool pairwise, void *d_out, void *d_stat, void *d_group_mean, void *d_z,
                         hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(check_columns(M));
    COHORT_TRY(check_present(d_kr, labels, d_out, d_group_mean, d_z));
    const uint32_t S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    COHORT_TRY(check_arguments(labels, S, M, P));
    COHORT_TRY(check_has_distances(cohort));
    // the distinct labels of a column bound its G: the largest decides where the accumulators are, and each bounds the tests
    // of its column that can have something to permute (the grids of its launches; none below two labels)
    std::vector<uint32_t> most_tests;
    const uint32_t most_groups = most_distinct_labels(labels, S, M, kMissing, &most_tests);
    for (uint32_t &n : most_tests) n = n >= 2 ? 1 + (pairwise ? n * (n - 1) / 2 : 0) : 0;
    HIP_TRY(hipSetDevice(cohort->device));
    HIP_TRY(hipDeviceSynchronize());  // (the distances enqueued on whatever stream, and an earlier call that reads the workspace)
    COHORT_TRY(cohort_space_ensure(cohort, kSpacePermdisp, permdisp_space(nullptr, padded, M, pairwise, strata != nullptr, nullptr)));
    DispArgs args{};
    permdisp_space(cohort->space[kSpacePermdisp].d, padded, M, pairwise, strata != nullptr, &args.sp);
    COHORT_TRY(upload_labels_by_column(labels, S, M, padded, kMissing, args.sp.lab));
    if (strata) COHORT_TRY(upload_strata(strata, S, padded, args.sp.strata));
    const uint32_t slots = 1 + (pairwise ? kPairSlots : 0), lists = pairwise ? kGroups : 1;
    args.kr = static_cast<const double *>(d_kr), args.out = static_cast<epik_amd_permdisp *>(d_out);
    args.stat = static_cast<double *>(d_stat), args.group_mean = static_cast<double *>(d_group_mean), args.z = static_cast<double *>(d_z);
    args.seed = seed, args.num_samples = S, args.padded = padded, args.num_columns = M, args.slots = slots, args.lists = lists;
    args.num_permutations = P;
    const uint64_t tests = (uint64_t)M * slots;
    hipLaunchKernelGGL(permdisp_columns_kernel, cohort_grid(cohort, M, kColumns), dim3(kWave), 0, stream, cohort->d_total, args);
    hipLaunchKernelGGL(permdisp_distance_kernel, cohort_grid(cohort, M, kColumns), dim3(kBlock), 0, stream, args);
    hipLaunchKernelGGL(permdisp_tests_kernel, cohort_grid(cohort, tests, kManyBlocks), dim3(kWave), 0, stream, args);
    if (strata) hipLaunchKernelGGL(permdisp_strata_kernel, cohort_grid(cohort, tests, kManyBlocks), dim3(kBlock), 0, stream, args);
    const bool registers = most_groups <= kRegisterGroups;
    const uint32_t lanes = registers ? kBlock : kLdsLanes;
    const size_t dynamic = registers ? 0 : (size_t)kGroups * lanes * sizeof(double);
    // Two launches a (column, chunk): 2 M ceil(P / 1 024) in all, about 125 000 at M = 64 and P = 999 999 -- a column's
    // labellings live in one MU pool, so the columns are not batched.  A column that cannot have a defined test launches nothing.
    for (uint32_t c = 0; c < M; ++c) {
        if (!most_tests[c]) continue;
        for (uint32_t p0 = 1; p0 <= P; p0 += kChunk) {
            args.column = c, args.p0 = p0, args.np = std::min<uint32_t>(kChunk, P + 1 - p0);
            const uint64_t subs = (args.np + lanes - 1) / lanes, listed = most_tests[c];
            const dim3 labellings = cohort_grid(cohort, listed * args.np, kManyBlocks);
            if (strata) hipLaunchKernelGGL(permdisp_labellings_kernel<true>, labellings, dim3(kBlock), 0, stream, args);
            else hipLaunchKernelGGL(permdisp_labellings_kernel<false>, labellings, dim3(kBlock), 0, stream, args);
            if (registers)
                hipLaunchKernelGGL(permdisp_chains_kernel<kRegisterGroups>, cohort_grid(cohort, listed * subs, kManyBlocks), dim3(lanes), 0,
                                   stream, args);
            else
                hipLaunchKernelGGL(permdisp_chains_kernel<0>, cohort_grid(cohort, listed * subs, kManyBlocks), dim3(lanes), dynamic, stream,
                                   args);
        }
    }
    const uint64_t finish = d_stat ? tests * ((uint64_t)P + 1) : tests;
    hipLaunchKernelGGL(permdisp_finish_kernel, cohort_grid(cohort, (finish + kBlock - 1) / kBlock, kManyBlocks), dim3(kBlock), 0, stream, args);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

}  // namespace

extern "C" {

int epik_amd_cohort_permdisp_device(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *labels, uint32_t num_columns,
                                    uint32_t num_permutations, uint64_t seed, int pairwise, void *d_out, void *d_stat,
                                    void *d_group_mean, void *d_z, void *stream)
{
    return epik_amd_cohort_permdisp_strata_device(cohort, d_kr, labels, num_columns, num_permutations, seed, pairwise, d_out, d_stat,
                                                  d_group_mean, d_z, stream, nullptr);
}

int epik_amd_cohort_permdisp_strata_device(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *labels, uint32_t num_columns,
                                           uint32_t num_permutations, uint64_t seed, int pairwise, void *d_out, void *d_stat,
                                           void *d_group_mean, void *d_z, void *stream, const uint32_t *strata)
{
    return guarded("cohort_permdisp_device", [&]() -> int {
        return permdisp_device_impl(cohort, d_kr, labels, strata, num_columns, num_permutations, seed, pairwise != 0, d_out, d_stat,
                                    d_group_mean, d_z, static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_permdisp(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, const uint32_t *labels,
                             uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise, epik_amd_permdisp *out,
                             double *stat, double *group_mean, double *z)
{
    return epik_amd_cohort_permdisp_metric(cohort, tree, branch_length, EPIK_AMD_DISTANCE_KR, labels, num_columns, num_permutations, seed,
                                           pairwise, out, stat, group_mean, z);
}

int epik_amd_cohort_permdisp_metric(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                                    const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise,
                                    epik_amd_permdisp *out, double *stat, double *group_mean, double *z)
{
    return epik_amd_cohort_permdisp_strata(cohort, tree, branch_length, metric, labels, num_columns, num_permutations, seed, pairwise, out,
                                           stat, group_mean, z, nullptr);
}

int epik_amd_cohort_permdisp_strata(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                                    const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise,
                                    epik_amd_permdisp *out, double *stat, double *group_mean, double *z, const uint32_t *strata)
{
    return guarded("cohort_permdisp", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(check_columns(num_columns));
        COHORT_TRY(check_present(labels, out, group_mean, z));
        const uint32_t S = cohort->num_samples;
        COHORT_TRY(check_arguments(labels, S, num_columns, num_permutations));
        const size_t tests = (size_t)num_columns * (1 + (pairwise ? kPairSlots : 0));
        const size_t out_bytes = tests * sizeof(epik_amd_permdisp), stat_bytes = tests * ((size_t)num_permutations + 1) * sizeof(double);
        const size_t mean_bytes = (size_t)num_columns * kGroups * sizeof(double), z_bytes = (size_t)num_columns * S * sizeof(double);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult kr, r, s, g, zz;
        COHORT_TRY(kr.alloc((size_t)S * S * sizeof(double)));
        COHORT_TRY(r.alloc(out_bytes));
        COHORT_TRY(s.alloc(stat_bytes, stat != nullptr));
        COHORT_TRY(g.alloc(mean_bytes));
        COHORT_TRY(zz.alloc(z_bytes));
        COHORT_TRY(cohort_distance_enqueue(cohort, tree, branch_length, metric, kr.d, nullptr));
        COHORT_TRY(permdisp_device_impl(cohort, kr.d, labels, strata, num_columns, num_permutations, seed, pairwise != 0, r.d, s.d, g.d,
                                        zz.d, nullptr));
        COHORT_TRY(r.copy_to(out, out_bytes));
        COHORT_TRY(s.copy_to(stat, stat_bytes));
        COHORT_TRY(g.copy_to(group_mean, mean_bytes));
        return zz.copy_to(z, z_bytes);
    });
}

int epik_amd_cohort_permdisp_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                  const double *branch_length, const uint32_t *labels, uint32_t num_columns,
                                  uint32_t num_permutations, uint64_t seed, int pairwise, epik_amd_permdisp *out, double *stat,
                                  double *group_mean, double *z)
{
    return epik_amd_cohort_permdisp_metric_host(mass, num_samples, num_branches, first, branch_length, EPIK_AMD_DISTANCE_KR, labels,
                                                num_columns, num_permutations, seed, pairwise, out, stat, group_mean, z);
}

int epik_amd_cohort_permdisp_metric_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                         const double *branch_length, uint32_t metric, const uint32_t *labels, uint32_t num_columns,
                                         uint32_t num_permutations, uint64_t seed, int pairwise, epik_amd_permdisp *out, double *stat,
                                         double *group_mean, double *z)
{
    return epik_amd_cohort_permdisp_strata_host(mass, num_samples, num_branches, first, branch_length, metric, labels, num_columns,
                                                num_permutations, seed, pairwise, out, stat, group_mean, z, nullptr);
}

int epik_amd_cohort_permdisp_strata_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                         const double *branch_length, uint32_t metric, const uint32_t *labels, uint32_t num_columns,
                                         uint32_t num_permutations, uint64_t seed, int pairwise, epik_amd_permdisp *out, double *stat,
                                         double *group_mean, double *z, const uint32_t *strata)
{
    return guarded("cohort_permdisp_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(check_present(mass, first, branch_length, labels, out, group_mean, z));
        std::string err;
        return rule_result(permdisp_records(mass, num_samples, num_branches, first, branch_length, labels, num_columns, num_permutations,
                                            seed, pairwise != 0, out, stat, group_mean, z, err, metric, strata),
                           err);
    });
}

int epik_amd_cohort_permdisp_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const uint32_t *labels,
                                     uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise,
                                     epik_amd_permdisp *out, double *stat, double *group_mean, double *z)
{
    return epik_amd_cohort_permdisp_strata_kr_host(kr, totals, num_samples, labels, num_columns, num_permutations, seed, pairwise, out,
                                                   stat, group_mean, z, nullptr);
}

int epik_amd_cohort_permdisp_strata_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const uint32_t *labels,
                                            uint32_t num_columns, uint32_t num_permutations, uint64_t seed, int pairwise,
                                            epik_amd_permdisp *out, double *stat, double *group_mean, double *z, const uint32_t *strata)
{
    return guarded("cohort_permdisp_kr_host", [&]() -> int {
        COHORT_TRY(check_host_samples(num_samples));
        COHORT_TRY(check_present(kr, totals, labels, out, group_mean, z));
        std::string err;
        return rule_result(permdisp_records_of_kr(kr, totals, num_samples, labels, num_columns, num_permutations, seed, pairwise != 0, out,
                                                  stat, group_mean, z, err, strata),
                           err);
    });
}

}  // extern "C"
