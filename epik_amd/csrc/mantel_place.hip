// mantel_place.hip -- the Mantel and partial Mantel tests and ANOSIM of a cohort's samples over their distances on the device:
// does the distance grow with a variable or with another distance, a third held fixed; are the ranked distances between groups
// larger than within?  epik_amd_cohort_mantel_device / _mantel / _mantel_host / _mantel_kr_host and the same four of anosim
// (include/epik_amd.h).
//
// No reference counterpart.  The rule is stated once, in include/epik_amd.h behind the strata rule (DESIGN.md 3.27;
// epik_amd/host/cohort.cpp: mantel_records_of_kr and anosim_records_of_kr are the same rule on the CPU).  Every sum over the
// pairs is the rule's triangle chain: a row's chain in one lane, then the chain of the rows in one lane (__dadd_rn / __dmul_rn /
// __ddiv_rn / __dsqrt_rn; the file is built with -ffp-contract=off as well).  A rank is a count or the slot of a sort, exact
// either way; ANOSIM's sums are integers.  NA is stored as its bit pattern and never computed.
//
// The host loops over the tests and enqueues, never synchronising: the workspace holds one test's tables and every test's
// record.  A test's list is known on the device only, so every grid is sized by S and reads n.
//
//   mantel_list_kernel      a wave: the list of a (side, control) in ascending s by ballots; the record's NA.
//   anosim_list_kernel      a wave: column_list, m_W, whether the column is defined; the record's NA.
//   mantel_strata_kernel    with strata: the strata rule's tables of the list.
//   mantel_triangle_kernel  x, y and z over the list as symmetric tables [n][n]; a column is expanded on the fly.
//   rank_fill_kernel, sort_tile_kernel, sort_global_kernel, rank_write_kernel
//                           the midranks of a table's m values (spearman, ANOSIM): the pairs and a padding of +inf up to a power
//                           of two, sorted by a bitonic network -- tiles of kSortTile values in LDS, the strides from a tile
//                           upwards in global memory -- then midrank_sorted per cell, written back over the table.
//   mantel_rowsum_kernel, mantel_mean_kernel, mantel_centre_kernel, mantel_rowprod_kernel, mantel_observed_kernel
//                           the means, the deviations in the tables' place, ss and the observed s_xy, s_xz, s_yz by triangle
//                           chains (a lane a row, reading down the symmetric table's column: a coalesced line), the record.
//   mantel_cross_kernel     a workgroup a chunk of kPerms permutations.  The four arrangements side by side as the four uint16 of a
//                           word per position, so that one read of sigma(j) and one of y'[j][i] serve four chains.  A wave takes
//                           64 rows i and the mirrored 64 (the triangle is level) and walks j together: y'[j][i] is read down a
//                           column, a coalesced line; x' is gathered as x'[sigma(j)][sigma(i)], within one row a step; with a
//                           control z'[j][i] rides on the same gather.  Then a lane a chain over the rows, the statistic, and
//                           one vector atomic a chunk for at_least.  The keys are ranked by counting up to kCountPositions
//                           positions and by a bitonic sort of (key, position) beyond; the vectors of a call of up to
//                           kLdsPositions samples (kLdsControlPositions with a control) stay in LDS, beyond (or with
//                           EPIK_AMD_MANTEL_LDS=0) in the workgroup's slice of global memory, ranked by counting: the same code
//                           on other pointers.  kStrata: the arrangements of the strata rule.  kAnosim: the labellings
//                           lambda(sigma(i)) as the bytes of a word and the sum of twice the midranks within groups, integers;
//                           launched for p = 0 (R_0 and the record's means), then for 1 .. P.
//   mantel_finish_kernel    p = (1 + at_least) / (P + 1), and NA into the stat of the tests that did not run.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kGroups = EPIK_AMD_PERMANOVA_MAX_GROUPS;
constexpr uint32_t kMissing = EPIK_AMD_PERMANOVA_MISSING;
constexpr uint32_t kNone = EPIK_AMD_MANTEL_NO_CONTROL;
constexpr uint32_t kPerms = 4;                 // the arrangements a workgroup carries through one pass: the uint16 of a word
constexpr uint32_t kLdsPositions = 1024;       // the most samples of a call whose vectors stay in LDS (52 KiB with strata)
constexpr uint32_t kLdsControlPositions = 512; // ... with a control: twice the row sums
constexpr uint32_t kCountPositions = 256;      // up to here the LDS path ranks the keys by counting; beyond, it sorts
constexpr uint32_t kSmallSamples = 128;        // up to here a workgroup is one wave
constexpr uint32_t kGeneralBlocks = 256;       // workgroups of the general path: each has a slice
constexpr uint32_t kSortTile = 4096;           // the values of the triangle sort that a workgroup sorts in LDS (32 KiB)
constexpr uint32_t kTables = 3, kProducts = 6; // x, y, z; xx, yy, xy, zz, xz, yz
constexpr uint64_t kManyBlocks = 65536;

static_assert(sizeof(epik_amd_mantel) == 64, "the record is 64 bytes");
static_assert(sizeof(epik_amd_anosim) == 48, "the record is 48 bytes");
static_assert(kPerms == 4 && kBlock == 256 && kWave == 64 && EPIK_AMD_MANTEL_MAX_SAMPLES <= 65536, "a position is a uint16");
static_assert(kCountPositions <= kLdsControlPositions && (kLdsPositions & (kLdsPositions - 1)) == 0 &&
              (kSortTile & (kSortTile - 1)) == 0 && kSortTile >= 2 * kBlock);

struct MantelTest {
    uint32_t n, run, defined, pad;  // run: the tables are made; defined: the permutations run
    uint64_t m, m_within;           // (m_within: ANOSIM)
    double mean[kTables];
    double den_xy, den_xz, r_yz, stat0;
};

struct MantelSpace {
    double *tab[kTables];  // [S][S] each: x, y, z over the list, [n][n]
    double *sorted;        // [P2]
    double *rows;          // [kProducts][Sp]: the rows' chains
    double *scratch;       // [kGeneralBlocks] slices
    double *values;        // [Mv][S]
    double *matrices;      // [Mm][S][S]
    uint8_t *present;      // [Mm][S]
    uint32_t *lab;         // [M][Sp] (ANOSIM)
    uint32_t *idx;         // [Sp]: the samples of the positions
    uint8_t *lam;          // [Sp]: their groups (ANOSIM)
    uint32_t *strata, *hs, *home;  // [Sp] each, with strata
    MantelTest *tests;     // [tests]
};

constexpr size_t kSliceBytes = 2 * kPerms * 8 + 8 + 4;  // the bytes of a slice per padded sample: t | sigma | mu

// the power of two that the triangle of S samples is padded to
uint32_t sort_size(uint32_t S)
{
    const uint64_t m = (uint64_t)S * (S ? S - 1 : 0) / 2;
    uint32_t P2 = 2;
    while (P2 < m) P2 <<= 1;  // (m < 2^25 + 1: S <= 8 192)
    return P2;
}

size_t mantel_space(void *base, uint32_t S, uint32_t padded, uint32_t Mv, uint32_t Mm, uint32_t M, uint32_t tables, bool ranks,
                    bool strata, uint32_t tests, MantelSpace *sp)
{
    Carver c(base);
    const size_t cells = (size_t)S * S;
    MantelSpace parts{};
    for (uint32_t k = 0; k < kTables; ++k) parts.tab[k] = c.take<double>(k < tables ? cells : 0);
    parts.sorted = c.take<double>(ranks ? sort_size(S) : 0);
    parts.rows = c.take<double>((size_t)kProducts * padded);
    parts.scratch = c.take<double>((size_t)kGeneralBlocks * kSliceBytes * padded / sizeof(double));
    parts.values = c.take<double>((size_t)Mv * S);
    parts.matrices = c.take<double>((size_t)Mm * cells);
    parts.present = c.take<uint8_t>((size_t)Mm * S);
    parts.lab = c.take<uint32_t>((size_t)M * padded);
    parts.idx = c.take<uint32_t>(padded);
    parts.lam = c.take<uint8_t>(padded);
    parts.strata = c.take<uint32_t>(strata ? padded : 0);
    parts.hs = c.take<uint32_t>(strata ? padded : 0);
    parts.home = c.take<uint32_t>(strata ? padded : 0);
    parts.tests = c.take<MantelTest>(tests);
    if (sp) *sp = parts;
    return c.bytes();
}

// ---- the lists ---------------------------------------------------------------------------------------------------------------
__device__ inline bool side_present(const double *__restrict__ values, const uint8_t *__restrict__ present, uint32_t S, uint32_t Mv,
                                    uint32_t q, uint32_t s)
{
    if (q < Mv) {
        const double v = values[(uint64_t)q * S + s];
        return v == v;
    }
    return present[(uint64_t)(q - Mv) * S + s] != 0;
}

// the side's distance of the samples s < t
__device__ inline double side_distance(const double *__restrict__ values, const double *__restrict__ matrices, uint32_t S, uint32_t Mv,
                                       uint32_t q, uint32_t s, uint32_t t)
{
    if (q < Mv) return fabs(__dsub_rn(values[(uint64_t)q * S + s], values[(uint64_t)q * S + t]));
    return matrices[((uint64_t)(q - Mv) * S + s) * S + t];
}

__global__ __launch_bounds__(kWave) void mantel_list_kernel(const uint64_t *__restrict__ total, const double *__restrict__ values,
                                                            const uint8_t *__restrict__ present, uint32_t S, uint32_t Mv, uint32_t side,
                                                            uint32_t control, uint32_t method, uint32_t *__restrict__ idx,
                                                            MantelTest *__restrict__ test, epik_amd_mantel *__restrict__ rec)
{
    uint32_t n = 0;  // (uniform)
    for (uint32_t base = 0; base < S; base += kWave) {
        const uint32_t s = base + threadIdx.x;
        const bool flag = s < S && total[s] != 0 && side_present(values, present, S, Mv, side, s) &&
                          (control == kNone || side_present(values, present, S, Mv, control, s));
        const unsigned long long mask = __ballot(flag);
        if (flag) idx[n + __popcll(mask & ((1ull << threadIdx.x) - 1))] = s;
        n += __popcll(mask);
    }
    if (threadIdx.x == 0) {
        *test = MantelTest{};
        test->n = n, test->run = n >= 3, test->m = (uint64_t)n * (n ? n - 1 : 0) / 2;
        rec->used = n, rec->side = side, rec->method = method, rec->partial = control != kNone, rec->at_least = 0;
        rec->r = rec->r_xz = rec->r_yz = rec->stat = rec->p = na_value();
    }
}

__global__ __launch_bounds__(kWave) void anosim_list_kernel(const uint64_t *__restrict__ total, const uint32_t *__restrict__ lab, uint32_t S,
                                                            uint32_t *__restrict__ idx, uint8_t *__restrict__ lam,
                                                            MantelTest *__restrict__ test, epik_amd_anosim *__restrict__ rec)
{
    __shared__ uint32_t group_of[kGroups], size[kGroups];
    uint32_t L, G;  // (uniform)
    column_list<kGroups>(total, lab, S, kMissing, group_of, size, idx, lam, L, G);
    if (threadIdx.x == 0) {
        uint64_t within = 0;
        for (uint32_t g = 0; g < G; ++g) within += (uint64_t)size[g] * (size[g] - 1) / 2;
        *test = MantelTest{};
        test->n = L, test->run = test->defined = G >= 2 && within >= 1;
        test->m = (uint64_t)L * (L ? L - 1 : 0) / 2, test->m_within = within;
        rec->used = L, rec->groups = G, rec->at_least = 0;
        rec->r = rec->mean_between = rec->mean_within = rec->p = na_value();
    }
}

__global__ __launch_bounds__(kBlock) void mantel_strata_kernel(const uint32_t *__restrict__ strata, const uint32_t *__restrict__ idx,
                                                               const MantelTest *__restrict__ test, uint32_t *hs, uint32_t *home)
{
    strata_tables(strata, [&](uint32_t i) { return idx[i]; }, test->n, hs, home);
}

// ---- the tables --------------------------------------------------------------------------------------------------------------
struct Tables {
    double *tab[kTables];
    uint32_t count;  // the tables in use: x; x, y; x, y, z
};

// side == kNone: x alone (ANOSIM)
__global__ __launch_bounds__(kBlock) void mantel_triangle_kernel(const double *__restrict__ dist, const double *__restrict__ values,
                                                                 const double *__restrict__ matrices, uint32_t S, uint32_t Mv, uint32_t side,
                                                                 uint32_t control, const uint32_t *__restrict__ idx,
                                                                 const MantelTest *__restrict__ test, const Tables t)
{
    if (!test->run) return;
    const uint64_t n = test->n, cells = n * n;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock) {
        const uint32_t i = (uint32_t)(e / n), j = (uint32_t)(e - i * n);
        double x = 0.0, y = 0.0, z = 0.0;  // (the diagonal is never used)
        if (i != j) {
            const uint32_t s = idx[i < j ? i : j], u = idx[i < j ? j : i];  // (s < u: the list ascends)
            x = dist[(uint64_t)s * S + u];
            if (side != kNone) y = side_distance(values, matrices, S, Mv, side, s, u);
            if (control != kNone) z = side_distance(values, matrices, S, Mv, control, s, u);
        }
        t.tab[0][e] = x;
        if (side != kNone) t.tab[1][e] = y;
        if (control != kNone) t.tab[2][e] = z;
    }
}

// the pairs of the table in i-major order into sorted[0 .. m), +inf beyond
__global__ __launch_bounds__(kBlock) void rank_fill_kernel(const double *__restrict__ tab, const MantelTest *__restrict__ test,
                                                           double *__restrict__ sorted, uint32_t P2)
{
    if (!test->run) return;
    const uint64_t n = test->n, cells = n * n, first = (uint64_t)blockIdx.x * kBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t e = first; e < cells; e += stride) {
        const uint64_t i = e / n, j = e - i * n;
        if (i < j) sorted[i * (2 * n - i - 1) / 2 + (j - i - 1)] = tab[e];  // (below m <= P2)
    }
    for (uint64_t e = test->m + first; e < P2; e += stride) sorted[e] = HUGE_VAL;
}

// The bitonic network over v[0 .. P2), P2 a power of two, ascending.  A workgroup a tile of min(kSortTile, P2) values in LDS:
// the steps below the tile of the widths first .. last (first == 2: every tile sorted; first == last beyond the tile: the tail
// of that width's merge, whose wider strides sort_global_kernel made).
__global__ __launch_bounds__(kBlock) void sort_tile_kernel(double *__restrict__ v, uint32_t P2, uint32_t first, uint32_t last,
                                                           const MantelTest *__restrict__ test)
{
    __shared__ double tile[kSortTile];
    if (!test->run) return;
    const uint32_t count = min(kSortTile, P2);
    for (uint64_t base = (uint64_t)blockIdx.x * count; base < P2; base += (uint64_t)gridDim.x * count) {
        for (uint32_t e = threadIdx.x; e < count; e += kBlock) tile[e] = v[base + e];
        __syncthreads();
        for (uint64_t width = first; width <= last; width <<= 1)
            for (uint32_t step = width / 2 < count / 2 ? (uint32_t)(width / 2) : count / 2; step > 0; step >>= 1) {
                for (uint32_t e = threadIdx.x; e < count / 2; e += kBlock) {
                    const uint32_t lo = 2 * e - (e & (step - 1)), hi = lo + step;  // (hi < count)
                    const bool up = ((base + lo) & width) == 0;
                    const double a = tile[lo], c = tile[hi];
                    if ((a > c) == up) tile[lo] = c, tile[hi] = a;
                }
                __syncthreads();
            }
        for (uint32_t e = threadIdx.x; e < count; e += kBlock) v[base + e] = tile[e];
        __syncthreads();  // (the tile is written again)
    }
}

// one step of the network at a stride of a tile or more, in global memory
__global__ __launch_bounds__(kBlock) void sort_global_kernel(double *__restrict__ v, uint32_t P2, uint32_t width, uint32_t step,
                                                             const MantelTest *__restrict__ test)
{
    if (!test->run) return;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < P2 / 2; e += (uint64_t)gridDim.x * kBlock) {
        const uint64_t lo = 2 * e - (e & (step - 1)), hi = lo + step;  // (hi < P2)
        const bool up = (lo & width) == 0;
        const double a = v[lo], c = v[hi];
        if ((a > c) == up) v[lo] = c, v[hi] = a;
    }
}

// every cell's midrank over its value (a cell reads itself only)
__global__ __launch_bounds__(kBlock) void rank_write_kernel(double *__restrict__ tab, const MantelTest *__restrict__ test,
                                                            const double *__restrict__ sorted, uint32_t P2)
{
    if (!test->run) return;
    const uint64_t n = test->n, cells = n * n;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock)
        if (e / n != e % n) tab[e] = midrank_sorted(sorted, P2, tab[e]);
}

// ---- the moments -------------------------------------------------------------------------------------------------------------
// rows[k][i] = the chain over j > i of table k: a lane a row, down the column (the table is symmetric bit for bit)
__global__ __launch_bounds__(kBlock) void mantel_rowsum_kernel(const Tables t, const MantelTest *__restrict__ test, double *__restrict__ rows,
                                                               uint32_t padded)
{
    if (!test->run) return;
    const uint64_t n = test->n, units = t.count * n;
    for (uint64_t unit = (uint64_t)blockIdx.x * kBlock + threadIdx.x; unit < units; unit += (uint64_t)gridDim.x * kBlock) {
        const uint32_t k = (uint32_t)(unit / n), i = (uint32_t)(unit - k * n);
        const double *column = t.tab[k] + i;
        double acc = 0.0;
#pragma unroll 4
        for (uint64_t j = i + 1; j < n; ++j) acc = __dadd_rn(acc, column[j * n]);
        rows[(uint64_t)k * padded + i] = acc;
    }
}

// the chain of rows[0 .. n - 1): one lane's work
__device__ inline double chain_of_rows(const double *__restrict__ rows, uint32_t n)
{
    double acc = 0.0;
#pragma unroll 4
    for (uint32_t i = 0; i + 1 < n; ++i) acc = __dadd_rn(acc, rows[i]);
    return acc;
}

__global__ __launch_bounds__(kWave) void mantel_mean_kernel(uint32_t tables, MantelTest *__restrict__ test, const double *__restrict__ rows,
                                                            uint32_t padded)
{
    if (!test->run) return;
    if (threadIdx.x < tables)
        test->mean[threadIdx.x] = __ddiv_rn(chain_of_rows(rows + (uint64_t)threadIdx.x * padded, test->n), (double)test->m);
}

__global__ __launch_bounds__(kBlock) void mantel_centre_kernel(const Tables t, const MantelTest *__restrict__ test)
{
    if (!test->run) return;
    const uint64_t n = test->n, cells = n * n;
    for (uint32_t k = 0; k < t.count; ++k) {
        const double mean = test->mean[k];
        for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock)
            if (e / n != e % n) t.tab[k][e] = __dsub_rn(t.tab[k][e], mean);
    }
}

// rows[c][i] = the chain over j > i of the product c: xx, yy, xy and, with a control, zz, xz, yz
__global__ __launch_bounds__(kBlock) void mantel_rowprod_kernel(const Tables t, const MantelTest *__restrict__ test,
                                                                double *__restrict__ rows, uint32_t padded)
{
    if (!test->run) return;
    const uint64_t n = test->n, units = (t.count == kTables ? kProducts : 3) * n;
    for (uint64_t unit = (uint64_t)blockIdx.x * kBlock + threadIdx.x; unit < units; unit += (uint64_t)gridDim.x * kBlock) {
        const uint32_t c = (uint32_t)(unit / n), i = (uint32_t)(unit - c * n);
        // xx yy xy zz xz yz
        const double *a = t.tab[c == 1 || c == 5 ? 1 : c == 3 ? 2 : 0] + i, *b = t.tab[c == 0 ? 0 : c == 1 || c == 2 ? 1 : 2] + i;
        double acc = 0.0;
#pragma unroll 4
        for (uint64_t j = i + 1; j < n; ++j) acc = __dadd_rn(acc, __dmul_rn(a[j * n], b[j * n]));
        rows[(uint64_t)c * padded + i] = acc;
    }
}

// the rule's partial statistic; false where a radicand is not > 0
__device__ inline bool partial_statistic(double r_xy, double r_xz, double r_yz, double &stat)
{
    const double rad_x = __dsub_rn(1.0, __dmul_rn(r_xz, r_xz)), rad_y = __dsub_rn(1.0, __dmul_rn(r_yz, r_yz));
    if (!(rad_x > 0.0) || !(rad_y > 0.0)) return false;
    stat = __ddiv_rn(__dsub_rn(r_xy, __dmul_rn(r_xz, r_yz)), __dmul_rn(__dsqrt_rn(rad_x), __dsqrt_rn(rad_y)));
    return true;
}

__global__ __launch_bounds__(kWave) void mantel_observed_kernel(uint32_t tables, MantelTest *__restrict__ test, const double *__restrict__ rows,
                                                                uint32_t padded, epik_amd_mantel *__restrict__ rec, double *__restrict__ stat)
{
    __shared__ double s[kProducts];
    if (!test->run) return;
    const bool partial = tables == kTables;
    if (threadIdx.x < (partial ? kProducts : 3)) s[threadIdx.x] = chain_of_rows(rows + (uint64_t)threadIdx.x * padded, test->n);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double ss_x = s[0], ss_y = s[1];
    if (ss_x == 0.0 || ss_y == 0.0 || (partial && s[3] == 0.0)) return;
    const double den_xy = __dsqrt_rn(__dmul_rn(ss_x, ss_y)), r_xy = __ddiv_rn(s[2], den_xy);
    double den_xz = 0.0, r_xz = na_value(), r_yz = na_value(), stat0 = r_xy;
    if (partial) {
        den_xz = __dsqrt_rn(__dmul_rn(ss_x, s[3]));
        r_xz = __ddiv_rn(s[4], den_xz), r_yz = __ddiv_rn(s[5], __dsqrt_rn(__dmul_rn(ss_y, s[3])));
        if (!partial_statistic(r_xy, r_xz, r_yz, stat0)) return;
    }
    rec->r = r_xy, rec->r_xz = r_xz, rec->r_yz = r_yz, rec->stat = stat0;
    if (stat) stat[0] = stat0;
    test->den_xy = den_xy, test->den_xz = den_xz, test->r_yz = r_yz, test->stat0 = stat0, test->defined = 1;
}

// ---- the permutations --------------------------------------------------------------------------------------------------------
struct CrossArgs {
    const double *x, *y, *z;       // the tables of the test; z null without a control; ANOSIM: x alone, the midranks
    const uint8_t *lam;            // ANOSIM: the groups of the positions
    const uint32_t *hs, *home;     // the strata rule's tables of the list, or null
    MantelTest *test;
    unsigned long long *at_least;  // of the test's record
    void *record;                  // ANOSIM: the record, for p = 0
    double *stat;                  // the test's row [P + 1], or null
    double *scratch;
    uint64_t seed;
    uint32_t p_first, p_last, pitch;
};

template <bool kLds, bool kStrata, bool kAnosim>
__global__ __launch_bounds__(kBlock) void mantel_cross_kernel(const CrossArgs a)
{
    extern __shared__ __align__(16) unsigned char dynamic_lds[];
    __shared__ double total[2 * kPerms];
    __shared__ unsigned long long within[kPerms];
    const MantelTest info = *a.test;
    if (!info.defined) return;  // (uniform)
    const uint32_t tid = threadIdx.x, threads = blockDim.x, pitch = a.pitch, n = info.n;
    const bool control = a.z != nullptr;
    const uint32_t chains = control ? 2 * kPerms : kPerms;
    // t[chains][pitch] | sigma[pitch] | mu[pitch] (| hs[pitch] | home[pitch] in LDS); the keys and the sort's positions live in
    // t's place, which the rows write after the last arrangement is made
    double *t;
    uint64_t *sigma;
    if (kLds) {
        t = reinterpret_cast<double *>(dynamic_lds);
        sigma = reinterpret_cast<uint64_t *>(t + (size_t)chains * pitch);
    } else {
        // (kSliceBytes * pitch bytes a slice, pitch % 32 == 0: every slice is aligned)
        t = reinterpret_cast<double *>(reinterpret_cast<char *>(a.scratch) + (uint64_t)blockIdx.x * kSliceBytes * pitch);
        sigma = reinterpret_cast<uint64_t *>(t + (size_t)2 * kPerms * pitch);
    }
    uint32_t *mu = reinterpret_cast<uint32_t *>(sigma + pitch);
    uint64_t *keys = reinterpret_cast<uint64_t *>(t);
    uint32_t *pos = reinterpret_cast<uint32_t *>(keys + pitch);
    uint16_t *sigma16 = reinterpret_cast<uint16_t *>(sigma);
    uint8_t *mu8 = reinterpret_cast<uint8_t *>(mu);
    const uint32_t *hs = a.hs, *home = a.home;
    if constexpr (kLds && kStrata) {
        uint32_t *lds_hs = mu + pitch, *lds_home = lds_hs + pitch;
        for (uint32_t i = tid; i < n; i += threads) lds_hs[i] = hs[i], lds_home[i] = home[i];
        hs = lds_hs, home = lds_home;
    }
    const uint32_t wave = tid / kWave, lane = tid % kWave, waves = threads / kWave;
    const uint32_t chunks = (a.p_last - a.p_first + kPerms) / kPerms;
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const uint32_t p0 = a.p_first + chunk * kPerms, np = min(kPerms, a.p_last + 1 - p0);
        __syncthreads();  // (the strata's tables are there; the vectors are written again)
        for (uint32_t k = 0; k < kPerms; ++k) {
            const uint32_t p = p0 + k;
            if (k >= np || p == 0) {  // the identity: permutation 0, and the filling, whose gathers stay inside the table
                for (uint32_t i = tid; i < n; i += threads) sigma16[i * kPerms + k] = (uint16_t)i;
                continue;
            }
            for (uint32_t i = tid; i < n; i += threads) keys[i] = permutation_key(a.seed, p, i);
            __syncthreads();
            if (kLds && n > kCountPositions) {
                // (key, position) sorted by a bitonic network over the next power of two, the padding above every pair:
                // the slot of a pair is its rank
                uint32_t P2 = 2 * kCountPositions;
                while (P2 < n) P2 <<= 1;  // (<= pitch)
                for (uint32_t i = tid; i < P2; i += threads) {
                    pos[i] = i < n ? i : 0xffffffffu;
                    if (i >= n) keys[i] = ~0ull;
                }
                __syncthreads();
                for (uint32_t width = 2; width <= P2; width <<= 1)
                    for (uint32_t step = width >> 1; step > 0; step >>= 1) {
                        for (uint32_t e = tid; e < P2 / 2; e += threads) {
                            const uint32_t lo = 2 * e - (e & (step - 1)), hi = lo + step;  // (hi < P2)
                            const bool up = (lo & width) == 0;
                            const uint64_t ka = keys[lo], kc = keys[hi];
                            const uint32_t pa = pos[lo], pc = pos[hi];
                            bool above;
                            if constexpr (kStrata)  // (the padding's position is no index: its stratum is above every other)
                                above = strata_before(pc < n ? hs[pc] : 0xffffffffu, kc, pc, pa < n ? hs[pa] : 0xffffffffu, ka, pa);
                            else
                                above = ka > kc || (ka == kc && pa > pc);
                            if (above == up) keys[lo] = kc, keys[hi] = ka, pos[lo] = pc, pos[hi] = pa;
                        }
                        __syncthreads();
                    }
                for (uint32_t r = tid; r < n; r += threads) sigma16[pos[r] * kPerms + k] = (uint16_t)(kStrata ? home[r] : r);
            } else {
                for (uint32_t i = tid; i < n; i += threads) {
                    const uint64_t mine = keys[i];
                    uint32_t rank = 0;
#pragma unroll 4
                    for (uint32_t j = 0; j < n; ++j) {
                        const uint64_t other = keys[j];  // a broadcast
                        if constexpr (kStrata) rank += strata_before(hs[j], other, j, hs[i], mine, i);
                        else rank += other < mine || (other == mine && j < i);
                    }
                    sigma16[i * kPerms + k] = (uint16_t)(kStrata ? home[rank] : rank);
                }
            }
            __syncthreads();  // (the keys are written again)
        }
        __syncthreads();
        if constexpr (kAnosim) {
            for (uint32_t e = tid; e < n * kPerms; e += threads) mu8[e] = a.lam[sigma16[e]];
            if (tid < kPerms) within[tid] = 0;
            __syncthreads();
        }
        // 64 rows and the mirrored 64 in one wave, j walked together: the rows 0 .. n - 2 have a chain
        const uint32_t blocks = (n - 1 + kWave - 1) / kWave;
        for (uint32_t h = wave; h < (blocks + 1) / 2; h += waves)
            for (uint32_t mirrored = 0; mirrored < 2; ++mirrored) {
                const uint32_t b = mirrored ? blocks - 1 - h : h;
                if (mirrored && b == h) break;
                const uint32_t i0 = b * kWave, i = i0 + lane;
                const bool live = i + 1 < n;
                const uint32_t ic = live ? i : n - 1;  // (a lane without a row reads the last one and adds nothing)
                if constexpr (kAnosim) {
                    const uint32_t mine = mu[ic];
                    unsigned long long w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll 4
                    for (uint32_t j = i0 + 1; j < n; ++j) {
                        const uint32_t differ = mu[j] ^ mine;  // a broadcast
                        const unsigned long long twice = (unsigned long long)__dmul_rn(2.0, a.x[(uint64_t)j * n + ic]);
                        const unsigned long long add = j > i ? twice : 0;
                        if (!(differ & 0x000000ffu)) w0 += add;
                        if (!(differ & 0x0000ff00u)) w1 += add;
                        if (!(differ & 0x00ff0000u)) w2 += add;
                        if (!(differ & 0xff000000u)) w3 += add;
                    }
                    if (live) {
                        if (w0) atomicAdd(&within[0], w0);
                        if (w1) atomicAdd(&within[1], w1);
                        if (w2) atomicAdd(&within[2], w2);
                        if (w3) atomicAdd(&within[3], w3);
                    }
                } else {
                    const uint64_t si = sigma[ic];
                    const double *x0 = a.x + (si & 0xffffu), *x1 = a.x + (si >> 16 & 0xffffu), *x2 = a.x + (si >> 32 & 0xffffu),
                                 *x3 = a.x + (si >> 48);
                    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, u0 = 0.0, u1 = 0.0, u2 = 0.0, u3 = 0.0;
#pragma unroll 4  // (the reads of four steps are in flight ahead of the dependent adds)
                    for (uint32_t j = i0 + 1; j < n; ++j) {
                        const uint64_t sj = sigma[j];  // a broadcast
                        const bool mine = j > i;
                        const double v0 = x0[(sj & 0xffffu) * n], v1 = x1[(sj >> 16 & 0xffffu) * n], v2 = x2[(sj >> 32 & 0xffffu) * n],
                                     v3 = x3[(sj >> 48) * n];
                        const double y = a.y[(uint64_t)j * n + ic];
                        if (mine) {
                            t0 = __dadd_rn(t0, __dmul_rn(v0, y)), t1 = __dadd_rn(t1, __dmul_rn(v1, y));
                            t2 = __dadd_rn(t2, __dmul_rn(v2, y)), t3 = __dadd_rn(t3, __dmul_rn(v3, y));
                        }
                        if (control) {  // (uniform)
                            const double z = a.z[(uint64_t)j * n + ic];
                            if (mine) {
                                u0 = __dadd_rn(u0, __dmul_rn(v0, z)), u1 = __dadd_rn(u1, __dmul_rn(v1, z));
                                u2 = __dadd_rn(u2, __dmul_rn(v2, z)), u3 = __dadd_rn(u3, __dmul_rn(v3, z));
                            }
                        }
                    }
                    if (live) {
                        t[i] = t0, t[pitch + i] = t1, t[2 * pitch + i] = t2, t[3 * pitch + i] = t3;
                        if (control) t[4 * pitch + i] = u0, t[5 * pitch + i] = u1, t[6 * pitch + i] = u2, t[7 * pitch + i] = u3;
                    }
                }
            }
        __syncthreads();
        if constexpr (!kAnosim) {
            if (tid < chains) total[tid] = chain_of_rows(t + (size_t)tid * pitch, n);
            __syncthreads();
        }
        if (tid == 0) {
            unsigned long long count = 0;
            for (uint32_t k = 0; k < np; ++k) {
                double value;
                bool counted = true;
                if constexpr (kAnosim) {
                    const double w = __dmul_rn(0.5, (double)within[k]), all = (double)(info.m * (info.m + 1) / 2);
                    const double mean_within = __ddiv_rn(w, (double)info.m_within);
                    const double mean_between = __ddiv_rn(__dsub_rn(all, w), (double)(info.m - info.m_within));
                    value = __ddiv_rn(__dsub_rn(mean_between, mean_within), __ddiv_rn((double)info.m, 2.0));
                    if (p0 + k == 0) {
                        epik_amd_anosim *rec = static_cast<epik_amd_anosim *>(a.record);
                        rec->r = value, rec->mean_between = mean_between, rec->mean_within = mean_within;
                        a.test->stat0 = value;
                        counted = false;
                    }
                } else {
                    value = __ddiv_rn(total[k], info.den_xy);
                    if (control && !partial_statistic(value, __ddiv_rn(total[kPerms + k], info.den_xz), info.r_yz, value))
                        value = na_value(), counted = false;
                }
                if (a.stat) a.stat[p0 + k] = value;
                count += counted && value >= info.stat0;
            }
            if (count) atomicAdd(a.at_least, count);
        }
    }
}

// record: epik_amd_mantel or epik_amd_anosim
template <class Record>
__global__ __launch_bounds__(kBlock) void mantel_finish_kernel(const MantelTest *__restrict__ tests, uint32_t num_tests,
                                                               uint32_t num_permutations, Record *__restrict__ out, double *__restrict__ stat)
{
    const uint64_t first = (uint64_t)blockIdx.x * kBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t test = first; test < num_tests; test += stride)
        if (tests[test].defined) out[test].p = __ddiv_rn((double)(1 + out[test].at_least), (double)(num_permutations + 1));
    if (!stat) return;
    const uint64_t row = (uint64_t)num_permutations + 1;
    for (uint64_t e = first; e < num_tests * row; e += stride)
        if (!tests[e / row].defined) stat[e] = na_value();
}

// ---- the host side -----------------------------------------------------------------------------------------------------------
struct Launch {
    epik_amd_cohort *cohort;
    hipStream_t stream;
    uint32_t S, padded, P2, pitch;
    bool lds, strata, control;
    dim3 cells() const { return cohort_grid(cohort, ((uint64_t)S * S + kBlock - 1) / kBlock, kManyBlocks); }
    dim3 rows(uint32_t vectors) const { return cohort_grid(cohort, ((uint64_t)vectors * S + kBlock - 1) / kBlock, kManyBlocks); }
};

// the midranks of table `tab` in its place
void enqueue_ranks(const Launch &l, double *tab, const MantelSpace &sp, const MantelTest *test)
{
    const uint32_t P2 = l.P2, tile = std::min(kSortTile, P2);
    const dim3 tiles = cohort_grid(l.cohort, P2 / tile, kManyBlocks), halves = cohort_grid(l.cohort, (P2 / 2 + kBlock - 1) / kBlock, kManyBlocks);
    hipLaunchKernelGGL(rank_fill_kernel, cohort_grid(l.cohort, (std::max<uint64_t>((uint64_t)l.S * l.S, P2) + kBlock - 1) / kBlock, kManyBlocks),
                       dim3(kBlock), 0, l.stream, tab, test, sp.sorted, P2);
    hipLaunchKernelGGL(sort_tile_kernel, tiles, dim3(kBlock), 0, l.stream, sp.sorted, P2, 2u, tile, test);
    for (uint64_t width = 2ull * tile; width <= P2; width <<= 1) {
        for (uint64_t step = width >> 1; step >= tile; step >>= 1)
            hipLaunchKernelGGL(sort_global_kernel, halves, dim3(kBlock), 0, l.stream, sp.sorted, P2, (uint32_t)width, (uint32_t)step, test);
        hipLaunchKernelGGL(sort_tile_kernel, tiles, dim3(kBlock), 0, l.stream, sp.sorted, P2, (uint32_t)width, (uint32_t)width, test);
    }
    hipLaunchKernelGGL(rank_write_kernel, l.cells(), dim3(kBlock), 0, l.stream, tab, test, sp.sorted, P2);
}

template <bool kAnosim>
void enqueue_cross(const Launch &l, const CrossArgs &args)
{
    const uint32_t chains = l.control ? 2 * kPerms : kPerms;
    const size_t dynamic = l.lds ? (size_t)l.pitch * (chains * 8 + 8 + 4 + (l.strata ? 4 + 4 : 0)) : 0;
    const dim3 block(l.S <= kSmallSamples ? kWave : kBlock);
    const uint64_t chunks = ((uint64_t)args.p_last - args.p_first + kPerms) / kPerms;
    const dim3 grid = cohort_grid(l.cohort, chunks, l.lds ? kManyBlocks : kGeneralBlocks);
    if (l.lds) {
        if (l.strata) hipLaunchKernelGGL((mantel_cross_kernel<true, true, kAnosim>), grid, block, dynamic, l.stream, args);
        else hipLaunchKernelGGL((mantel_cross_kernel<true, false, kAnosim>), grid, block, dynamic, l.stream, args);
    } else {
        if (l.strata) hipLaunchKernelGGL((mantel_cross_kernel<false, true, kAnosim>), grid, block, 0, l.stream, args);
        else hipLaunchKernelGGL((mantel_cross_kernel<false, false, kAnosim>), grid, block, 0, l.stream, args);
    }
}

// what both analyses start with: the checks of the handle, the device drained, the workspace; `bytes` sizes it
int begin_analysis(epik_amd_cohort *cohort, size_t bytes)
{
    COHORT_TRY(check_has_distances(cohort));
    HIP_TRY(hipSetDevice(cohort->device));
    HIP_TRY(hipDeviceSynchronize());  // (the distances enqueued on whatever stream, and an earlier call that reads the workspace)
    return cohort_space_ensure(cohort, kSpaceMantel, bytes);
}

Launch make_launch(epik_amd_cohort *cohort, hipStream_t stream, bool ranks, bool strata, bool control)
{
    const uint32_t S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    // (=0, tests: the general path whatever S)
    const bool lds = lds_switch("EPIK_AMD_MANTEL_LDS", S, control ? kLdsControlPositions : kLdsPositions);
    uint32_t pitch = padded;  // the general path's; the LDS path's: a power of two, for the sort
    if (lds)
        for (pitch = kWave; pitch < S; pitch <<= 1) {}
    return Launch{cohort, stream, S, padded, ranks ? sort_size(S) : 0, pitch, lds, strata, control};
}

int mantel_device_impl(epik_amd_cohort *cohort, const void *d_dist, const mantel_sides &sides, const uint32_t *strata, uint32_t P,
                       uint64_t seed, void *d_out, void *d_stat, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(check_present(d_dist, d_out));
    const uint32_t S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    std::string err;
    COHORT_TRY(rule_result(mantel_arguments_valid(sides, S, P, err), err));
    const uint32_t Mv = sides.num_columns, Mm = sides.num_matrices, tests = sides.tests();
    const bool control = sides.control != kNone, ranks = (sides.methods & EPIK_AMD_MANTEL_SPEARMAN) != 0;
    const uint32_t tables = control ? kTables : 2;
    COHORT_TRY(begin_analysis(cohort, mantel_space(nullptr, S, padded, Mv, Mm, 0, tables, ranks, strata != nullptr, tests, nullptr)));
    MantelSpace sp;
    mantel_space(cohort->space[kSpaceMantel].d, S, padded, Mv, Mm, 0, tables, ranks, strata != nullptr, tests, &sp);
    if (Mv) HIP_TRY(hipMemcpy(sp.values, sides.values, (size_t)Mv * S * sizeof(double), hipMemcpyHostToDevice));
    if (Mm) {
        HIP_TRY(hipMemcpy(sp.matrices, sides.matrices, (size_t)Mm * S * S * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(sp.present, sides.matrix_present, (size_t)Mm * S, hipMemcpyHostToDevice));
    }
    if (strata) COHORT_TRY(upload_strata(strata, S, padded, sp.strata));
    auto *out = static_cast<epik_amd_mantel *>(d_out);
    auto *stat = static_cast<double *>(d_stat);
    const dim3 one(1), wave(kWave), block(kBlock);
    uint32_t index = 0;
    for (uint32_t q = 0; q < Mv + Mm; ++q)
        for (uint32_t method = 0; method < 2; ++method) {
            if (!(sides.methods >> method & 1u)) continue;
            const uint32_t z = control && sides.control != q ? sides.control : kNone;
            const Launch l = make_launch(cohort, stream, ranks, strata != nullptr, z != kNone);
            MantelTest *test = sp.tests + index;
            epik_amd_mantel *rec = out + index;
            double *row = stat ? stat + (uint64_t)index * (P + 1) : nullptr;
            ++index;
            const Tables t{{sp.tab[0], sp.tab[1], z != kNone ? sp.tab[2] : nullptr}, z != kNone ? kTables : 2};
            hipLaunchKernelGGL(mantel_list_kernel, one, wave, 0, stream, cohort->d_total, sp.values, sp.present, S, Mv, q, z, method, sp.idx,
                               test, rec);
            if (strata) hipLaunchKernelGGL(mantel_strata_kernel, one, block, 0, stream, sp.strata, sp.idx, test, sp.hs, sp.home);
            hipLaunchKernelGGL(mantel_triangle_kernel, l.cells(), block, 0, stream, static_cast<const double *>(d_dist), sp.values,
                               sp.matrices, S, Mv, q, z, sp.idx, test, t);
            if (method == 1)
                for (uint32_t k = 0; k < t.count; ++k) enqueue_ranks(l, t.tab[k], sp, test);
            hipLaunchKernelGGL(mantel_rowsum_kernel, l.rows(t.count), block, 0, stream, t, test, sp.rows, padded);
            hipLaunchKernelGGL(mantel_mean_kernel, one, wave, 0, stream, t.count, test, sp.rows, padded);
            hipLaunchKernelGGL(mantel_centre_kernel, l.cells(), block, 0, stream, t, test);
            hipLaunchKernelGGL(mantel_rowprod_kernel, l.rows(kProducts), block, 0, stream, t, test, sp.rows, padded);
            hipLaunchKernelGGL(mantel_observed_kernel, one, wave, 0, stream, t.count, test, sp.rows, padded, rec, row);
            const CrossArgs args{t.tab[0], t.tab[1], t.tab[2], nullptr, strata ? sp.hs : nullptr, strata ? sp.home : nullptr, test,
                                 reinterpret_cast<unsigned long long *>(&rec->at_least), rec, row, sp.scratch, seed, 1, P, l.pitch};
            enqueue_cross<false>(l, args);
        }
    const uint64_t finish = stat ? (uint64_t)tests * (P + 1) : tests;
    hipLaunchKernelGGL(mantel_finish_kernel<epik_amd_mantel>, cohort_grid(cohort, (finish + kBlock - 1) / kBlock, kManyBlocks), block, 0,
                       stream, sp.tests, tests, P, out, stat);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

int anosim_device_impl(epik_amd_cohort *cohort, const void *d_dist, const uint32_t *labels, const uint32_t *strata, uint32_t M, uint32_t P,
                       uint64_t seed, void *d_out, void *d_stat, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(check_columns(M));
    COHORT_TRY(check_present(d_dist, labels, d_out));
    const uint32_t S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    std::string err;
    COHORT_TRY(rule_result(anosim_arguments_valid(labels, S, M, P, err), err));
    COHORT_TRY(begin_analysis(cohort, mantel_space(nullptr, S, padded, 0, 0, M, 1, true, strata != nullptr, M, nullptr)));
    MantelSpace sp;
    mantel_space(cohort->space[kSpaceMantel].d, S, padded, 0, 0, M, 1, true, strata != nullptr, M, &sp);
    COHORT_TRY(upload_labels_by_column(labels, S, M, padded, kMissing, sp.lab));
    if (strata) COHORT_TRY(upload_strata(strata, S, padded, sp.strata));
    auto *out = static_cast<epik_amd_anosim *>(d_out);
    auto *stat = static_cast<double *>(d_stat);
    const dim3 one(1), wave(kWave), block(kBlock);
    const Launch l = make_launch(cohort, stream, true, strata != nullptr, false);
    const Tables t{{sp.tab[0], nullptr, nullptr}, 1};
    for (uint32_t c = 0; c < M; ++c) {
        MantelTest *test = sp.tests + c;
        double *row = stat ? stat + (uint64_t)c * (P + 1) : nullptr;
        hipLaunchKernelGGL(anosim_list_kernel, one, wave, 0, stream, cohort->d_total, sp.lab + (uint64_t)c * padded, S, sp.idx, sp.lam, test,
                           out + c);
        if (strata) hipLaunchKernelGGL(mantel_strata_kernel, one, block, 0, stream, sp.strata, sp.idx, test, sp.hs, sp.home);
        hipLaunchKernelGGL(mantel_triangle_kernel, l.cells(), block, 0, stream, static_cast<const double *>(d_dist), nullptr, nullptr, S, 0u,
                           kNone, kNone, sp.idx, test, t);
        enqueue_ranks(l, t.tab[0], sp, test);
        CrossArgs args{t.tab[0], nullptr, nullptr, sp.lam, strata ? sp.hs : nullptr, strata ? sp.home : nullptr, test,
                       reinterpret_cast<unsigned long long *>(&out[c].at_least), out + c, row, sp.scratch, seed, 0, 0, l.pitch};
        enqueue_cross<true>(l, args);  // R_0, which the permutations are set against
        args.p_first = 1, args.p_last = P;
        enqueue_cross<true>(l, args);
    }
    const uint64_t finish = stat ? (uint64_t)M * (P + 1) : M;
    hipLaunchKernelGGL(mantel_finish_kernel<epik_amd_anosim>, cohort_grid(cohort, (finish + kBlock - 1) / kBlock, kManyBlocks), block, 0,
                       stream, sp.tests, M, P, out, stat);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

}  // namespace

extern "C" {

int epik_amd_cohort_mantel_device(epik_amd_cohort *cohort, const void *d_dist, const double *values, uint32_t num_columns,
                                  const double *matrices, const uint8_t *matrix_present, uint32_t num_matrices, uint32_t methods,
                                  uint32_t control, uint32_t num_permutations, uint64_t seed, const uint32_t *strata, void *d_out,
                                  void *d_stat, void *stream)
{
    return guarded("cohort_mantel_device", [&]() -> int {
        const mantel_sides sides{values, num_columns, matrices, matrix_present, num_matrices, methods, control};
        return mantel_device_impl(cohort, d_dist, sides, strata, num_permutations, seed, d_out, d_stat, static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_mantel(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                           const double *values, uint32_t num_columns, const double *matrices, const uint8_t *matrix_present,
                           uint32_t num_matrices, uint32_t methods, uint32_t control, uint32_t num_permutations, uint64_t seed,
                           const uint32_t *strata, epik_amd_mantel *out, double *stat)
{
    return guarded("cohort_mantel", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(check_present(out));
        const uint32_t S = cohort->num_samples;
        const mantel_sides sides{values, num_columns, matrices, matrix_present, num_matrices, methods, control};
        std::string err;
        COHORT_TRY(rule_result(mantel_arguments_valid(sides, S, num_permutations, err), err));
        const size_t tests = sides.tests(), out_bytes = tests * sizeof(epik_amd_mantel);
        const size_t stat_bytes = tests * ((size_t)num_permutations + 1) * sizeof(double);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult dist, r, s;
        COHORT_TRY(dist.alloc((size_t)S * S * sizeof(double)));
        COHORT_TRY(r.alloc(out_bytes));
        COHORT_TRY(s.alloc(stat_bytes, stat != nullptr));
        COHORT_TRY(cohort_distance_enqueue(cohort, tree, branch_length, metric, dist.d, nullptr));
        COHORT_TRY(mantel_device_impl(cohort, dist.d, sides, strata, num_permutations, seed, r.d, s.d, nullptr));
        COHORT_TRY(r.copy_to(out, out_bytes));
        return s.copy_to(stat, stat_bytes);
    });
}

int epik_amd_cohort_mantel_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                const double *branch_length, uint32_t metric, const double *values, uint32_t num_columns,
                                const double *matrices, const uint8_t *matrix_present, uint32_t num_matrices, uint32_t methods,
                                uint32_t control, uint32_t num_permutations, uint64_t seed, const uint32_t *strata,
                                epik_amd_mantel *out, double *stat)
{
    return guarded("cohort_mantel_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(check_present(mass, first, branch_length, out));
        const mantel_sides sides{values, num_columns, matrices, matrix_present, num_matrices, methods, control};
        std::string err;
        return rule_result(mantel_records(mass, num_samples, num_branches, first, branch_length, sides, num_permutations, seed, out, stat,
                                          err, metric, strata),
                           err);
    });
}

int epik_amd_cohort_mantel_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const double *values,
                                   uint32_t num_columns, const double *matrices, const uint8_t *matrix_present,
                                   uint32_t num_matrices, uint32_t methods, uint32_t control, uint32_t num_permutations,
                                   uint64_t seed, const uint32_t *strata, epik_amd_mantel *out, double *stat)
{
    return guarded("cohort_mantel_kr_host", [&]() -> int {
        COHORT_TRY(check_host_samples(num_samples));
        COHORT_TRY(check_present(kr, totals, out));
        const mantel_sides sides{values, num_columns, matrices, matrix_present, num_matrices, methods, control};
        std::string err;
        return rule_result(mantel_records_of_kr(kr, totals, num_samples, sides, num_permutations, seed, out, stat, err, strata), err);
    });
}

int epik_amd_cohort_anosim_device(epik_amd_cohort *cohort, const void *d_dist, const uint32_t *labels, uint32_t num_columns,
                                  uint32_t num_permutations, uint64_t seed, const uint32_t *strata, void *d_out, void *d_stat,
                                  void *stream)
{
    return guarded("cohort_anosim_device", [&]() -> int {
        return anosim_device_impl(cohort, d_dist, labels, strata, num_columns, num_permutations, seed, d_out, d_stat,
                                  static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_anosim(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                           const uint32_t *labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed,
                           const uint32_t *strata, epik_amd_anosim *out, double *stat)
{
    return guarded("cohort_anosim", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(check_columns(num_columns));
        COHORT_TRY(check_present(labels, out));
        const uint32_t S = cohort->num_samples;
        std::string err;
        COHORT_TRY(rule_result(anosim_arguments_valid(labels, S, num_columns, num_permutations, err), err));
        const size_t out_bytes = (size_t)num_columns * sizeof(epik_amd_anosim);
        const size_t stat_bytes = (size_t)num_columns * ((size_t)num_permutations + 1) * sizeof(double);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult dist, r, s;
        COHORT_TRY(dist.alloc((size_t)S * S * sizeof(double)));
        COHORT_TRY(r.alloc(out_bytes));
        COHORT_TRY(s.alloc(stat_bytes, stat != nullptr));
        COHORT_TRY(cohort_distance_enqueue(cohort, tree, branch_length, metric, dist.d, nullptr));
        COHORT_TRY(anosim_device_impl(cohort, dist.d, labels, strata, num_columns, num_permutations, seed, r.d, s.d, nullptr));
        COHORT_TRY(r.copy_to(out, out_bytes));
        return s.copy_to(stat, stat_bytes);
    });
}

int epik_amd_cohort_anosim_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                const double *branch_length, uint32_t metric, const uint32_t *labels, uint32_t num_columns,
                                uint32_t num_permutations, uint64_t seed, const uint32_t *strata, epik_amd_anosim *out,
                                double *stat)
{
    return guarded("cohort_anosim_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(check_present(mass, first, branch_length, labels, out));
        std::string err;
        return rule_result(anosim_records(mass, num_samples, num_branches, first, branch_length, labels, num_columns, num_permutations,
                                          seed, out, stat, err, metric, strata),
                           err);
    });
}

int epik_amd_cohort_anosim_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const uint32_t *labels,
                                   uint32_t num_columns, uint32_t num_permutations, uint64_t seed, const uint32_t *strata,
                                   epik_amd_anosim *out, double *stat)
{
    return guarded("cohort_anosim_kr_host", [&]() -> int {
        COHORT_TRY(check_host_samples(num_samples));
        COHORT_TRY(check_present(kr, totals, labels, out));
        std::string err;
        return rule_result(anosim_records_of_kr(kr, totals, num_samples, labels, num_columns, num_permutations, seed, out, stat, err, strata),
                           err);
    });
}

}  // extern "C"
