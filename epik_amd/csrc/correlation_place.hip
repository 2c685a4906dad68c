// correlation_place.hip -- edge correlation with per-sample metadata and edge dispersion (Czech et al. 2019) of a cohort's
// samples on the device: epik_amd_cohort_correlation_device / _correlation / _correlation_host and
// epik_amd_cohort_dispersion_device / _dispersion / _dispersion_host (include/epik_amd.h).
//
// No reference counterpart.  The rule is stated once, in include/epik_amd.h beside the KR, squash, epca, kmeans and alpha
// rules (epik_amd/host/cohort.cpp: correlation_records and dispersion_records are the same rule on the
// CPU).  Every sum over the samples is sequential, from +0.0 in ascending j, in one lane; the midranks are counted, and a
// count is exact.  Nothing is fused (__dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn / __dsqrt_rn; the file is built with
// -ffp-contract=off as well).  NA is stored as its bit pattern and never computed.
//
// cohort_normalise_kernel (cohort_place.hip) leaves T_s and the planes C, B [b][Sp].  Then
//
//   correlation_mass_kernel     xm = mass / T_s from the cells [s][b] into a plane [b][Sp] beside C and B, a 32 x 32 tile
//                               through LDS: read branch-fastest, written sample-fastest, both coalesced.
//   correlation_lists_kernel    a workgroup a list: U of a group of columns (the host groups the columns by their pattern
//                               of missing values; columns of one group have the same U_c), or all used samples.
//   correlation_columns_kernel  the column side, once per call, a workgroup a column: y over U_c, its midranks, and, in a
//                               lane each, my, dy, syy and the same of the ranks.
//   correlation_branch_kernel   a workgroup a (branch, group): xm, xi and their midranks over U, four vectors in LDS (or,
//                               beyond kLdsSamples samples, in the workgroup's slice of global memory: the same code on
//                               another pointer, hence the same bits).  A lane ranks its j against broadcasts of all i;
//                               beyond kCountSamples samples the LDS path sorts a copy of each vector instead (a bitonic
//                               network) and a lane finds its two counts by binary search: the ranks are exact either way.
//                               Then a lane a (vector, column of the group): the sequential sums.  mx, dx, sxx and the
//                               ranks of x are formed once per group: they do not depend on y.
//                               The same kernel over the list of all used samples, without ranks or columns, is the
//                               dispersion.
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kTile = kCohortTile;                         // the planes' sample pitch is a multiple of it
constexpr uint32_t kColumns = EPIK_AMD_CORRELATION_MAX_COLUMNS;
constexpr uint32_t kAllUsed = kColumns;                         // the list after the groups': every used sample
constexpr uint32_t kLdsSamples = kCohortLdsSamples;             // the most samples whose four vectors stay in LDS (32 KiB)
constexpr uint32_t kCountSamples = kCohortCountSamples;         // up to here the LDS path counts its ranks; beyond, it sorts
constexpr uint32_t kGeneralBlocks = 256;                        // workgroups of the general path: each has a slice
constexpr uint32_t kVectors = 4;                                // xm, xi, rank(xm), rank(xi)
constexpr uint32_t kTotals = 5;                                 // the totals that end a row of cells (cohort_place.hip)
constexpr uint64_t kManyBlocks = 65536;

static_assert(sizeof(epik_amd_correlation) == 32 && sizeof(epik_amd_dispersion) == 64);
static_assert(kTile == 32 && kBlock == 256 && kLdsSamples % kBlock == 0 && 2 * kCountSamples <= kLdsSamples);

// the small tables of a call: the host fills the groups, the kernels the counts and the columns' sums
struct CorrTables {
    double stat[kColumns][2];        // syy of y_c, and of its ranks
    uint32_t count[kColumns + 1];    // L of a list
    uint32_t col_group[kColumns];    // the group of a column
    uint32_t group_rep[kColumns];    // a column of the group: its NaNs are the group's
    uint32_t group_start[kColumns + 1], group_cols[kColumns];  // the columns of group g: group_cols[start[g] .. start[g + 1])
    uint32_t num_groups;
};

struct CorrSpace {
    double *X;        // [N][Sp]: xm by sample
    double *y;        // [64][Sp]: the columns by sample
    double *dy, *dr;  // [64][Sp]: by j, y - my and rank(y) - its mean
    double *scratch;  // [kGeneralBlocks][4][Sp]
    uint32_t *lists;  // [65][Sp]
    CorrTables *tab;
};

size_t correlation_space(void *base, uint32_t N, uint32_t padded, CorrSpace *sp)
{
    const size_t cols = (size_t)kColumns * padded;
    Carver c(base);
    const CorrSpace parts{.X = c.take<double>((size_t)N * padded),
                          .y = c.take<double>(cols),
                          .dy = c.take<double>(cols),
                          .dr = c.take<double>(cols),
                          .scratch = c.take<double>((size_t)kGeneralBlocks * kVectors * padded),
                          .lists = c.take<uint32_t>((size_t)(kColumns + 1) * padded),
                          .tab = c.take<CorrTables>(1)};
    if (sp) *sp = parts;
    return c.bytes();
}

__global__ __launch_bounds__(kBlock) void correlation_mass_kernel(const uint64_t *__restrict__ g_cells, const uint64_t *__restrict__ total,
                                                                  uint32_t num_samples, uint32_t num_branches, uint32_t padded,
                                                                  double *__restrict__ X)
{
    __shared__ double tile[kTile][kTile + 1];  // [sample][branch]
    const uint64_t stride = 2ull * num_branches + kTotals;
    const uint32_t across = (num_branches + kTile - 1) / kTile;
    const uint64_t tiles = (uint64_t)across * (padded / kTile);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint32_t b0 = (uint32_t)(t % across) * kTile, s0 = (uint32_t)(t / across) * kTile;
        for (uint32_t e = threadIdx.x; e < kTile * kTile; e += kBlock) {
            const uint32_t ls = e / kTile, lb = e % kTile, s = s0 + ls, b = b0 + lb;
            double v = 0.0;
            if (s < num_samples && b < num_branches) {
                const uint64_t T = total[s];
                if (T != 0) v = __ddiv_rn(__ull2double_rn(g_cells[s * stride + b]), __ull2double_rn(T));
            }
            tile[ls][lb] = v;
        }
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < kTile * kTile; e += kBlock) {
            const uint32_t lb = e / kTile, ls = e % kTile, b = b0 + lb;
            if (b < num_branches) X[(uint64_t)b * padded + s0 + ls] = tile[ls][lb];  // (s0 + ls < padded)
        }
        __syncthreads();  // (the tile is written again)
    }
}

// list `first_list + i`, i < num_lists: the used samples in ascending s, without those whose value in the group's column
// is missing; the list kAllUsed takes every used sample
__global__ __launch_bounds__(kWave) void correlation_lists_kernel(const uint64_t *__restrict__ total, const double *__restrict__ y,
                                                                  uint32_t num_samples, uint32_t padded, uint32_t first_list,
                                                                  uint32_t num_lists, uint32_t *__restrict__ lists,
                                                                  CorrTables *__restrict__ tab)
{
    if (threadIdx.x != 0) return;
    for (uint32_t i = blockIdx.x; i < num_lists; i += gridDim.x) {
        const uint32_t g = first_list + i;
        const double *col = g == kAllUsed ? nullptr : y + (uint64_t)tab->group_rep[g] * padded;
        uint32_t *list = lists + (uint64_t)g * padded;
        uint32_t L = 0;
        for (uint32_t s = 0; s < num_samples; ++s) {
            if (total[s] == 0) continue;
            if (col) {
                const double v = col[s];
                if (v != v) continue;  // missing
            }
            list[L++] = s;
        }
        tab->count[g] = L;
    }
}

__global__ __launch_bounds__(kBlock) void correlation_columns_kernel(const double *__restrict__ y, const uint32_t *__restrict__ lists,
                                                                     uint32_t num_columns, uint32_t padded, double *__restrict__ dy,
                                                                     double *__restrict__ dr, CorrTables *__restrict__ tab,
                                                                     uint32_t *__restrict__ used)
{
    for (uint32_t c = blockIdx.x; c < num_columns; c += gridDim.x) {
        const uint32_t g = tab->col_group[c], L = tab->count[g];
        const uint32_t *list = lists + (uint64_t)g * padded;
        const double *col = y + (uint64_t)c * padded;
        double *d = dy + (uint64_t)c * padded, *r = dr + (uint64_t)c * padded;
        for (uint32_t j = threadIdx.x; j < L; j += kBlock) d[j] = col[list[j]];
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < L; j += kBlock) r[j] = midrank(d, L, d[j]);
        __syncthreads();  // (every rank is formed from the values: they become deviations)
        if (threadIdx.x == 0) {
            used[c] = L;
            tab->stat[c][0] = L ? centre(d, L) : 0.0;
        }
        if (threadIdx.x == kWave) tab->stat[c][1] = L ? centre(r, L) : 0.0;
        __syncthreads();
    }
}

// kDisp: the dispersion of every branch over the list kAllUsed; else the correlations of every (branch, group of columns)
template <bool kLds, bool kDisp>
__global__ __launch_bounds__(kBlock) void correlation_branch_kernel(const double *__restrict__ X, const double *__restrict__ planes,
                                                                    const uint32_t *__restrict__ first,
                                                                    const uint32_t *__restrict__ lists, const double *__restrict__ dy,
                                                                    const double *__restrict__ dr, const CorrTables *__restrict__ tab,
                                                                    uint32_t num_branches, uint32_t padded,
                                                                    double *__restrict__ scratch, double *__restrict__ out)
{
    __shared__ double lds_vec[kLds ? kVectors * kLdsSamples : 1];
    __shared__ double res[kVectors * (kColumns + 1)];
    __shared__ double mean_of[kVectors];
    constexpr uint32_t nvec = kDisp ? 2 : kVectors;  // 0: xm, 1: xi, 2: rank(xm), 3: rank(xi)
    const uint32_t pitch = kLds ? kLdsSamples : padded;
    double *vec = kLds ? lds_vec : scratch + (uint64_t)blockIdx.x * kVectors * padded;
    const double *C = planes, *B = planes + (uint64_t)num_branches * padded;
    const uint32_t groups = kDisp ? 1 : tab->num_groups;
    const uint64_t units = (uint64_t)num_branches * groups;
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t b = (uint32_t)(unit % num_branches), g = kDisp ? kAllUsed : (uint32_t)(unit / num_branches);
        const uint32_t L = tab->count[g];
        const uint32_t *list = lists + (uint64_t)g * padded;
        const bool inner = first[b] < b;
        const uint32_t col0 = kDisp ? 0 : tab->group_start[g], nc = kDisp ? 0 : tab->group_start[g + 1] - col0;
        const uint32_t chains = nvec * (1 + nc);
        const bool defined = L >= (kDisp ? 1u : 3u);  // (uniform, as is every condition around a barrier below)
        if (defined) {
            const double *xrow = X + (uint64_t)b * padded, *crow = C + (uint64_t)b * padded, *brow = B + (uint64_t)b * padded;
            branch_vectors<kLds, !kDisp>(xrow, crow, brow, list, L, inner, vec, pitch);  // (cohort_device.hpp)
            if (threadIdx.x < nvec) {
                const double *v = vec + threadIdx.x * pitch;
                double acc = 0.0;
#pragma unroll 8  // (the reads of eight values are in flight ahead of the dependent adds)
                for (uint32_t j = 0; j < L; ++j) acc = __dadd_rn(acc, v[j]);
                mean_of[threadIdx.x] = __ddiv_rn(acc, (double)L);
            }
            __syncthreads();
            for (uint32_t e = threadIdx.x; e < chains; e += kBlock) {
                const uint32_t k = e % nvec, q = e / nvec;
                double acc = 0.0;
                if (inner || (k & 1) == 0) {
                    const double *v = vec + k * pitch;
                    const double mean = mean_of[k];
                    if (q == 0) {
#pragma unroll 8
                        for (uint32_t j = 0; j < L; ++j) {
                            const double dev = __dsub_rn(v[j], mean);
                            acc = __dadd_rn(acc, __dmul_rn(dev, dev));
                        }
                    } else {
                        const double *w = (k < 2 ? dy : dr) + (uint64_t)tab->group_cols[col0 + q - 1] * padded;
#pragma unroll 8
                        for (uint32_t j = 0; j < L; ++j) acc = __dadd_rn(acc, __dmul_rn(__dsub_rn(v[j], mean), w[j]));
                    }
                }
                res[e] = acc;
            }
            __syncthreads();
        }
        if (kDisp) {
            if (threadIdx.x < 2) {
                // lane 0: the five fields of the mass; lane 1: the three of the imbalance
                const uint32_t k = threadIdx.x;
                double mean = na_value(), var = na_value(), sd = na_value(), cv = na_value(), vmr = na_value();
                if (defined && (k == 0 || inner)) {
                    mean = mean_of[k], var = __ddiv_rn(res[k], (double)L), sd = __dsqrt_rn(var);
                    if (mean > 0.0) cv = __ddiv_rn(sd, mean), vmr = __ddiv_rn(var, mean);
                }
                double *record = out + (uint64_t)b * 8 + (k ? 5 : 0);
                record[0] = mean, record[1] = var, record[2] = sd;
                if (k == 0) record[3] = cv, record[4] = vmr;
            }
        } else {
            for (uint32_t e = threadIdx.x; e < chains; e += kBlock) {
                const uint32_t k = e % nvec, q = e / nvec;
                if (q == 0) continue;
                const uint32_t c = tab->group_cols[col0 + q - 1];
                double r = na_value();
                if (defined && (inner || (k & 1) == 0)) {
                    const double den = __dmul_rn(__dsqrt_rn(res[k]), __dsqrt_rn(tab->stat[c][k < 2 ? 0 : 1]));
                    if (den > 0.0) {
                        r = __ddiv_rn(res[e], den);
                        if (r < -1.0) r = -1.0;
                        if (r > 1.0) r = 1.0;
                    }
                }
                // xm, xi, rank(xm), rank(xi) -> mass_pearson, imbalance_pearson, mass_spearman, imbalance_spearman
                out[((uint64_t)c * num_branches + b) * 4 + (k & 1) * 2 + (k >> 1)] = r;
            }
        }
        __syncthreads();  // (the vectors, the means and the sums are written again)
    }
}

// the checks of epca_device, the device drained, T_s and the planes, the workspace, then xm as a plane
int correlation_begin(epik_amd_cohort *cohort, const epik_amd_tree *tree, hipStream_t stream, const uint32_t **d_first, CorrSpace *sp)
{
    COHORT_TRY(cohort_normalise_enqueue(cohort, tree, stream, d_first));
    const uint32_t N = cohort->num_branches, S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    COHORT_TRY(cohort_space_ensure(cohort, kSpaceCorrelation, correlation_space(nullptr, N, padded, nullptr)));
    correlation_space(cohort->space[kSpaceCorrelation].d, N, padded, sp);
    const uint64_t tiles = (uint64_t)((N + kTile - 1) / kTile) * (padded / kTile);
    hipLaunchKernelGGL(correlation_mass_kernel, cohort_grid(cohort, tiles, kManyBlocks), dim3(kBlock), 0, stream, cohort->d_cells,
                       cohort->d_total, S, N, padded, sp->X);
    return EPIK_AMD_OK;
}

template <bool kDisp>
void branch_launch(epik_amd_cohort *cohort, const CorrSpace &sp, const uint32_t *d_first, uint32_t groups, void *d_out, hipStream_t stream)
{
    const uint32_t N = cohort->num_branches, padded = cohort_padded_samples(cohort);
    const uint64_t units = (uint64_t)N * groups;
    if (lds_switch("EPIK_AMD_CORRELATION_LDS", cohort->num_samples, kLdsSamples))  // (=0, tests: the general path whatever S)
        hipLaunchKernelGGL((correlation_branch_kernel<true, kDisp>), cohort_grid(cohort, units, kManyBlocks), dim3(kBlock), 0, stream, sp.X,
                           cohort->d_planes, d_first, sp.lists, sp.dy, sp.dr, sp.tab, N, padded, sp.scratch,
                           static_cast<double *>(d_out));
    else
        hipLaunchKernelGGL((correlation_branch_kernel<false, kDisp>), cohort_grid(cohort, units, kGeneralBlocks), dim3(kBlock), 0, stream,
                           sp.X, cohort->d_planes, d_first, sp.lists, sp.dy, sp.dr, sp.tab, N, padded, sp.scratch,
                           static_cast<double *>(d_out));
}

int check_values(const double *meta, uint32_t num_samples, uint32_t num_columns)
{
    std::string err;
    return rule_result(correlation_columns_valid(meta, num_samples, num_columns, err), err);
}

int correlation_device_impl(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *meta, uint32_t M, void *d_out,
                            void *d_used, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(check_columns(M));
    COHORT_TRY(check_present(meta, d_out, d_used));
    const uint32_t S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    COHORT_TRY(check_values(meta, S, M));
    // the columns by sample, and their groups: columns with the same pattern of missing values have the same U_c
    std::vector<double> y((size_t)M * padded, 0.0);
    CorrTables tab{};
    std::map<std::vector<bool>, uint32_t> group_of;
    std::vector<std::vector<uint32_t>> members;
    for (uint32_t c = 0; c < M; ++c) {
        std::vector<bool> missing(S);
        for (uint32_t s = 0; s < S; ++s) {
            y[(size_t)c * padded + s] = meta[(size_t)s * M + c];
            missing[s] = std::isnan(meta[(size_t)s * M + c]);
        }
        const auto [it, fresh] = group_of.emplace(std::move(missing), (uint32_t)members.size());
        if (fresh) tab.group_rep[it->second] = c, members.emplace_back();
        tab.col_group[c] = it->second;
        members[it->second].push_back(c);
    }
    tab.num_groups = (uint32_t)members.size();
    for (uint32_t g = 0, at = 0; g < tab.num_groups; ++g) {
        tab.group_start[g] = at;
        for (const uint32_t c : members[g]) tab.group_cols[at++] = c;
        tab.group_start[g + 1] = at;
    }
    const uint32_t *d_first = nullptr;
    CorrSpace sp;
    COHORT_TRY(correlation_begin(cohort, tree, stream, &d_first, &sp));
    // (correlation_begin has drained the device of every call before: nothing reads the columns or the tables)
    HIP_TRY(hipMemcpy(sp.y, y.data(), y.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(sp.tab, &tab, sizeof tab, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(correlation_lists_kernel, cohort_grid(cohort, tab.num_groups, kColumns), dim3(kWave), 0, stream, cohort->d_total, sp.y,
                       S, padded, 0u, tab.num_groups, sp.lists, sp.tab);
    hipLaunchKernelGGL(correlation_columns_kernel, cohort_grid(cohort, M, kColumns), dim3(kBlock), 0, stream, sp.y, sp.lists, M, padded, sp.dy,
                       sp.dr, sp.tab, static_cast<uint32_t *>(d_used));
    branch_launch<false>(cohort, sp, d_first, tab.num_groups, d_out, stream);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

int dispersion_device_impl(epik_amd_cohort *cohort, const epik_amd_tree *tree, void *d_out, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(check_present(d_out));
    const uint32_t S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    const uint32_t *d_first = nullptr;
    CorrSpace sp;
    COHORT_TRY(correlation_begin(cohort, tree, stream, &d_first, &sp));
    hipLaunchKernelGGL(correlation_lists_kernel, dim3(1), dim3(kWave), 0, stream, cohort->d_total, sp.y, S, padded, kAllUsed, 1u,
                       sp.lists, sp.tab);
    branch_launch<true>(cohort, sp, d_first, 1, d_out, stream);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

}  // namespace

namespace epik_amd {

int cohort_mass_plane_enqueue(epik_amd_cohort *cohort, const epik_amd_tree *tree, hipStream_t stream, const uint32_t **d_first,
                              const double **d_X)
{
    CorrSpace sp;
    COHORT_TRY(correlation_begin(cohort, tree, stream, d_first, &sp));
    *d_X = sp.X;
    return EPIK_AMD_OK;
}

}  // namespace epik_amd

extern "C" {

int epik_amd_cohort_correlation_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *meta, uint32_t num_columns,
                                       void *d_out, void *d_used, void *stream)
{
    return guarded("cohort_correlation_device", [&]() -> int {
        return correlation_device_impl(cohort, tree, meta, num_columns, d_out, d_used, static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_correlation(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *meta, uint32_t num_columns,
                                epik_amd_correlation *out, uint32_t *used)
{
    return guarded("cohort_correlation", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(check_columns(num_columns));
        COHORT_TRY(check_present(meta, out, used));
        const size_t bytes = (size_t)num_columns * cohort->num_branches * sizeof(epik_amd_correlation);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult r, u;
        COHORT_TRY(r.alloc(bytes));
        COHORT_TRY(u.alloc(num_columns * sizeof(uint32_t)));
        COHORT_TRY(correlation_device_impl(cohort, tree, meta, num_columns, r.d, u.d, nullptr));
        COHORT_TRY(r.copy_to(out, bytes));
        return u.copy_to(used, num_columns * sizeof(uint32_t));
    });
}

int epik_amd_cohort_correlation_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                     const double *meta, uint32_t num_columns, epik_amd_correlation *out, uint32_t *used)
{
    return guarded("cohort_correlation_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(check_present(mass, first, meta, out, used));
        std::string err;
        return rule_result(correlation_records(mass, num_samples, num_branches, first, meta, num_columns, out, used, err), err);
    });
}

int epik_amd_cohort_dispersion_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, void *d_out, void *stream)
{
    return guarded("cohort_dispersion_device", [&]() -> int { return dispersion_device_impl(cohort, tree, d_out, static_cast<hipStream_t>(stream)); });
}

int epik_amd_cohort_dispersion(epik_amd_cohort *cohort, const epik_amd_tree *tree, epik_amd_dispersion *out)
{
    return guarded("cohort_dispersion", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(check_present(out));
        const size_t bytes = (size_t)cohort->num_branches * sizeof(epik_amd_dispersion);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult r;
        COHORT_TRY(r.alloc(bytes));
        COHORT_TRY(dispersion_device_impl(cohort, tree, r.d, nullptr));
        return r.copy_to(out, bytes);
    });
}

int epik_amd_cohort_dispersion_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                    epik_amd_dispersion *out)
{
    return guarded("cohort_dispersion_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(check_present(mass, first, out));
        std::string err;
        return rule_result(dispersion_records(mass, num_samples, num_branches, first, out, err), err);
    });
}

}  // extern "C"
