// model_place.hip -- the sequential distance-based linear model (McArdle & Anderson 2001; `adonis2`, by = "terms") of a
// cohort's samples over their distances on the device: do the samples still differ by a term once the terms before it are
// accounted for?  epik_amd_cohort_model_device / _model / _model_metric / _model_host / _model_metric_host / _model_kr_host
// (include/epik_amd.h).
//
// No reference counterpart.  The rule is stated once, in include/epik_amd.h beside the PERMDISP rule (DESIGN.md 3.21;
// epik_amd/host/cohort.cpp: model_records_of_kr is the same rule on the CPU).  Every sum is a sequential chain from +0.0 in
// one lane (__dadd_rn / __dsub_rn / __dmul_rn / __ddiv_rn / __dsqrt_rn; the file is built with -ffp-contract=off as well).  No
// MFMA: the chains have a fixed order.  NA is stored as its bit pattern and never computed.
//
//   (model_terms_kernel, model_basis_kernel and model_strata_kernel are in model_basis.hpp, which the edge model shares)
//   model_terms_kernel   a wave a term: the complete cases with mass in list order (the host has set the label of every term
//                        to `missing` for a sample that lacks any value, so every term sees the same list) and the groups of
//                        a factor by first appearance: column_list of cohort_device.hpp, PERMANOVA's.
//   model_rows_kernel, model_total_kernel, model_centre_kernel
//                        the Gower matrix B[L][L] over the list exactly as pcoa_place.hip forms it (gower_centred is the
//                        shared element), and ss_total, the chain of its diagonal, in one lane.
//   model_basis_kernel   one workgroup: a column at a time, centred, then classical Gram-Schmidt twice: a lane a k for the
//                        chains h_k (Q is [L][64], so the lanes read a line), a lane an i for the update, one lane for the mean,
//                        n0 and n1.  Q, df, the aliased bytes and df_res.
//   model_ss_kernel      the hot kernel, a workgroup a batch of kPerms permutations.  A lane owns row i and keeps
//                        kPerms x kCols chains t_c in registers; for j ascending it reads B[j][i] (a coalesced line, and B[i][j]:
//                        B is symmetric bit for bit) and multiplies it into the rows Q[sigma_p(j)][c0 .. c0 + kCols), the same
//                        address for the whole wave (the arrangement is read through readfirstlane: uniform loads).  One read of
//                        B feeds kPerms x kCols chains; a design of more than kCols accepted columns takes a pass over B for
//                        every kCols of them.  Then a lane a (permutation, column): the chain s_c over t, which sits in LDS up to
//                        kLdsPositions samples and in the workgroup's slice of global memory beyond (or with
//                        EPIK_AMD_MODEL_LDS=0): the same code on other pointers.  Then a lane a permutation: SS_k and SS_model;
//                        and a lane a term: F of every permutation and one vector atomic for the unit's count.  sigma_p is
//                        permutation_rank of cohort_device.hpp.  Launched twice: the identity alone, which writes the records,
//                        the info block and F_0; then the permutations 1 .. P.
//   model_finish_kernel  p = (1 + at_least) / (P + 1), and NA into the rows of stat whose test is undefined.
//   model_strata_kernel  with strata only (the strata rule): the tables of the list of the complete cases; the
//                        permutations' model_ss_kernel<.., kStrata = true> then takes sigma_p from permutation_arrangement.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"
#include "model_basis.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kTerms = kModelTerms, kColumns = kModelColumns, kPitch = kModelPitch;
constexpr uint32_t kPerms = 4;             // the permutations a workgroup carries through one pass over B
constexpr uint32_t kChunk = 8;             // the columns a lane accumulates at a time: kPerms * kChunk chains in registers
constexpr uint32_t kSmallColumns = 4;      // a design of up to here columns accumulates kSmallColumns at a time instead
constexpr uint32_t kLdsPositions = 128;    // the most samples whose row sums and arrangements stay in LDS (34 KiB)
constexpr uint32_t kGeneralBlocks = 256;   // workgroups of the general path: each has a slice
constexpr uint64_t kManyBlocks = 65536;

static_assert(sizeof(epik_amd_model_term) == 48 && sizeof(epik_amd_model_info) == 40, "the records are 48 and 40 bytes");
static_assert(kBlock == 256 && kWave == 64 && kColumns % kChunk == 0 && kChunk % kSmallColumns == 0);
static_assert(kPerms * (kTerms + 1) <= kBlock && kPerms * kChunk <= kBlock && kColumns <= kBlock);

struct ModelSpace {
    double *B;        // [S][S]: the Gower matrix, L x L compact
    double *Q;        // [Sp][kPitch]: the basis, a position a row
    double *r, *v;    // [Sp]: the row means; the column at work
    double *val;      // [T][Sp]: the values by sample
    double *scratch;  // [slices] x (t[kPerms][kChunk][Sp] | sigma[kPerms][Sp]): a slice a workgroup of the general path, none on the LDS path
    ModelMeta *meta;
    uint32_t *lab;    // [T][Sp]: the labels by sample, `missing` for a sample that is no complete case
    uint32_t *idx;    // [T][Sp]: the samples of the positions (every term's list is the same)
    uint8_t *lam;     // [T][Sp]: the groups of the positions
    uint32_t *strata;  // with strata only: [Sp], the strata by sample
    uint32_t *hs, *home;  // ... and [Sp]: the strata of the positions, and the positions by (stratum, position)
};

constexpr size_t kSliceBytes = kPerms * kChunk * 8 + kPerms * 4;  // the bytes of a slice per padded sample

size_t model_space(void *base, uint32_t S, uint32_t padded, uint32_t T, uint32_t slices, bool strata, ModelSpace *sp)
{
    Carver c(base);
    const ModelSpace parts{.B = c.take<double>((size_t)S * S),
                           .Q = c.take<double>((size_t)padded * kPitch),
                           .r = c.take<double>(padded),
                           .v = c.take<double>(padded),
                           .val = c.take<double>((size_t)T * padded),
                           .scratch = c.take<double>((size_t)slices * kSliceBytes * padded / sizeof(double)),
                           .meta = c.take<ModelMeta>(1),
                           .lab = c.take<uint32_t>((size_t)T * padded),
                           .idx = c.take<uint32_t>((size_t)T * padded),
                           .lam = c.take<uint8_t>((size_t)T * padded),
                           .strata = c.take<uint32_t>(strata ? padded : 0),
                           .hs = c.take<uint32_t>(strata ? padded : 0),
                           .home = c.take<uint32_t>(strata ? padded : 0)};
    if (sp) *sp = parts;
    return c.bytes();
}

__global__ __launch_bounds__(kBlock) void model_rows_kernel(const double *__restrict__ kr, const uint32_t *__restrict__ used,
                                                            uint32_t num_samples, const ModelMeta *__restrict__ meta,
                                                            double *__restrict__ r)
{
    const uint32_t L = meta->L;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < L; i += gridDim.x * kBlock) r[i] = gower_row_mean(kr, used, num_samples, L, i);
}

__global__ __launch_bounds__(kWave) void model_total_kernel(const double *__restrict__ kr, const uint32_t *__restrict__ used,
                                                            uint32_t num_samples, ModelMeta *__restrict__ meta,
                                                            const double *__restrict__ r)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint32_t L = meta->L;
    const double g = gower_mean_of_means(r, L);
    double total = 0.0;
    for (uint32_t j = 0; j < L; ++j) {
        const uint32_t s = used[j];
        total = __dadd_rn(total, gower_centred(kr[(uint64_t)s * num_samples + s], r[j], r[j], g));
    }
    meta->g = g, meta->ss_total = total;
}

__global__ __launch_bounds__(kBlock) void model_centre_kernel(const double *__restrict__ kr, const uint32_t *__restrict__ used,
                                                              uint32_t num_samples, const ModelMeta *__restrict__ meta,
                                                              const double *__restrict__ r, double *__restrict__ B)
{
    gower_centre_cells(kr, used, num_samples, meta->L, r, meta->g, B);
}

struct SsArgs {
    const double *B, *Q;
    ModelMeta *meta;
    double *scratch;
    epik_amd_model_term *out;
    epik_amd_model_info *info;
    double *stat;  // or null
    uint64_t seed;
    uint32_t num_terms, num_permutations, pitch;
    const uint32_t *hs, *home;  // the strata rule's tables, or null
};

// F of a term from its sums: the rule's three divisions, +infinity where the residual is not > 0
__device__ inline double f_of(double ss, uint32_t df, double res, int64_t df_res)
{
    if (!(res > 0.0)) return HUGE_VAL;
    return __ddiv_rn(__ddiv_rn(ss, (double)df), __ddiv_rn(res, (double)df_res));
}

// kObserved: the identity alone, and the records; else the permutations 1 .. P, kPerms a unit.  kCols: the chains of a
// permutation that a lane keeps at a time.
template <bool kLds, bool kObserved, uint32_t kCols, bool kStrata>
__global__ __launch_bounds__(kBlock) void model_ss_kernel(const SsArgs a)
{
    extern __shared__ __align__(16) unsigned char dynamic_lds[];
    __shared__ uint64_t tile[kCohortKeyTile];
    __shared__ double s_of[kPerms][kColumns];     // s_c of permutation k
    __shared__ double ss_of[kPerms][kTerms + 1];  // SS_k of permutation k, SS_model last
    __shared__ ModelMeta m;
    const uint32_t tid = threadIdx.x, pitch = a.pitch, T = a.num_terms, P = a.num_permutations;
    if (tid == 0) m = *a.meta;
    __syncthreads();
    const uint32_t L = m.L, R = m.R;
    if (!kObserved && (!m.testable || R == 0)) return;  // (uniform: no F is defined)
    double *t;
    uint32_t *sigma;
    if (kLds) {
        t = reinterpret_cast<double *>(dynamic_lds);
    } else {
        // (kSliceBytes * pitch bytes a slice, pitch % 32 == 0: every slice is aligned)
        t = reinterpret_cast<double *>(reinterpret_cast<char *>(a.scratch) + (uint64_t)blockIdx.x * kSliceBytes * pitch);
    }
    sigma = reinterpret_cast<uint32_t *>(t + (uint64_t)kPerms * kChunk * pitch);
    const uint32_t units = kObserved ? 1 : (P + kPerms - 1) / kPerms;
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t p0 = kObserved ? 0 : 1 + unit * kPerms, np = kObserved ? 1 : min(kPerms, P + 1 - p0);
        for (uint32_t k = 0; k < kPerms; ++k) {
            const uint32_t p = k < np ? p0 + k : 0;  // (beyond np: filling, the identity)
            for (uint32_t base = 0; base < L; base += kBlock) {  // (every lane calls: it has barriers)
                const uint32_t i = base + tid;
                uint32_t rank;
                if constexpr (kStrata && !kObserved) {
                    __shared__ uint32_t htile[kCohortKeyTile];
                    rank = permutation_arrangement(a.seed, p, i, L, tile, htile, a.hs, a.home);
                } else {
                    rank = permutation_rank(a.seed, p, i, L, tile);
                }
                if (i < L) sigma[k * pitch + i] = rank;
            }
        }
        __syncthreads();
        for (uint32_t c0 = 0; c0 < R; c0 += kCols) {
            for (uint32_t i = tid; i < L; i += kBlock) {
                double acc[kPerms][kCols];
#pragma unroll
                for (uint32_t k = 0; k < kPerms; ++k)
#pragma unroll
                    for (uint32_t c = 0; c < kCols; ++c) acc[k][c] = 0.0;
                const double *column = a.B + i;  // B[j][i] = B[i][j]
                for (uint32_t j = 0; j < L; ++j) {  // ascending: the rule's order
                    const double b = column[(uint64_t)j * L];
#pragma unroll
                    for (uint32_t k = 0; k < kPerms; ++k) {
                        const uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)sigma[k * pitch + j]);  // (the wave shares j)
                        const double *row = a.Q + (uint64_t)at * kPitch + c0;
#pragma unroll
                        for (uint32_t c = 0; c < kCols; ++c) acc[k][c] = __dadd_rn(acc[k][c], __dmul_rn(b, row[c]));
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < kPerms; ++k)
#pragma unroll
                    for (uint32_t c = 0; c < kCols; ++c) t[(uint64_t)(k * kCols + c) * pitch + i] = acc[k][c];
            }
            __syncthreads();
            for (uint32_t e = tid; e < kPerms * kCols; e += kBlock) {
                const uint32_t k = e / kCols, c = e % kCols;
                if (c0 + c >= R) continue;
                const double *tk = t + (uint64_t)e * pitch;
                const uint32_t *sk = sigma + k * pitch;
                double s = 0.0;
#pragma unroll 4
                for (uint32_t i = 0; i < L; ++i) s = __dadd_rn(s, __dmul_rn(a.Q[(uint64_t)sk[i] * kPitch + c0 + c], tk[i]));
                s_of[k][c0 + c] = s;
            }
            __syncthreads();  // (t is written again)
        }
        if (tid < kPerms) {
            double model = 0.0;
            for (uint32_t term = 0; term < T; ++term) {
                double ss = 0.0;
                for (uint32_t w = 0; w < m.df[term]; ++w) ss = __dadd_rn(ss, s_of[tid][m.first[term] + w]);
                ss_of[tid][term] = ss;
                model = __dadd_rn(model, ss);
            }
            ss_of[tid][T] = model;
        }
        __syncthreads();
        if (kObserved) {
            if (tid == 0) {
                const double ss_res = __dsub_rn(m.ss_total, ss_of[0][T]);
                const bool testable = m.df_res >= 1 && ss_res > 0.0;
                a.meta->ss_res = ss_res, a.meta->testable = testable;
                *a.info = epik_amd_model_info{L, T, m.C, R, m.df_res, m.ss_total, ss_res};
                for (uint32_t term = 0; term <= T; ++term) {
                    epik_amd_model_term rec{m.df[term], m.columns[term], 0, na_value(), na_value(), na_value(), na_value()};
                    double f0 = na_value();
                    if (rec.df) {
                        rec.ss = ss_of[0][term];
                        if (m.ss_total > 0.0) rec.r2 = __ddiv_rn(rec.ss, m.ss_total);
                        if (testable) rec.f = f0 = f_of(rec.ss, rec.df, ss_res, m.df_res);
                        if (testable && a.stat) a.stat[(uint64_t)term * (P + 1)] = f0;
                    }
                    a.out[term] = rec, a.meta->f0[term] = f0;
                }
            }
        } else if (tid <= T && m.df[tid]) {
            unsigned long long count = 0;
            for (uint32_t k = 0; k < np; ++k) {
                const double f = f_of(ss_of[k][tid], m.df[tid], __dsub_rn(m.ss_total, ss_of[k][T]), m.df_res);
                if (a.stat) a.stat[(uint64_t)tid * (P + 1) + p0 + k] = f;
                count += f >= m.f0[tid];
            }
            if (count) atomicAdd(reinterpret_cast<unsigned long long *>(&a.out[tid].at_least), count);
        }
        __syncthreads();  // (the arrangements and the sums are written again)
    }
}

__global__ __launch_bounds__(kBlock) void model_finish_kernel(const ModelMeta *__restrict__ meta, uint32_t num_terms,
                                                              uint32_t num_permutations, epik_amd_model_term *__restrict__ out,
                                                              double *__restrict__ stat)
{
    const uint64_t first = (uint64_t)blockIdx.x * kBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kBlock;
    const bool testable = meta->testable != 0;
    for (uint64_t term = first; term <= num_terms; term += stride)
        if (testable && meta->df[term])
            out[term].p = __ddiv_rn((double)(1 + out[term].at_least), (double)(num_permutations + 1));
    if (!stat) return;
    const uint64_t row = (uint64_t)num_permutations + 1;
    for (uint64_t e = first; e < (num_terms + 1) * row; e += stride)
        if (!(testable && meta->df[e / row])) stat[e] = na_value();
}

int check_arguments(const uint32_t *kind, const uint32_t *labels, const double *values, uint32_t S, uint32_t T, uint32_t P)
{
    std::string err;
    return rule_result(model_arguments_valid(kind, labels, values, S, T, P, err), err);
}

int terms_valid(uint32_t T)
{
    if (T < 1 || T > kTerms) return fail_with(EPIK_AMD_ERR_INVALID, "num_terms = " + std::to_string(T) + " is outside [1, 16]");
    return EPIK_AMD_OK;
}

template <bool kLds, uint32_t kCols>
void launch_ss(const epik_amd_cohort *cohort, const SsArgs &args, size_t dynamic, hipStream_t stream)
{
    const uint64_t units = (args.num_permutations + kPerms - 1) / kPerms, most = kLds ? kManyBlocks : kGeneralBlocks;
    const dim3 grid = cohort_grid(cohort, units, most);
    hipLaunchKernelGGL((model_ss_kernel<kLds, true, kCols, false>), dim3(1), dim3(kBlock), dynamic, stream, args);  // (the identity)
    if (args.hs) hipLaunchKernelGGL((model_ss_kernel<kLds, false, kCols, true>), grid, dim3(kBlock), dynamic, stream, args);
    else hipLaunchKernelGGL((model_ss_kernel<kLds, false, kCols, false>), grid, dim3(kBlock), dynamic, stream, args);
}

int model_device_impl(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *kind, const uint32_t *labels, const double *values,
                      const uint32_t *strata, uint32_t T, uint32_t P, uint64_t seed, void *d_out, void *d_info, void *d_stat,
                      void *d_aliased, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(terms_valid(T));
    COHORT_TRY(check_present(d_kr, kind, labels, values, d_out, d_info, d_aliased));
    const uint32_t S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    COHORT_TRY(check_arguments(kind, labels, values, S, T, P));
    COHORT_TRY(check_has_distances(cohort));
    HIP_TRY(hipSetDevice(cohort->device));
    HIP_TRY(hipDeviceSynchronize());  // (the distances enqueued on whatever stream, and an earlier call that reads the workspace)
    const bool lds = lds_switch("EPIK_AMD_MODEL_LDS", S, kLdsPositions);  // (=0, tests: the general path whatever S)
    // the general path's workgroups, each with a slice: the grid that launch_ss makes of the permutations' units
    const uint32_t slices = lds ? 0 : cohort_grid(cohort, (P + kPerms - 1) / kPerms, kGeneralBlocks).x;
    COHORT_TRY(cohort_space_ensure(cohort, kSpaceModel, model_space(nullptr, S, padded, T, slices, strata != nullptr, nullptr)));
    ModelSpace sp;
    model_space(cohort->space[kSpaceModel].d, S, padded, T, slices, strata != nullptr, &sp);
    if (strata) COHORT_TRY(upload_strata(strata, S, padded, sp.strata));
    // the design by term, every term listing the complete cases (model_basis.hpp)
    ModelKinds kinds{};
    size_t bound = 0;  // the columns as the rule counts them: at least those of the used samples
    COHORT_TRY(model_design_upload(kind, labels, values, S, T, padded, sp.lab, sp.val, kinds, bound));
    HIP_TRY(hipMemsetAsync(sp.meta, 0, sizeof(ModelMeta), stream));
    HIP_TRY(hipMemsetAsync(sp.Q, 0, (size_t)padded * kPitch * sizeof(double), stream));  // (a lane reads whole chunks of a row)
    const auto *kr = static_cast<const double *>(d_kr);
    const uint64_t cells = (uint64_t)S * S;
    hipLaunchKernelGGL(model_terms_kernel, cohort_grid(cohort, T, kTerms), dim3(kWave), 0, stream, cohort->d_total, sp.lab, S, padded, T, sp.idx,
                       sp.lam, sp.meta);
    if (strata) hipLaunchKernelGGL(model_strata_kernel, dim3(1), dim3(kBlock), 0, stream, sp.strata, sp.idx, sp.meta, sp.hs, sp.home);
    hipLaunchKernelGGL(model_rows_kernel, cohort_grid(cohort, (S + kBlock - 1) / kBlock, kManyBlocks), dim3(kBlock), 0, stream, kr, sp.idx, S,
                       sp.meta, sp.r);
    hipLaunchKernelGGL(model_total_kernel, dim3(1), dim3(kWave), 0, stream, kr, sp.idx, S, sp.meta, sp.r);
    hipLaunchKernelGGL(model_centre_kernel, cohort_grid(cohort, (cells + kBlock - 1) / kBlock, kManyBlocks), dim3(kBlock), 0, stream, kr, sp.idx,
                       S, sp.meta, sp.r, sp.B);
    hipLaunchKernelGGL(model_basis_kernel, dim3(1), dim3(kBlock), 0, stream, kinds, T, padded, sp.val, sp.idx, sp.lam, sp.v, sp.Q, sp.meta,
                       static_cast<uint8_t *>(d_aliased));
    const uint32_t pitch = lds ? kLdsPositions : padded;
    const SsArgs args{sp.B, sp.Q, sp.meta, sp.scratch, static_cast<epik_amd_model_term *>(d_out),
                      static_cast<epik_amd_model_info *>(d_info), static_cast<double *>(d_stat), seed, T, P, pitch,
                      strata ? sp.hs : nullptr, strata ? sp.home : nullptr};
    const size_t dynamic = lds ? kSliceBytes * pitch : 0;
    const bool small = bound <= kSmallColumns;
    if (lds && small) launch_ss<true, kSmallColumns>(cohort, args, dynamic, stream);
    else if (lds) launch_ss<true, kChunk>(cohort, args, dynamic, stream);
    else if (small) launch_ss<false, kSmallColumns>(cohort, args, dynamic, stream);
    else launch_ss<false, kChunk>(cohort, args, dynamic, stream);
    const uint64_t finish = d_stat ? (uint64_t)(T + 1) * (P + 1) : T + 1;
    hipLaunchKernelGGL(model_finish_kernel, cohort_grid(cohort, (finish + kBlock - 1) / kBlock, kManyBlocks), dim3(kBlock), 0, stream, sp.meta,
                       T, P, static_cast<epik_amd_model_term *>(d_out), static_cast<double *>(d_stat));
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

}  // namespace

extern "C" {

int epik_amd_cohort_model_device(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *kind, const uint32_t *labels,
                                 const double *values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed, void *d_out,
                                 void *d_info, void *d_stat, void *d_aliased, void *stream)
{
    return epik_amd_cohort_model_strata_device(cohort, d_kr, kind, labels, values, num_terms, num_permutations, seed, d_out, d_info, d_stat,
                                               d_aliased, stream, nullptr);
}

int epik_amd_cohort_model_strata_device(epik_amd_cohort *cohort, const void *d_kr, const uint32_t *kind, const uint32_t *labels,
                                        const double *values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed, void *d_out,
                                        void *d_info, void *d_stat, void *d_aliased, void *stream, const uint32_t *strata)
{
    return guarded("cohort_model_device", [&]() -> int {
        return model_device_impl(cohort, d_kr, kind, labels, values, strata, num_terms, num_permutations, seed, d_out, d_info, d_stat,
                                 d_aliased, static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_model(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, const uint32_t *kind,
                          const uint32_t *labels, const double *values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed,
                          epik_amd_model_term *out, epik_amd_model_info *info, double *stat, uint8_t *aliased)
{
    return epik_amd_cohort_model_metric(cohort, tree, branch_length, EPIK_AMD_DISTANCE_KR, kind, labels, values, num_terms,
                                        num_permutations, seed, out, info, stat, aliased);
}

int epik_amd_cohort_model_metric(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                                 const uint32_t *kind, const uint32_t *labels, const double *values, uint32_t num_terms,
                                 uint32_t num_permutations, uint64_t seed, epik_amd_model_term *out, epik_amd_model_info *info,
                                 double *stat, uint8_t *aliased)
{
    return epik_amd_cohort_model_strata(cohort, tree, branch_length, metric, kind, labels, values, num_terms, num_permutations, seed, out,
                                        info, stat, aliased, nullptr);
}

int epik_amd_cohort_model_strata(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                                 const uint32_t *kind, const uint32_t *labels, const double *values, uint32_t num_terms,
                                 uint32_t num_permutations, uint64_t seed, epik_amd_model_term *out, epik_amd_model_info *info,
                                 double *stat, uint8_t *aliased, const uint32_t *strata)
{
    return guarded("cohort_model", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(terms_valid(num_terms));
        COHORT_TRY(check_present(kind, labels, values, out, info, aliased));
        const uint32_t S = cohort->num_samples;
        COHORT_TRY(check_arguments(kind, labels, values, S, num_terms, num_permutations));
        const size_t out_bytes = ((size_t)num_terms + 1) * sizeof(epik_amd_model_term);
        const size_t stat_bytes = ((size_t)num_terms + 1) * ((size_t)num_permutations + 1) * sizeof(double);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult kr, r, s;
        COHORT_TRY(kr.alloc((size_t)S * S * sizeof(double)));
        COHORT_TRY(r.alloc(out_bytes + sizeof(epik_amd_model_info) + kColumns));  // the records | the info block | aliased
        COHORT_TRY(s.alloc(stat_bytes, stat != nullptr));
        COHORT_TRY(cohort_distance_enqueue(cohort, tree, branch_length, metric, kr.d, nullptr));
        COHORT_TRY(model_device_impl(cohort, kr.d, kind, labels, values, strata, num_terms, num_permutations, seed, r.d, r.at(out_bytes),
                                     s.d, r.at(out_bytes + sizeof(epik_amd_model_info)), nullptr));
        COHORT_TRY(r.copy_to(out, out_bytes));
        COHORT_TRY(r.copy_to(info, sizeof *info, out_bytes));
        COHORT_TRY(r.copy_to(aliased, kColumns, out_bytes + sizeof *info));
        return s.copy_to(stat, stat_bytes);
    });
}

int epik_amd_cohort_model_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                               const double *branch_length, const uint32_t *kind, const uint32_t *labels, const double *values,
                               uint32_t num_terms, uint32_t num_permutations, uint64_t seed, epik_amd_model_term *out,
                               epik_amd_model_info *info, double *stat, uint8_t *aliased)
{
    return epik_amd_cohort_model_metric_host(mass, num_samples, num_branches, first, branch_length, EPIK_AMD_DISTANCE_KR, kind, labels,
                                             values, num_terms, num_permutations, seed, out, info, stat, aliased);
}

int epik_amd_cohort_model_metric_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                      const double *branch_length, uint32_t metric, const uint32_t *kind, const uint32_t *labels,
                                      const double *values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed,
                                      epik_amd_model_term *out, epik_amd_model_info *info, double *stat, uint8_t *aliased)
{
    return epik_amd_cohort_model_strata_host(mass, num_samples, num_branches, first, branch_length, metric, kind, labels, values, num_terms,
                                             num_permutations, seed, out, info, stat, aliased, nullptr);
}

int epik_amd_cohort_model_strata_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                      const double *branch_length, uint32_t metric, const uint32_t *kind, const uint32_t *labels,
                                      const double *values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed,
                                      epik_amd_model_term *out, epik_amd_model_info *info, double *stat, uint8_t *aliased,
                                      const uint32_t *strata)
{
    return guarded("cohort_model_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(terms_valid(num_terms));
        COHORT_TRY(check_present(mass, first, branch_length, kind, labels, values, out, info, aliased));
        std::string err;
        return rule_result(model_records(mass, num_samples, num_branches, first, branch_length, kind, labels, values, num_terms,
                                         num_permutations, seed, out, info, stat, aliased, err, metric, strata),
                           err);
    });
}

int epik_amd_cohort_model_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const uint32_t *kind,
                                  const uint32_t *labels, const double *values, uint32_t num_terms, uint32_t num_permutations,
                                  uint64_t seed, epik_amd_model_term *out, epik_amd_model_info *info, double *stat, uint8_t *aliased)
{
    return epik_amd_cohort_model_strata_kr_host(kr, totals, num_samples, kind, labels, values, num_terms, num_permutations, seed, out, info,
                                                stat, aliased, nullptr);
}

int epik_amd_cohort_model_strata_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, const uint32_t *kind,
                                         const uint32_t *labels, const double *values, uint32_t num_terms, uint32_t num_permutations,
                                         uint64_t seed, epik_amd_model_term *out, epik_amd_model_info *info, double *stat,
                                         uint8_t *aliased, const uint32_t *strata)
{
    return guarded("cohort_model_kr_host", [&]() -> int {
        COHORT_TRY(check_host_samples(num_samples));
        COHORT_TRY(terms_valid(num_terms));
        COHORT_TRY(check_present(kr, totals, kind, labels, values, out, info, aliased));
        std::string err;
        return rule_result(model_records_of_kr(kr, totals, num_samples, kind, labels, values, num_terms, num_permutations, seed, out, info,
                                               stat, aliased, err, strata),
                           err);
    });
}

}  // extern "C"
