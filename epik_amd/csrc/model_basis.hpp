// model_basis.hpp -- what the sequential model (model_place.hip) and the edge model (edgemodel_place.hip) share of a design: the
// steps 1, 3 and 4 of the model's rule (include/epik_amd.h), none of which depends on the response.  The design by term on the
// device, the list of the complete cases, the centred columns and the basis Q by classical Gram-Schmidt twice, with df, R,
// df_res and the aliased bytes; and the strata rule's tables of that list.  A file that includes it gets kernels of its own.
#ifndef EPIK_AMD_MODEL_BASIS_HPP
#define EPIK_AMD_MODEL_BASIS_HPP

#include <hip/hip_runtime.h>

#include <cmath>
#include <set>
#include <vector>

#include "cohort_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kModelTerms = EPIK_AMD_MODEL_MAX_TERMS;
constexpr uint32_t kModelColumns = EPIK_AMD_MODEL_MAX_COLUMNS;
constexpr uint32_t kModelGroups = EPIK_AMD_MODEL_MAX_GROUPS;
constexpr uint32_t kModelMissing = EPIK_AMD_MODEL_MISSING;
constexpr uint32_t kModelPitch = kModelColumns;  // doubles a row of Q

// what the kernels hand on to one another, in the workspace
struct ModelMeta {
    uint32_t L, C, R, testable;
    int64_t df_res;
    double g, ss_total, ss_res;
    uint32_t groups[kModelTerms];
    uint32_t df[kModelTerms + 1], columns[kModelTerms + 1], first[kModelTerms + 1];  // of a term, and of the whole model; first: its first accepted column
    double f0[kModelTerms + 1];
};

struct ModelKinds {
    uint32_t kind[kModelTerms];
};

__global__ __launch_bounds__(kWave) void model_terms_kernel(const uint64_t *__restrict__ total, const uint32_t *__restrict__ lab,
                                                            uint32_t num_samples, uint32_t padded, uint32_t num_terms,
                                                            uint32_t *__restrict__ idx, uint8_t *__restrict__ lam,
                                                            ModelMeta *__restrict__ meta)
{
    __shared__ uint32_t group_of[kModelGroups], size[kModelGroups];
    for (uint32_t t = blockIdx.x; t < num_terms; t += gridDim.x) {
        const uint64_t offset = (uint64_t)t * padded;
        uint32_t L, G;  // (uniform)
        column_list<kModelGroups>(total, lab + offset, num_samples, kModelMissing, group_of, size, idx + offset, lam + offset, L, G);
        if (threadIdx.x == 0) {
            meta->groups[t] = G;
            if (t == 0) meta->L = L;
        }
        __syncthreads();  // (the tables are written again)
    }
}

// one workgroup; every condition around a barrier is uniform (L, G, R and the acceptance come from shared memory)
__global__ __launch_bounds__(kBlock) void model_basis_kernel(const ModelKinds kinds, uint32_t num_terms, uint32_t padded,
                                                             const double *__restrict__ val, const uint32_t *__restrict__ idx,
                                                             const uint8_t *__restrict__ lam, double *v, double *Q,
                                                             ModelMeta *meta, uint8_t *__restrict__ aliased)
{
    __shared__ double h[kModelColumns];
    __shared__ double mean_of, root_of;
    __shared__ uint32_t accepted;
    const uint32_t tid = threadIdx.x, L = meta->L;
    uint32_t C = 0, R = 0;
    for (uint32_t t = 0; t < num_terms; ++t) {
        const bool numeric = kinds.kind[t] != 0;
        const uint32_t G = meta->groups[t], width = numeric ? 1 : G ? G - 1 : 0, first = R;
        const uint64_t offset = (uint64_t)t * padded;
        for (uint32_t w = 0; w < width; ++w, ++C) {
            for (uint32_t i = tid; i < L; i += kBlock) v[i] = numeric ? val[offset + idx[i]] : lam[offset + i] == w + 1 ? 1.0 : 0.0;
            __syncthreads();
            if (tid == 0 && L) {
                double acc = 0.0;
#pragma unroll 4
                for (uint32_t i = 0; i < L; ++i) acc = __dadd_rn(acc, v[i]);
                mean_of = __ddiv_rn(acc, (double)L);
            }
            __syncthreads();
            for (uint32_t i = tid; i < L; i += kBlock) v[i] = __dsub_rn(v[i], mean_of);
            __syncthreads();
            double n0 = 0.0;  // (lane 0's)
            if (tid == 0) {
#pragma unroll 4
                for (uint32_t i = 0; i < L; ++i) n0 = __dadd_rn(n0, __dmul_rn(v[i], v[i]));
            }
            for (uint32_t pass = 0; pass < 2; ++pass) {
                for (uint32_t k = tid; k < R; k += kBlock) {
                    double acc = 0.0;
#pragma unroll 4
                    for (uint32_t i = 0; i < L; ++i) acc = __dadd_rn(acc, __dmul_rn(Q[(uint64_t)i * kModelPitch + k], v[i]));
                    h[k] = acc;
                }
                __syncthreads();
                for (uint32_t i = tid; i < L; i += kBlock) {
                    const double *row = Q + (uint64_t)i * kModelPitch;
                    double x = v[i];
                    for (uint32_t k = 0; k < R; ++k) x = __dsub_rn(x, __dmul_rn(h[k], row[k]));
                    v[i] = x;
                }
                __syncthreads();
            }
            if (tid == 0) {
                double n1 = 0.0;
#pragma unroll 4
                for (uint32_t i = 0; i < L; ++i) n1 = __dadd_rn(n1, __dmul_rn(v[i], v[i]));
                const bool accept = n0 > 0.0 && n1 > __dmul_rn(0x1p-40, n0);
                accepted = accept, root_of = accept ? __dsqrt_rn(n1) : 0.0;
                aliased[C] = accept ? 0 : 1;
            }
            __syncthreads();
            if (accepted) {
                for (uint32_t i = tid; i < L; i += kBlock) Q[(uint64_t)i * kModelPitch + R] = __ddiv_rn(v[i], root_of);
                ++R;
            }
            __syncthreads();  // (v, the acceptance and Q are complete before the next column)
        }
        if (tid == 0) meta->df[t] = R - first, meta->columns[t] = width, meta->first[t] = first;
    }
    for (uint32_t c = C + tid; c < kModelColumns; c += kBlock) aliased[c] = 0;
    if (tid == 0) {
        meta->C = C, meta->R = R, meta->df[num_terms] = R, meta->columns[num_terms] = C, meta->first[num_terms] = 0;
        meta->df_res = (int64_t)L - 1 - (int64_t)R;
    }
}

// the strata rule's tables of the list of the complete cases: one workgroup
__global__ __launch_bounds__(kBlock) void model_strata_kernel(const uint32_t *__restrict__ strata, const uint32_t *__restrict__ idx,
                                                              const ModelMeta *__restrict__ meta, uint32_t *hs, uint32_t *home)
{
    if (blockIdx.x == 0) strata_tables(strata, [&](uint32_t i) { return idx[i]; }, meta->L, hs, home);
}

// the columns of a design as the rule counts them on the arguments, whatever the used samples: a bound of C and of R
inline size_t model_design_columns(const uint32_t *kind, const uint32_t *labels, uint32_t S, uint32_t T)
{
    size_t bound = 0;
    for (uint32_t t = 0; t < T; ++t) {
        std::set<uint32_t> distinct;
        for (uint32_t s = 0; s < S; ++s)
            if (!kind[t] && labels[(size_t)s * T + t] != kModelMissing) distinct.insert(labels[(size_t)s * T + t]);
        bound += kind[t] ? 1 : distinct.empty() ? 0 : distinct.size() - 1;
    }
    return bound;
}

// The design by term into d_lab[T][padded] and d_val[T][padded] on the device: a sample that lacks any value is missing in
// every term, so every term lists the complete cases.  kinds: the kinds for the basis kernel; bound: the columns as the rule
// counts them, at least those of the used samples.
inline int model_design_upload(const uint32_t *kind, const uint32_t *labels, const double *values, uint32_t S, uint32_t T,
                               uint32_t padded, uint32_t *d_lab, double *d_val, ModelKinds &kinds, size_t &bound)
{
    std::vector<uint32_t> lab((size_t)T * padded, kModelMissing);
    std::vector<double> val((size_t)T * padded, 0.0);
    for (uint32_t t = 0; t < T; ++t) kinds.kind[t] = kind[t];
    bound = model_design_columns(kind, labels, S, T);
    for (uint32_t s = 0; s < S; ++s) {
        bool complete = true;
        for (uint32_t t = 0; t < T; ++t)
            complete = complete && (kind[t] ? !std::isnan(values[(size_t)s * T + t]) : labels[(size_t)s * T + t] != kModelMissing);
        if (!complete) continue;
        for (uint32_t t = 0; t < T; ++t) {
            lab[(size_t)t * padded + s] = kind[t] ? 0 : labels[(size_t)s * T + t];
            val[(size_t)t * padded + s] = kind[t] ? values[(size_t)s * T + t] : 0.0;
        }
    }
    HIP_TRY(hipMemcpy(d_lab, lab.data(), lab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_val, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice));
    return EPIK_AMD_OK;
}

}  // namespace

#endif
