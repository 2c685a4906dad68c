// unifrac_place.hip -- the UniFrac distances between every two samples of a cohort: unweighted (Lozupone & Knight 2005),
// normalised weighted (Lozupone et al. 2007) and generalised at alpha = 0.5 (Chen et al. 2012): epik_amd_cohort_unifrac_device
// / _unifrac / _unifrac_host (include/epik_amd.h), and cohort_distance_enqueue, which the analyses that take a distance matrix
// (permanova_place.hip, pcoa_place.hip, permdisp_place.hip) start from.
//
// No reference counterpart: the reference writes a jplace per sample and leaves distances to a second tool.
//
// The rule is stated once, in include/epik_amd.h beside KR's (unifrac_matrix of epik_amd/host/cohort.cpp is
// the same rule on the CPU).  It starts from what the KR distance starts from -- T_s, and the planes C and B that
// cohort_normalise_kernel (cohort_place.hip) leaves as [b][Sp], sample fastest, the padding samples zero -- and from
// d_half, so a call enqueues one normalisation and one distance kernel.
//
// cohort_unifrac_kernel<Metric>: cohort_kr_kernel with a numerator and a denominator a pair.  A workgroup owns a tile of
// 32 x 32 pairs on or above the diagonal, lane (ty, tx) of 16 x 16 the pairs (ty | ty + 16) x (tx | tx + 16): eight
// accumulators in registers.  A chunk of kChunk branches of C and B of the tile's row and column samples is staged in LDS
// as [branch][32 samples]; for one branch a half-wave reads two row addresses (ty: broadcasts) and sixteen consecutive
// doubles of the column samples (tx) -- no bank conflict, as in the KR kernel -- and walks the chunk in ascending order.
// Nothing is fused (__dadd_rn / __dsub_rn / __dmul_rn, and __dsqrt_rn / __ddiv_rn, which round correctly; the file is built
// with -ffp-contract=off as well).  The planes of a sample without mass are NaN (0 / 0) and those of a padding sample zero:
// either only reaches the accumulators of its own pairs, which the rule overwrites (-1.0) or the bounds keep from memory.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kTile = kCohortTile;  // samples a side of a tile of pairs
constexpr uint32_t kChunk = 32;          // branches staged at a time: 4 * 32 * 32 * 8 = 32 KB of LDS
constexpr uint64_t kUnifracBlocks = 65536;

static_assert(kBlock == 256 && kTile == 32, "a lane owns 2 x 2 pairs of a 32 x 32 tile");

// one half-branch of one pair: its terms of the rule's tn_b and td_b
template <uint32_t Metric>
__device__ inline void half_terms(double x, double y, double &tn, double &td)
{
    if (Metric == EPIK_AMD_DISTANCE_UNWEIGHTED) {
        const bool px = x > 0.0, py = y > 0.0;
        tn = px != py ? 1.0 : 0.0;
        td = px || py ? 1.0 : 0.0;
    } else if (Metric == EPIK_AMD_DISTANCE_WEIGHTED) {
        tn = fabs(__dsub_rn(x, y));
        td = __dadd_rn(x, y);
    } else {
        const double sum = __dadd_rn(x, y);
        td = __dsqrt_rn(sum);
        tn = sum > 0.0 ? __dmul_rn(td, __ddiv_rn(fabs(__dsub_rn(x, y)), sum)) : 0.0;
    }
}

// num = num + h * tn_b, den = den + h * td_b of one pair and one branch
template <uint32_t Metric>
__device__ inline void pair_step(double h, double cs, double ct, double bs, double bt, double &num, double &den)
{
    double cn, cd, bn, bd;
    half_terms<Metric>(cs, ct, cn, cd);
    half_terms<Metric>(bs, bt, bn, bd);
    num = __dadd_rn(num, __dmul_rn(h, __dadd_rn(cn, bn)));
    den = __dadd_rn(den, __dmul_rn(h, __dadd_rn(cd, bd)));
}

template <uint32_t Metric>
__global__ __launch_bounds__(kBlock) void cohort_unifrac_kernel(const double *__restrict__ planes, const double *__restrict__ half,
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
        double num00 = 0.0, num01 = 0.0, num10 = 0.0, num11 = 0.0;
        double den00 = 0.0, den01 = 0.0, den10 = 0.0, den11 = 0.0;
        for (uint32_t b0 = 0; b0 < num_branches; b0 += kChunk) {
            const uint32_t kc = num_branches - b0 < kChunk ? num_branches - b0 : kChunk;
            for (uint32_t e = threadIdx.x; e < kc * kTile; e += kBlock) {
                const uint32_t k = e / kTile, x = e % kTile;
                const uint64_t at = (uint64_t)(b0 + k) * padded;  // (b0 + k < num_branches, ti and tj below side: inside the planes)
                c_row[k][x] = C[at + ti * kTile + x], b_row[k][x] = B[at + ti * kTile + x];
                c_col[k][x] = C[at + tj * kTile + x], b_col[k][x] = B[at + tj * kTile + x];
            }
            if (threadIdx.x < kc) half_of[threadIdx.x] = half[b0 + threadIdx.x];
            __syncthreads();
            for (uint32_t k = 0; k < kc; ++k) {  // ascending, one branch after the other: the rule's order
                const double h = half_of[k];
                const double cr0 = c_row[k][ty], cr1 = c_row[k][ty + 16], br0 = b_row[k][ty], br1 = b_row[k][ty + 16];
                const double cc0 = c_col[k][tx], cc1 = c_col[k][tx + 16], bc0 = b_col[k][tx], bc1 = b_col[k][tx + 16];
                pair_step<Metric>(h, cr0, cc0, br0, bc0, num00, den00);
                pair_step<Metric>(h, cr0, cc1, br0, bc1, num01, den01);
                pair_step<Metric>(h, cr1, cc0, br1, bc0, num10, den10);
                pair_step<Metric>(h, cr1, cc1, br1, bc1, num11, den11);
            }
            __syncthreads();
        }
        const double num[2][2] = {{num00, num01}, {num10, num11}}, den[2][2] = {{den00, den01}, {den10, den11}};
#pragma unroll
        for (uint32_t u = 0; u < 2; ++u)
#pragma unroll
            for (uint32_t v = 0; v < 2; ++v) {
                const uint32_t r = ti * kTile + ty + 16 * u, c = tj * kTile + tx + 16 * v;
                // a padding sample (its den is 0) and a diagonal tile's lower half end here: no cell is stored for them
                if (r >= num_samples || c >= num_samples || r > c) continue;
                double d = 0.0;
                if (r != c) {
                    if (total[r] == 0 || total[c] == 0)
                        d = -1.0;
                    else if (den[u][v] != 0.0)
                        d = __ddiv_rn(num[u][v], den[u][v]);
                }
                out[(uint64_t)r * num_samples + c] = d;
                out[(uint64_t)c * num_samples + r] = d;
            }
    }
}

int metric_valid(uint32_t metric)
{
    if (metric < EPIK_AMD_DISTANCE_UNWEIGHTED || metric > EPIK_AMD_DISTANCE_GENERALIZED)
        return fail_with(EPIK_AMD_ERR_INVALID, "metric = " + std::to_string(metric) +
                                                   " is no UniFrac distance (1 unweighted, 2 weighted, 3 generalized)");
    return EPIK_AMD_OK;
}

int unifrac_device_impl(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric, void *d_out,
                        hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(check_present(branch_length, d_out));
    COHORT_TRY(metric_valid(metric));
    const uint32_t N = cohort->num_branches, S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    std::vector<double> half;
    COHORT_TRY(half_branch_lengths(branch_length, N, half));
    // the checks of the tree, the device drained (a distance still reading d_half), the planes: one normalisation a call
    const uint32_t *d_first = nullptr;
    COHORT_TRY(cohort_normalise_enqueue(cohort, tree, stream, &d_first));
    HIP_TRY(hipMemcpy(cohort->d_half, half.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice));
    const uint64_t side = padded / kTile, tiles = side * (side + 1) / 2;
    const dim3 grid = cohort_grid(cohort, tiles, kUnifracBlocks);
    auto *out = static_cast<double *>(d_out);
    if (metric == EPIK_AMD_DISTANCE_UNWEIGHTED)
        hipLaunchKernelGGL(cohort_unifrac_kernel<EPIK_AMD_DISTANCE_UNWEIGHTED>, grid, dim3(kBlock), 0, stream, cohort->d_planes,
                           cohort->d_half, cohort->d_total, S, N, padded, out);
    else if (metric == EPIK_AMD_DISTANCE_WEIGHTED)
        hipLaunchKernelGGL(cohort_unifrac_kernel<EPIK_AMD_DISTANCE_WEIGHTED>, grid, dim3(kBlock), 0, stream, cohort->d_planes,
                           cohort->d_half, cohort->d_total, S, N, padded, out);
    else
        hipLaunchKernelGGL(cohort_unifrac_kernel<EPIK_AMD_DISTANCE_GENERALIZED>, grid, dim3(kBlock), 0, stream, cohort->d_planes,
                           cohort->d_half, cohort->d_total, S, N, padded, out);
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

}  // namespace

namespace epik_amd {

int cohort_distance_enqueue(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                            void *d_out, hipStream_t stream)
{
    if (metric == EPIK_AMD_DISTANCE_KR) return cohort_kr_enqueue(cohort, tree, branch_length, d_out, stream);
    if (metric > EPIK_AMD_DISTANCE_GENERALIZED)
        return fail_with(EPIK_AMD_ERR_INVALID, "metric = " + std::to_string(metric) +
                                                   " is no distance (0 kr, 1 unweighted, 2 weighted, 3 generalized)");
    return unifrac_device_impl(cohort, tree, branch_length, metric, d_out, stream);
}

}  // namespace epik_amd

extern "C" {

int epik_amd_cohort_unifrac_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                                   void *d_out, void *stream)
{
    return guarded("cohort_unifrac_device", [&]() -> int {
        return unifrac_device_impl(cohort, tree, branch_length, metric, d_out, static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_unifrac(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                            double *out)
{
    return guarded("cohort_unifrac", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(check_present(out));
        const size_t bytes = (size_t)cohort->num_samples * cohort->num_samples * sizeof(double);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult m;
        COHORT_TRY(m.alloc(bytes));
        COHORT_TRY(unifrac_device_impl(cohort, tree, branch_length, metric, m.d, nullptr));
        return m.copy_to(out, bytes);
    });
}

int epik_amd_cohort_unifrac_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                 const double *branch_length, uint32_t metric, double *out)
{
    return guarded("cohort_unifrac_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(check_present(mass, first, branch_length, out));
        std::string err;
        return rule_result(unifrac_matrix(mass, num_samples, num_branches, first, branch_length, metric, out, err), err);
    });
}

}  // extern "C"
