// diversity_place.hip -- alpha diversity (McCoy & Matsen 2013) and rarefaction curves (Nipperess & Matsen 2013) of a
// cohort's samples on the device: epik_amd_cohort_alpha_device / _alpha / _alpha_host and epik_amd_cohort_rarefy_device /
// _rarefy / _rarefy_host (include/epik_amd.h).
//
// No reference counterpart.  The rule is stated once, in include/epik_amd.h beside the KR, squash, epca and kmeans rules
// (epik_amd/host/cohort.cpp: alpha_indices and rarefy_curves are the same rule on the CPU).  Every sum
// over the branches is the rule's blocked sum -- the 256 terms of a block in ascending b, then the blocks in ascending g
// -- so every output is the same bits here, on the host and in the tests' numpy.  Nothing is fused (__dmul_rn / __dadd_rn /
// __dsub_rn / __ddiv_rn / __dsqrt_rn; the file is built with -ffp-contract=off as well).  No log, no pow: the header says
// why.
//
// cohort_normalise_kernel (cohort_place.hip) leaves the prefix sums of mass, T_s and the planes C, B [b][Sp].  Then
//
//   diversity_counts_kernel  that kernel's prefix scan run over `best`, a workgroup a sample: cc[s][b], cb[s][b] and n_s.
//   diversity_alpha_kernel   a workgroup a (sample, block): a lane forms the five terms of its branch into LDS, five lanes
//                            add the block's terms in order: partials [S][G][5].
//   diversity_rarefy_kernel  the hot path.  A workgroup a (sample, block), a lane a branch: the four recurrences Q(cb),
//                            Q(n - cb), Q(cc), Q(n - cc) live in registers across all depths, the factor n - m - k as a
//                            double decremented by 1.0 (exact below 2^53: the bits of the conversion).  r_k = 1 / (n - k)
//                            is computed once per workgroup for kRecips depths at a time into LDS and read as a
//                            broadcast.  At an output depth a lane leaves its two terms in LDS; after kBuffered output
//                            depths 2 * kBuffered lanes add the 256 terms of their (depth, index) in order, side by side:
//                            partials [S][G][J][2].
//   diversity_finish_*       add the block partials in ascending g; the -1.0 cells.
//
// A side that is empty (m == 0) is exactly 1 and a side with m >= n - k exactly 0 by the rule.  Here the factor of a side
// with m >= n starts at +0.0, the factor of every other side reaches +0.0 at k = n - m, and a product with it is a zero
// from then on; its sign cannot reach an output (1.0 - (+-0.0) = 1.0, and x - (+-0.0) = x for the x >= +0.0 at hand), and
// the kernel takes |Q| all the same.  The empty side is picked at the output.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kDivBlock = EPIK_AMD_DIVERSITY_BLOCK;  // branches of a block of the blocked sum: a lane each
constexpr uint32_t kPitch = kDivBlock + 1;  // of a row of terms in LDS: the adding lanes walk the rows side by side, a bank apart
constexpr uint32_t kIndices = 5;            // pd, rooted_pd, bwpd_half, bwpd_one, quadratic
constexpr uint32_t kBuffered = 8;           // output depths a workgroup buffers before it adds them
constexpr uint32_t kRecips = 256;           // reciprocals staged at a time
constexpr uint32_t kTotals = 5;             // the totals that end a row of cells (cohort_place.hip)
constexpr uint64_t kManyBlocks = 65536;
constexpr uint64_t kExact = 1ull << 53;     // a sample with n_s reads at or above is not rarefiable

static_assert(sizeof(epik_amd_alpha) == kIndices * sizeof(double));
static_assert(kDivBlock == kBlock && kRecips <= kBlock && 2 * kBuffered <= kBlock);

// the workspace of the counts and of the alpha partials, one allocation
struct DiversitySpace {
    uint64_t *cb, *cc;  // [S][N]: the reads strictly below b, and in its clade (cb holds the prefix sums on the way)
    uint64_t *reads;    // [S]: n_s
    double *partial;    // [S][G][5]
};

uint32_t num_blocks_of(uint32_t N) { return (N + kDivBlock - 1) / kDivBlock; }

size_t diversity_space(void *base, uint32_t S, uint32_t N, DiversitySpace *sp)
{
    // (cb and cc are one part, cc straight behind cb: S * N may be odd, and a part of its own would begin 8 bytes later)
    const size_t cells = (size_t)S * N;
    Carver c(base);
    uint64_t *counts = c.take<uint64_t>(2 * cells);
    const DiversitySpace parts{.cb = counts,
                               .cc = counts ? counts + cells : nullptr,
                               .reads = c.take<uint64_t>(S),
                               .partial = c.take<double>((size_t)S * num_blocks_of(N) * kIndices)};
    if (sp) *sp = parts;
    return c.bytes();
}

__global__ __launch_bounds__(kBlock) void diversity_counts_kernel(const uint64_t *__restrict__ g_cells, const uint32_t *__restrict__ first,
                                                                  uint32_t num_samples, uint32_t num_branches,
                                                                  uint64_t *__restrict__ cb, uint64_t *__restrict__ cc,
                                                                  uint64_t *__restrict__ reads)
{
    __shared__ uint64_t wave_sums[kBlockWaves];
    const uint64_t stride = 2ull * num_branches + kTotals;
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    for (uint32_t s = blockIdx.x; s < num_samples; s += gridDim.x) {
        const uint64_t *best = g_cells + s * stride + num_branches;
        uint64_t *P = cb + (uint64_t)s * num_branches, *clade = cc + (uint64_t)s * num_branches;
        uint64_t carry = 0;  // (the same in every lane)
        for (uint32_t base = 0; base < num_branches; base += kBlock) {
            const uint32_t b = base + threadIdx.x;
            uint64_t v = b < num_branches ? best[b] : 0;
#pragma unroll
            for (uint32_t d = 1; d < kWave; d <<= 1) {
                const uint64_t up = __shfl_up((unsigned long long)v, d);
                if (lane >= d) v += up;
            }
            if (lane == kWave - 1) wave_sums[wave] = v;
            __syncthreads();
            uint64_t before = carry, all = carry;
#pragma unroll
            for (uint32_t k = 0; k < kBlockWaves; ++k) {
                if (k < wave) before += wave_sums[k];
                all += wave_sums[k];
            }
            if (b < num_branches) P[b] = before + v;
            carry = all;
            __syncthreads();  // (wave_sums is written again; the last round: P is the workgroup's to read)
        }
        if (threadIdx.x == 0) reads[s] = carry;
        for (uint32_t b = threadIdx.x; b < num_branches; b += kBlock) {
            const uint32_t f = first[b];
            clade[b] = P[b] - (f ? P[f - 1] : 0);
        }
        __syncthreads();  // (every read of P is done: it becomes cb)
        for (uint32_t b = threadIdx.x; b < num_branches; b += kBlock) P[b] = clade[b] - best[b];
        __syncthreads();
    }
}

__device__ inline double balance(double d)
{
    const double w = fmin(d, __dsub_rn(1.0, d));
    return w > 0.0 ? w : 0.0;
}

__global__ __launch_bounds__(kBlock) void diversity_alpha_kernel(const uint64_t *__restrict__ g_cells, const uint32_t *__restrict__ first,
                                                                 const uint64_t *__restrict__ prefix, const uint64_t *__restrict__ total,
                                                                 const double *__restrict__ planes, const double *__restrict__ half,
                                                                 uint32_t num_samples, uint32_t num_branches, uint32_t padded,
                                                                 double *__restrict__ partial)
{
    __shared__ double terms[kIndices][kPitch];
    const uint64_t stride = 2ull * num_branches + kTotals;
    const uint32_t G = (num_branches + kDivBlock - 1) / kDivBlock;
    const uint64_t units = (uint64_t)num_samples * G;
    const double *C = planes, *B = planes + (uint64_t)num_branches * padded;
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t s = (uint32_t)(unit / G), g = (uint32_t)(unit % G);
        const uint64_t T = total[s];
        if (T == 0) continue;  // (uniform: the finish kernel writes -1.0)
        const uint32_t b = g * kDivBlock + threadIdx.x;
        const uint32_t count = num_branches - g * kDivBlock < kDivBlock ? num_branches - g * kDivBlock : kDivBlock;
        if (b < num_branches) {
            const uint64_t *P = prefix + (uint64_t)s * num_branches;
            const uint32_t f = first[b];
            const uint64_t clade = P[b] - (f ? P[f - 1] : 0), below = clade - g_cells[s * stride + b];
            const double c = C[(uint64_t)b * padded + s], bw = B[(uint64_t)b * padded + s], h = half[b];
            const double wb = balance(bw), wc = balance(c);
            terms[0][threadIdx.x] = __dmul_rn(h, __dadd_rn(below > 0 && below < T ? 1.0 : 0.0, clade > 0 && clade < T ? 1.0 : 0.0));
            terms[1][threadIdx.x] = __dmul_rn(h, __dadd_rn(below > 0 ? 1.0 : 0.0, clade > 0 ? 1.0 : 0.0));
            terms[2][threadIdx.x] = __dmul_rn(h, __dadd_rn(__dsqrt_rn(__dmul_rn(2.0, wb)), __dsqrt_rn(__dmul_rn(2.0, wc))));
            terms[3][threadIdx.x] = __dmul_rn(h, __dadd_rn(__dmul_rn(2.0, wb), __dmul_rn(2.0, wc)));
            terms[4][threadIdx.x] = __dmul_rn(h, __dadd_rn(__dmul_rn(bw, __dsub_rn(1.0, bw)), __dmul_rn(c, __dsub_rn(1.0, c))));
        }
        __syncthreads();
        if (threadIdx.x < kIndices) {
            double acc = 0.0;
#pragma unroll 8
            for (uint32_t i = 0; i < count; ++i) acc = __dadd_rn(acc, terms[threadIdx.x][i]);  // ascending b: the rule's order
            partial[unit * kIndices + threadIdx.x] = acc;
        }
        __syncthreads();  // (the terms are written again)
    }
}

__global__ __launch_bounds__(kBlock) void diversity_finish_alpha_kernel(const double *__restrict__ partial, const uint64_t *__restrict__ total,
                                                                        uint32_t num_samples, uint32_t num_branches,
                                                                        double *__restrict__ alpha)
{
    const uint32_t G = (num_branches + kDivBlock - 1) / kDivBlock;
    const uint64_t cells = (uint64_t)num_samples * kIndices;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock) {
        const uint32_t s = (uint32_t)(e / kIndices), f = (uint32_t)(e % kIndices);
        double acc = -1.0;
        if (total[s] != 0) {
            acc = 0.0;
            for (uint32_t g = 0; g < G; ++g) acc = __dadd_rn(acc, partial[((uint64_t)s * G + g) * kIndices + f]);  // ascending g
        }
        alpha[e] = acc;
    }
}

// the j with k_j <= n of a rarefiable sample, else 0
__device__ inline uint32_t depths_of(uint64_t n, uint32_t depth_step, uint32_t num_depths)
{
    if (n == 0 || n >= kExact) return 0;
    const uint64_t fit = n / depth_step;
    return fit < num_depths ? (uint32_t)fit : num_depths;
}

__global__ __launch_bounds__(kBlock) void diversity_rarefy_kernel(const uint64_t *__restrict__ cb, const uint64_t *__restrict__ cc,
                                                                  const uint64_t *__restrict__ reads, const double *__restrict__ half,
                                                                  uint32_t num_samples, uint32_t num_branches, uint32_t depth_step,
                                                                  uint32_t num_depths, double *__restrict__ partial)
{
    __shared__ double terms[kBuffered][2][kPitch];
    __shared__ double recip[kRecips];
    const uint32_t G = (num_branches + kDivBlock - 1) / kDivBlock;
    const uint64_t units = (uint64_t)num_samples * G;
    for (uint64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t s = (uint32_t)(unit / G), g = (uint32_t)(unit % G);
        const uint64_t n = reads[s];
        const uint32_t depths = depths_of(n, depth_step, num_depths);
        if (depths == 0) continue;  // (uniform: the finish kernel writes -1.0)
        const uint32_t deepest = depths * depth_step;  // <= 2^20, <= n
        const uint32_t b = g * kDivBlock + threadIdx.x;
        const uint32_t count = num_branches - g * kDivBlock < kDivBlock ? num_branches - g * kDivBlock : kDivBlock;
        const bool mine = b < num_branches;  // (a lane past N walks an empty branch and its terms are never added)
        const uint64_t x_b = mine ? cb[(uint64_t)s * num_branches + b] : 0, x_c = mine ? cc[(uint64_t)s * num_branches + b] : 0;
        const double h = mine ? half[b] : 0.0;
        // the four sides: below, all but below, clade, all but clade
        const uint64_t m0 = x_b, m1 = n - x_b, m2 = x_c, m3 = n - x_c;
        double f0 = m0 < n ? __ull2double_rn(n - m0) : 0.0, f1 = m1 < n ? __ull2double_rn(n - m1) : 0.0;
        double f2 = m2 < n ? __ull2double_rn(n - m2) : 0.0, f3 = m3 < n ? __ull2double_rn(n - m3) : 0.0;
        double q0 = 1.0, q1 = 1.0, q2 = 1.0, q3 = 1.0;
        uint32_t since = 0, slot = 0, j_base = 0;  // steps since the last output depth; buffered output depths; the first of them
        for (uint32_t k0 = 0; k0 < deepest; k0 += kRecips) {
            const uint32_t kc = deepest - k0 < kRecips ? deepest - k0 : kRecips;
            __syncthreads();  // (the reads of the reciprocals before are done)
            if (threadIdx.x < kc) recip[threadIdx.x] = __ddiv_rn(1.0, __ull2double_rn(n - (k0 + threadIdx.x)));
            __syncthreads();
            uint32_t kk = 0;
            while (kk < kc) {
                const uint32_t run = kc - kk < depth_step - since ? kc - kk : depth_step - since;
#pragma unroll 4
                for (uint32_t i = 0; i < run; ++i) {
                    const double r = recip[kk + i];  // a broadcast
                    q0 = __dmul_rn(__dmul_rn(q0, f0), r), f0 = __dsub_rn(f0, 1.0);
                    q1 = __dmul_rn(__dmul_rn(q1, f1), r), f1 = __dsub_rn(f1, 1.0);
                    q2 = __dmul_rn(__dmul_rn(q2, f2), r), f2 = __dsub_rn(f2, 1.0);
                    q3 = __dmul_rn(__dmul_rn(q3, f3), r), f3 = __dsub_rn(f3, 1.0);
                }
                kk += run, since += run;
                if (since != depth_step) continue;  // (uniform)
                since = 0;
                const double miss_b = m0 == 0 ? 1.0 : fabs(q0), all_b = m1 == 0 ? 1.0 : fabs(q1);
                const double miss_c = m2 == 0 ? 1.0 : fabs(q2), all_c = m3 == 0 ? 1.0 : fabs(q3);
                const double ru_b = __dsub_rn(1.0, miss_b), ru_c = __dsub_rn(1.0, miss_c);
                double uu_b = __dsub_rn(ru_b, all_b), uu_c = __dsub_rn(ru_c, all_c);
                uu_b = uu_b > 0.0 ? uu_b : 0.0, uu_c = uu_c > 0.0 ? uu_c : 0.0;
                terms[slot][0][threadIdx.x] = __dmul_rn(h, __dadd_rn(uu_b, uu_c));
                terms[slot][1][threadIdx.x] = __dmul_rn(h, __dadd_rn(ru_b, ru_c));
                ++slot;
                if (slot < kBuffered && j_base + slot < depths) continue;  // (uniform)
                __syncthreads();
                if (threadIdx.x < 2 * slot) {
                    const uint32_t d = threadIdx.x / 2, idx = threadIdx.x % 2;
                    const double *row = terms[d][idx];
                    double acc = 0.0;
#pragma unroll 8  // (the reads of eight terms are in flight ahead of the dependent adds)
                    for (uint32_t i = 0; i < count; ++i) acc = __dadd_rn(acc, row[i]);  // ascending b: the rule's order
                    partial[(unit * num_depths + j_base + d) * 2 + idx] = acc;
                }
                __syncthreads();  // (the terms are written again)
                j_base += slot, slot = 0;
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void diversity_finish_rarefy_kernel(const double *__restrict__ partial, const uint64_t *__restrict__ reads,
                                                                         uint32_t num_samples, uint32_t num_branches, uint32_t depth_step,
                                                                         uint32_t num_depths, double *__restrict__ curve)
{
    const uint32_t G = (num_branches + kDivBlock - 1) / kDivBlock;
    const uint64_t per = 2ull * num_depths, cells = (uint64_t)num_samples * per;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock) {
        const uint32_t s = (uint32_t)(e / per), j = (uint32_t)(e % per) / 2;
        double acc = -1.0;
        if (j < depths_of(reads[s], depth_step, num_depths)) {
            acc = 0.0;
            for (uint32_t g = 0; g < G; ++g) acc = __dadd_rn(acc, partial[((uint64_t)s * G + g) * per + e % per]);  // ascending g
        }
        curve[e] = acc;
    }
}

// the checks of kr_device, the device drained, T_s and the planes, the lengths copied, the workspace and the counts
int diversity_begin(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, hipStream_t stream,
                    const uint32_t **d_first, DiversitySpace *sp)
{
    const uint32_t N = cohort->num_branches, S = cohort->num_samples;
    std::vector<double> half;
    COHORT_TRY(half_branch_lengths(branch_length, N, half));
    COHORT_TRY(cohort_normalise_enqueue(cohort, tree, stream, d_first));
    HIP_TRY(hipMemcpy(cohort->d_half, half.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice));
    COHORT_TRY(cohort_space_ensure(cohort, kSpaceDiversity, diversity_space(nullptr, S, N, nullptr)));
    diversity_space(cohort->space[kSpaceDiversity].d, S, N, sp);
    return EPIK_AMD_OK;
}

int alpha_device_impl(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, void *d_alpha,
                      hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(check_present(branch_length, d_alpha));
    const uint32_t N = cohort->num_branches, S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    const uint32_t *d_first = nullptr;
    DiversitySpace sp;
    COHORT_TRY(diversity_begin(cohort, tree, branch_length, stream, &d_first, &sp));
    hipLaunchKernelGGL(diversity_alpha_kernel, cohort_grid(cohort, (uint64_t)S * num_blocks_of(N), kManyBlocks), dim3(kBlock), 0, stream,
                       cohort->d_cells, d_first, cohort->d_prefix, cohort->d_total, cohort->d_planes, cohort->d_half, S, N, padded,
                       sp.partial);
    hipLaunchKernelGGL(diversity_finish_alpha_kernel, cohort_grid_per(cohort, (uint64_t)S * kIndices, kBlock, kManyBlocks), dim3(kBlock), 0, stream,
                       sp.partial, cohort->d_total, S, N, static_cast<double *>(d_alpha));
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

int check_depths(uint32_t depth_step, uint32_t num_depths)
{
    std::string err;
    return rule_result(rarefy_depths_valid(depth_step, num_depths, err), err);
}

int rarefy_device_impl(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t depth_step,
                       uint32_t num_depths, void *d_curve, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(check_present(branch_length, d_curve));
    COHORT_TRY(check_depths(depth_step, num_depths));
    const uint32_t N = cohort->num_branches, S = cohort->num_samples;
    const uint32_t *d_first = nullptr;
    DiversitySpace sp;
    COHORT_TRY(diversity_begin(cohort, tree, branch_length, stream, &d_first, &sp));
    // the block partials of the curve, [S][G][J][2]: kept, and allocated anew only for more depths than any call before
    // (diversity_begin has drained the device)
    COHORT_TRY(cohort_space_ensure(cohort, kSpaceRarefy, (size_t)S * num_blocks_of(N) * num_depths * 2 * sizeof(double)));
    double *partial = static_cast<double *>(cohort->space[kSpaceRarefy].d);
    hipLaunchKernelGGL(diversity_counts_kernel, cohort_grid(cohort, S, kManyBlocks), dim3(kBlock), 0, stream, cohort->d_cells, d_first, S, N,
                       sp.cb, sp.cc, sp.reads);
    hipLaunchKernelGGL(diversity_rarefy_kernel, cohort_grid(cohort, (uint64_t)S * num_blocks_of(N), kManyBlocks), dim3(kBlock), 0, stream, sp.cb,
                       sp.cc, sp.reads, cohort->d_half, S, N, depth_step, num_depths, partial);
    hipLaunchKernelGGL(diversity_finish_rarefy_kernel, cohort_grid_per(cohort, (uint64_t)S * num_depths * 2, kBlock, kManyBlocks), dim3(kBlock), 0, stream,
                       partial, sp.reads, S, N, depth_step, num_depths, static_cast<double *>(d_curve));
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

// the shape and the arguments of a _host entry
int check_host(uint32_t num_samples, uint32_t num_branches, const void *cells, const uint32_t *first, const double *branch_length,
               const void *out)
{
    COHORT_TRY(check_host_shape(num_samples, num_branches));
    return check_present(cells, first, branch_length, out);
}

}  // namespace

extern "C" {

int epik_amd_cohort_alpha_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, void *d_alpha,
                                 void *stream)
{
    return guarded("cohort_alpha_device", [&]() -> int { return alpha_device_impl(cohort, tree, branch_length, d_alpha, static_cast<hipStream_t>(stream)); });
}

int epik_amd_cohort_alpha(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, epik_amd_alpha *alpha)
{
    return guarded("cohort_alpha", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(check_present(alpha));
        const size_t bytes = (size_t)cohort->num_samples * sizeof(epik_amd_alpha);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult r;
        COHORT_TRY(r.alloc(bytes));
        COHORT_TRY(alpha_device_impl(cohort, tree, branch_length, r.d, nullptr));
        return r.copy_to(alpha, bytes);
    });
}

int epik_amd_cohort_alpha_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                               const double *branch_length, epik_amd_alpha *alpha)
{
    return guarded("cohort_alpha_host", [&]() -> int {
        COHORT_TRY(check_host(num_samples, num_branches, mass, first, branch_length, alpha));
        std::string err;
        return rule_result(alpha_indices(mass, num_samples, num_branches, first, branch_length, alpha, err), err);
    });
}

int epik_amd_cohort_rarefy_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length,
                                  uint32_t depth_step, uint32_t num_depths, void *d_curve, void *stream)
{
    return guarded("cohort_rarefy_device", [&]() -> int {
        return rarefy_device_impl(cohort, tree, branch_length, depth_step, num_depths, d_curve, static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_rarefy(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t depth_step,
                           uint32_t num_depths, double *curve)
{
    return guarded("cohort_rarefy", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(check_present(curve));
        COHORT_TRY(check_depths(depth_step, num_depths));
        const size_t bytes = (size_t)cohort->num_samples * num_depths * 2 * sizeof(double);
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult r;
        COHORT_TRY(r.alloc(bytes));
        COHORT_TRY(rarefy_device_impl(cohort, tree, branch_length, depth_step, num_depths, r.d, nullptr));
        return r.copy_to(curve, bytes);
    });
}

int epik_amd_cohort_rarefy_host(const uint64_t *best, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                const double *branch_length, uint32_t depth_step, uint32_t num_depths, double *curve)
{
    return guarded("cohort_rarefy_host", [&]() -> int {
        COHORT_TRY(check_depths(depth_step, num_depths));
        COHORT_TRY(check_host(num_samples, num_branches, best, first, branch_length, curve));
        std::string err;
        return rule_result(rarefy_curves(best, num_samples, num_branches, first, branch_length, depth_step, num_depths, curve, err), err);
    });
}

}  // extern "C"
