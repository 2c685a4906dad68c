// epca_place.hip -- edge principal components (Matsen & Evans 2013) of a cohort's samples on the device:
// epik_amd_cohort_epca_device / _epca / _epca_host (include/epik_amd.h).
//
// No reference counterpart.  The rule is stated once, in include/epik_amd.h beside the KR and squash rules (DESIGN.md
// 3.10; epik_amd/host/cohort.cpp: epca_components is the same rule on the CPU).  Every sum the rule orders is walked in
// that order by one lane, and every rotation of a Jacobi round is formed from the matrix as it was when the round began,
// so the results are the same bits here, on the host and in the tests' numpy.  Nothing is fused (__dmul_rn / __dadd_rn /
// __dsub_rn / __ddiv_rn / __dsqrt_rn; the file is built with -ffp-contract=off as well).  No MFMA: the Gram matrix is a
// product, but the order in which v_mfma_f64_* adds up its terms is not documented, and the rule fixes that order.
//
// Start-up: cohort_normalise_kernel (cohort_place.hip) leaves T_s and the planes C, B [b][Sp].
//   used_index_kernel    (cohort_place.hip) the used samples (T_s > 0) in ascending s: used[j], jof[s], and L -- which the host reads back:
//                        the grids, the round-robin schedule and the choice of the eigensolver's path depend on it.
//   epca_centre_kernel   a lane a branch: X_j[b], the sequential sum over j for the mean, Y into a plane [b][Lp], used
//                        samples compacted, sample fastest, Lp a multiple of the tile, the padding zero.
//   epca_gram_kernel     cohort_kr_kernel's tile with one plane and a product for |a - b|: 32 x 32 pairs on or above the
//                        diagonal, 2 x 2 a lane, 32 branches staged in LDS a chunk, b ascending, mirrored on the way out.
//   epca_scale_kernel    scale, trace and tol by one lane in the rule's order; V = I and the sweep counters zeroed.
// The eigensolver is jacobi_place.hip's (shared with pcoa_place.hip): one launch in LDS for L <= 64, three launches a
// round beyond, the same bits; the host reads the sweep's rotation counter, 4 bytes, once a sweep there.
// Then epca_order_kernel (the ranks by counting), epca_raw_kernel (a lane per (b, k), j ascending), epca_sign_kernel
// (the (|value|, b) reduction, a workgroup a component) and epca_finish_kernel (edge, proj and the info block).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"
#include "jacobi_device.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kNone = kCohortNoIndex;
constexpr uint32_t kTile = kCohortTile;
constexpr uint32_t kChunk = 32;                              // branches staged at a time: 2 * 32 * 32 * 8 = 16 KB of LDS
constexpr uint32_t kMaxK = EPIK_AMD_EPCA_MAX_COMPONENTS;
constexpr uint32_t kMaxSweeps = kJacobiMaxSweeps;
constexpr uint64_t kMaxBlocks = 1024;
constexpr uint64_t kGramBlocks = 65536;

static_assert(sizeof(epik_amd_epca_info) == 32);
static_assert(kBlock == 256 && kTile == 32, "a lane owns 2 x 2 pairs of a 32 x 32 tile");

// the workspace, one allocation: what the kernels take
struct EpcaSpace {
    double *Y;         // [N][Lp]
    double *A, *A1;    // [L][L] each: the matrix, and the matrix after the column phase
    double *V;         // [L][L]
    double *cs, *sn;   // [L]: c_j, s_j of the round at hand
    double *gs;        // scale, trace, tol
    double *root, *sign;  // [kMaxK]: sqrt(mu_k), +-1
    uint32_t *used, *jof, *partner;  // [S]: the sample of index j; the index of sample s or kNone; j' or kNone
    uint32_t *count;                 // L
    uint32_t *counters;              // [kMaxSweeps]: the rotations of a sweep (the global path)
    uint32_t *status;                // sweeps, converged (the LDS path)
    uint32_t *column, *null_k;       // [kMaxK]: j(k); whether component k is null
};

size_t epca_space(void *base, uint32_t S, uint32_t N, uint32_t padded, EpcaSpace *sp)
{
    const size_t SS = (size_t)S * S;
    Carver c(base);
    const EpcaSpace parts{.Y = c.take<double>((size_t)N * padded),
                          .A = c.take<double>(SS),
                          .A1 = c.take<double>(SS),
                          .V = c.take<double>(SS),
                          .cs = c.take<double>(S),
                          .sn = c.take<double>(S),
                          .gs = c.take<double>(4),
                          .root = c.take<double>(kMaxK),
                          .sign = c.take<double>(kMaxK),
                          .used = c.take<uint32_t>(S),
                          .jof = c.take<uint32_t>(S),
                          .partner = c.take<uint32_t>(S),
                          .count = c.take<uint32_t>(1),
                          .counters = c.take<uint32_t>(kMaxSweeps),
                          .status = c.take<uint32_t>(2),
                          .column = c.take<uint32_t>(kMaxK),
                          .null_k = c.take<uint32_t>(kMaxK)};
    if (sp) *sp = parts;
    return c.bytes();
}

__global__ __launch_bounds__(kBlock) void epca_centre_kernel(const double *__restrict__ planes, const uint32_t *__restrict__ first,
                                                             const uint32_t *__restrict__ used, uint32_t num_branches,
                                                             uint32_t padded, uint32_t L, uint32_t Lp, double *__restrict__ Y)
{
    const double *C = planes, *B = planes + (uint64_t)num_branches * padded;
    for (uint32_t b = blockIdx.x * kBlock + threadIdx.x; b < num_branches; b += gridDim.x * kBlock) {
        const bool inner = first[b] < b;
        double *y = Y + (uint64_t)b * Lp;
        double acc = 0.0;
        for (uint32_t j = 0; j < L; ++j) {  // ascending: the rule's order
            const uint64_t at = (uint64_t)b * padded + used[j];
            const double x = inner ? __dsub_rn(__dadd_rn(B[at], C[at]), 1.0) : 0.0;
            y[j] = x;
            acc = __dadd_rn(acc, x);
        }
        const double mean = __ddiv_rn(acc, (double)L);
        for (uint32_t j = 0; j < L; ++j) y[j] = __dsub_rn(y[j], mean);
        for (uint32_t j = L; j < Lp; ++j) y[j] = 0.0;
    }
}

__global__ __launch_bounds__(kBlock) void epca_gram_kernel(const double *__restrict__ Y, uint32_t num_branches, uint32_t L,
                                                           uint32_t Lp, double *__restrict__ G)
{
    __shared__ double y_row[kChunk][kTile], y_col[kChunk][kTile];
    const uint32_t side = Lp / kTile, tx = threadIdx.x % 16, ty = threadIdx.x / 16;
    const uint64_t tiles = (uint64_t)side * (side + 1) / 2;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        // tile (ti, tj), ti <= tj, counted along the rows of the upper triangle
        uint32_t ti = 0;
        uint64_t rem = tile;
        while (rem >= side - ti) rem -= side - ti, ++ti;
        const uint32_t tj = ti + (uint32_t)rem;
        double acc00 = 0.0, acc01 = 0.0, acc10 = 0.0, acc11 = 0.0;
        for (uint32_t b0 = 0; b0 < num_branches; b0 += kChunk) {
            const uint32_t kc = num_branches - b0 < kChunk ? num_branches - b0 : kChunk;
            for (uint32_t e = threadIdx.x; e < kc * kTile; e += kBlock) {
                const uint32_t k = e / kTile, x = e % kTile;
                const uint64_t at = (uint64_t)(b0 + k) * Lp;
                y_row[k][x] = Y[at + ti * kTile + x];
                y_col[k][x] = Y[at + tj * kTile + x];
            }
            __syncthreads();
            for (uint32_t k = 0; k < kc; ++k) {  // ascending, one branch after the other: the rule's order
                const double r0 = y_row[k][ty], r1 = y_row[k][ty + 16], c0 = y_col[k][tx], c1 = y_col[k][tx + 16];
                acc00 = __dadd_rn(acc00, __dmul_rn(r0, c0));
                acc01 = __dadd_rn(acc01, __dmul_rn(r0, c1));
                acc10 = __dadd_rn(acc10, __dmul_rn(r1, c0));
                acc11 = __dadd_rn(acc11, __dmul_rn(r1, c1));
            }
            __syncthreads();
        }
        const double acc[2][2] = {{acc00, acc01}, {acc10, acc11}};
#pragma unroll
        for (uint32_t u = 0; u < 2; ++u)
#pragma unroll
            for (uint32_t v = 0; v < 2; ++v) {
                const uint32_t r = ti * kTile + ty + 16 * u, c = tj * kTile + tx + 16 * v;
                if (r >= L || c >= L || r > c) continue;  // (a diagonal tile: its upper half, mirrored)
                G[(uint64_t)r * L + c] = acc[u][v];
                G[(uint64_t)c * L + r] = acc[u][v];
            }
    }
}

__global__ __launch_bounds__(kBlock) void epca_scale_kernel(const double *__restrict__ G, uint32_t L, double *__restrict__ gs,
                                                            double *__restrict__ V, uint32_t *__restrict__ counters)
{
    const uint64_t cells = (uint64_t)L * L;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock)
        V[e] = e / L == e % L ? 1.0 : 0.0;
    if (blockIdx.x == 0 && threadIdx.x < kMaxSweeps) counters[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double scale = 0.0, trace = 0.0;
        for (uint32_t j = 0; j < L; ++j) {  // ascending: the rule's order
            const double g = G[(uint64_t)j * L + j];
            if (g > scale) scale = g;
            trace = __dadd_rn(trace, g);
        }
        gs[0] = scale, gs[1] = trace, gs[2] = __dmul_rn(0x1p-52, scale);
    }
}

__global__ __launch_bounds__(kBlock) void epca_order_kernel(const double *__restrict__ A, uint32_t L, uint32_t K, uint32_t Kc,
                                                            const double *__restrict__ gs, uint32_t *__restrict__ column,
                                                            uint32_t *__restrict__ null_k, double *__restrict__ root,
                                                            double *__restrict__ mu)
{
    const double floor_mu = __dmul_rn(0x1p-40, gs[0]);
    for (uint32_t j = threadIdx.x; j < L; j += kBlock) {
        const double mine = A[(uint64_t)j * L + j];
        uint32_t rank = 0;
        for (uint32_t i = 0; i < L; ++i) {
            const double other = A[(uint64_t)i * L + i];
            rank += other > mine || (other == mine && i < j) ? 1u : 0u;
        }
        if (rank < Kc) {  // (the ranks are a permutation: every k < Kc is written once)
            const bool is_null = !(mine > floor_mu);
            column[rank] = j, null_k[rank] = is_null ? 1u : 0u, mu[rank] = mine;
            root[rank] = is_null ? 0.0 : __dsqrt_rn(mine);
        }
    }
    for (uint32_t k = Kc + threadIdx.x; k < K; k += kBlock) mu[k] = 0.0;
}

__global__ __launch_bounds__(kBlock) void epca_raw_kernel(const double *__restrict__ V, const double *__restrict__ Y, uint32_t L,
                                                          uint32_t Lp, uint32_t num_branches, uint32_t K, uint32_t Kc,
                                                          const uint32_t *__restrict__ column, const uint32_t *__restrict__ null_k,
                                                          double *__restrict__ edge)
{
    const uint64_t cells = (uint64_t)K * num_branches;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock) {
        const uint32_t b = (uint32_t)(e / K), k = (uint32_t)(e - (uint64_t)b * K);  // k fastest: a wave shares its rows of Y
        double acc = 0.0;
        if (k < Kc && !null_k[k]) {
            const double *v = V + column[k], *y = Y + (uint64_t)b * Lp;
            for (uint32_t j = 0; j < L; ++j) acc = __dadd_rn(acc, __dmul_rn(v[(uint64_t)j * L], y[j]));  // ascending: the rule's order
        }
        edge[(uint64_t)k * num_branches + b] = acc;
    }
}

// whether (|v|, b) comes before (|best_v|, best_b): the larger magnitude, then the smaller branch
__device__ inline bool larger_first(double v, uint32_t b, double best_v, uint32_t best_b)
{
    return b != kNone && (best_b == kNone || fabs(v) > fabs(best_v) || (fabs(v) == fabs(best_v) && b < best_b));
}

__global__ __launch_bounds__(kBlock) void epca_sign_kernel(const double *__restrict__ edge, uint32_t num_branches, uint32_t Kc,
                                                           double *__restrict__ sign)
{
    __shared__ double wave_val[kBlockWaves];
    __shared__ uint32_t wave_at[kBlockWaves];
    for (uint32_t k = blockIdx.x; k < Kc; k += gridDim.x) {
        const double *raw = edge + (uint64_t)k * num_branches;
        double val = 0.0;
        uint32_t at = kNone;
        for (uint32_t b = threadIdx.x; b < num_branches; b += kBlock) {  // (ascending in a lane: strict > keeps the first)
            const double v = raw[b];
            if (at == kNone || fabs(v) > fabs(val)) val = v, at = b;
        }
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const double ov = __shfl_down(val, d);
            const uint32_t oa = __shfl_down(at, d);
            if (larger_first(ov, oa, val, at)) val = ov, at = oa;
        }
        if (threadIdx.x % kWave == 0) wave_val[threadIdx.x / kWave] = val, wave_at[threadIdx.x / kWave] = at;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (uint32_t w = 1; w < kBlockWaves; ++w)
                if (larger_first(wave_val[w], wave_at[w], val, at)) val = wave_val[w], at = wave_at[w];
            sign[k] = val < 0.0 ? -1.0 : 1.0;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void epca_finish_kernel(double *__restrict__ edge, double *__restrict__ proj,
                                                             const double *__restrict__ V, const uint32_t *__restrict__ jof,
                                                             const uint32_t *__restrict__ column, const uint32_t *__restrict__ null_k,
                                                             const double *__restrict__ root, const double *__restrict__ sign,
                                                             uint32_t num_samples, uint32_t num_branches, uint32_t K, uint32_t Kc,
                                                             uint32_t L, const double *__restrict__ gs, const uint32_t *status,
                                                             uint32_t sweeps, uint32_t converged, epik_amd_epca_info *__restrict__ info)
{
    const uint64_t edges = (uint64_t)K * num_branches, projs = (uint64_t)num_samples * K;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < edges + projs; e += (uint64_t)gridDim.x * kBlock) {
        if (e < edges) {
            const uint32_t k = (uint32_t)(e / num_branches);
            edge[e] = k < Kc && !null_k[k] ? __dmul_rn(sign[k], __ddiv_rn(edge[e], root[k])) : 0.0;
        } else {
            const uint64_t at = e - edges;
            const uint32_t s = (uint32_t)(at / K), k = (uint32_t)(at - (uint64_t)s * K), j = jof[s];
            proj[at] = k < Kc && !null_k[k] && j != kNone ? __dmul_rn(sign[k], __dmul_rn(V[(uint64_t)j * L + column[k]], root[k])) : 0.0;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *info = epik_amd_epca_info{L, Kc, status ? status[0] : sweeps, status ? status[1] : converged, gs[1], gs[0]};
}

int components_valid(uint32_t K)
{
    if (K < 1 || K > kMaxK) return fail_with(EPIK_AMD_ERR_INVALID, "num_components = " + std::to_string(K) + " is outside [1, 64]");
    return EPIK_AMD_OK;
}

int epca_device_impl(epik_amd_cohort *cohort, const epik_amd_tree *tree, uint32_t K, void *d_mu, void *d_proj, void *d_edge,
                     void *d_info, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(components_valid(K));
    COHORT_TRY(check_present(d_mu, d_proj, d_edge, d_info));
    // the checks of the tree, the device drained, the planes' workspace, T_s and the planes
    const uint32_t *d_first = nullptr;
    COHORT_TRY(cohort_normalise_enqueue(cohort, tree, stream, &d_first));
    const uint32_t N = cohort->num_branches, S = cohort->num_samples, padded = cohort_padded_samples(cohort);
    COHORT_TRY(cohort_space_ensure(cohort, kSpaceEpca, epca_space(nullptr, S, N, padded, nullptr)));
    EpcaSpace sp;
    epca_space(cohort->space[kSpaceEpca].d, S, N, padded, &sp);
    const uint64_t cap = cohort->max_blocks_cap ? cohort->max_blocks_cap : ~0ull;  // (the eigensolver's)
    COHORT_TRY(cohort_used_index_enqueue(cohort, sp.used, sp.jof, sp.count, stream));
    uint32_t L = 0;
    HIP_TRY(hipMemcpyAsync(&L, sp.count, sizeof L, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (L > S) return fail_with(EPIK_AMD_ERR_HIP, "cohort_epca: the device counted more used samples than there are samples");
    const uint32_t Lp = (L + kTile - 1) / kTile * kTile, Kc = std::min(K, L);
    const uint64_t cells = (uint64_t)L * L;
    if (L) {
        hipLaunchKernelGGL(epca_centre_kernel, cohort_grid_per(cohort, N, kBlock, kMaxBlocks), dim3(kBlock), 0, stream, cohort->d_planes, d_first,
                           sp.used, N, padded, L, Lp, sp.Y);
        const uint64_t side = Lp / kTile;
        hipLaunchKernelGGL(epca_gram_kernel, cohort_grid_per(cohort, side * (side + 1) / 2, 1, kGramBlocks), dim3(kBlock), 0, stream, sp.Y, N, L, Lp,
                           sp.A);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(epca_scale_kernel, cohort_grid_per(cohort, cells, kBlock, kMaxBlocks), dim3(kBlock), 0, stream, sp.A, L, sp.gs, sp.V, sp.counters);
    HIP_TRY(hipGetLastError());
    const bool lds = lds_switch("EPIK_AMD_EPCA_LDS", L, kJacobiLdsSide);  // (=0, tests: the global path whatever L)
    uint32_t sweeps = 1, converged = 1;  // (L = 0: one empty sweep)
    if (L) {
        const JacobiSpace js{sp.A, sp.A1, sp.V, sp.cs, sp.sn, sp.gs, sp.partner, sp.counters, sp.status};
        COHORT_TRY(jacobi_sweeps(js, L, lds, cap, stream, sweeps, converged));
    }
    auto *mu = static_cast<double *>(d_mu), *proj = static_cast<double *>(d_proj), *edge = static_cast<double *>(d_edge);
    hipLaunchKernelGGL(epca_order_kernel, dim3(1), dim3(kBlock), 0, stream, sp.A, L, K, Kc, sp.gs, sp.column, sp.null_k, sp.root, mu);
    hipLaunchKernelGGL(epca_raw_kernel, cohort_grid_per(cohort, (uint64_t)K * N, kBlock, kMaxBlocks), dim3(kBlock), 0, stream, sp.V, sp.Y, L, Lp, N, K,
                       Kc, sp.column, sp.null_k, edge);
    hipLaunchKernelGGL(epca_sign_kernel, cohort_grid_per(cohort, std::max(Kc, 1u), 1, kMaxBlocks), dim3(kBlock), 0, stream, edge, N, Kc, sp.sign);
    hipLaunchKernelGGL(epca_finish_kernel, cohort_grid_per(cohort, (uint64_t)K * N + (uint64_t)S * K, kBlock, kMaxBlocks), dim3(kBlock), 0, stream, edge,
                       proj, sp.V, sp.jof, sp.column, sp.null_k, sp.root, sp.sign, S, N, K, Kc, L, sp.gs,
                       L && lds ? sp.status : nullptr, sweeps, converged, static_cast<epik_amd_epca_info *>(d_info));
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

}  // namespace

extern "C" {

int epik_amd_cohort_epca_device(epik_amd_cohort *cohort, const epik_amd_tree *tree, uint32_t num_components, void *d_mu,
                                void *d_proj, void *d_edge, void *d_info, void *stream)
{
    return guarded("cohort_epca_device", [&]() -> int {
        return epca_device_impl(cohort, tree, num_components, d_mu, d_proj, d_edge, d_info, static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_epca(epik_amd_cohort *cohort, const epik_amd_tree *tree, uint32_t num_components, double *mu, double *proj,
                         double *edge, epik_amd_epca_info *info)
{
    return guarded("cohort_epca", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        const size_t K = num_components, S = cohort->num_samples, N = cohort->num_branches;
        COHORT_TRY(components_valid(num_components));
        COHORT_TRY(check_present(mu, proj, edge, info));
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult m;
        const size_t dd = sizeof(double), doubles = K + S * K + K * N;  // mu | proj | edge, then the info block
        COHORT_TRY(m.alloc(doubles * dd + sizeof(epik_amd_epca_info)));
        double *d = static_cast<double *>(m.d);
        COHORT_TRY(epca_device_impl(cohort, tree, num_components, d, d + K, d + K + S * K, d + doubles, nullptr));
        COHORT_TRY(m.copy_to(mu, K * dd));
        COHORT_TRY(m.copy_to(proj, S * K * dd, K * dd));
        COHORT_TRY(m.copy_to(edge, K * N * dd, (K + S * K) * dd));
        return m.copy_to(info, sizeof *info, doubles * dd);
    });
}

int epik_amd_cohort_epca_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                              uint32_t num_components, double *mu, double *proj, double *edge, epik_amd_epca_info *info)
{
    return guarded("cohort_epca_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(check_present(mass, first, mu, proj, edge, info));
        std::string err;
        return rule_result(epca_components(mass, num_samples, num_branches, first, num_components, mu, proj, edge, info, err), err);
    });
}

}  // extern "C"
