// pcoa_place.hip -- principal coordinates (Gower 1966) of a cohort's samples over their KR distances on the device:
// epik_amd_cohort_pcoa_device / _pcoa / _pcoa_host / _pcoa_kr_host (include/epik_amd.h).
//
// No reference counterpart.  The rule is stated once, in include/epik_amd.h beside the PERMANOVA rule (DESIGN.md 3.18;
// epik_amd/host/cohort.cpp: pcoa_components_of_kr is the same rule on the CPU).  Every sum the rule orders is walked in that
// order by one lane, and the eigensolver is the edge PCA's (jacobi_place.hip), so the results are the same bits here, on
// the host and in the tests' numpy.  Nothing is fused (__dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn / __dsqrt_rn; the
// file is built with -ffp-contract=off as well).  No MFMA, for the reason epca_place.hip gives: the centring is sums in a
// fixed order, and there is no product of matrices here at all.
//
//   used_index_kernel   (cohort_place.hip) the used samples (T_s > 0) in ascending s: used[j], jof[s], and L -- which the
//                       host reads back: the grids and the choice of the eigensolver's path depend on it.
//   pcoa_rows_kernel    a lane a row: r_i, the chain over j ascending of KR * KR, then one division.  The lanes of a wave
//                       read KR[u_j][u_i] for a j they share -- the matrix is symmetric bit for bit, so that is
//                       KR[u_i][u_j], and a coalesced line.
//   pcoa_scale_kernel   one lane: g, then scale, trace and tol over the diagonal of B in the rule's order (a diagonal
//                       element is the rule's expression of r_j and g, formed here as the centring kernel forms it); the
//                       other lanes set V = I and zero the sweep counters.
//   pcoa_centre_kernel  grid-stride over the cells: B[i][j] from (min, max) -- the upper triangle, mirrored.
//   the eigensolver     jacobi_place.hip: in LDS up to L = 64, three launches a round beyond.
//   pcoa_order_kernel   one workgroup: the ranks by counting, mu[k] for all L eigenvalues, both thresholds; then a lane an
//                       axis for the sign (the first j with the largest |V[j][j(k)]|) and one lane for the pos and neg
//                       chains in rank order.
//   pcoa_coord_kernel   grid-stride over coord[S][K], and the info block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../host/cohort.hpp"
#include "cohort_entry.hpp"
#include "jacobi_device.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kMaxK = EPIK_AMD_PCOA_MAX_COMPONENTS;
constexpr uint64_t kMaxBlocks = 1024;

static_assert(sizeof(epik_amd_pcoa_info) == 48, "the info block is 48 bytes");
static_assert(kMaxK <= kBlock, "a lane an axis in the order kernel");

// the workspace, one allocation: what the kernels take
struct PcoaSpace {
    double *A, *A1, *V;  // [S][S] each: B and then the rotated matrix; the matrix after the column phase; the vectors
    double *r;           // [S]: the row means of the squared distances
    double *cs, *sn;     // [S]: the eigensolver's
    double *gs;          // scale, trace, tol, g
    double *pn;          // pos, neg
    double *root, *sign; // [kMaxK]: sqrt(mu_k), +-1
    uint32_t *used, *jof, *partner;  // [S]
    uint32_t *count;                 // L
    uint32_t *counters;              // [kJacobiMaxSweeps]
    uint32_t *status;                // sweeps, converged (the LDS path)
    uint32_t *column, *real_k;       // [kMaxK]: j(k); whether axis k is real
};

size_t pcoa_space(void *base, uint32_t S, PcoaSpace *sp)
{
    const size_t SS = (size_t)S * S;
    Carver c(base);
    const PcoaSpace parts{.A = c.take<double>(SS),
                          .A1 = c.take<double>(SS),
                          .V = c.take<double>(SS),
                          .r = c.take<double>(S),
                          .cs = c.take<double>(S),
                          .sn = c.take<double>(S),
                          .gs = c.take<double>(4),
                          .pn = c.take<double>(2),
                          .root = c.take<double>(kMaxK),
                          .sign = c.take<double>(kMaxK),
                          .used = c.take<uint32_t>(S),
                          .jof = c.take<uint32_t>(S),
                          .partner = c.take<uint32_t>(S),
                          .count = c.take<uint32_t>(1),
                          .counters = c.take<uint32_t>(kJacobiMaxSweeps),
                          .status = c.take<uint32_t>(2),
                          .column = c.take<uint32_t>(kMaxK),
                          .real_k = c.take<uint32_t>(kMaxK)};
    if (sp) *sp = parts;
    return c.bytes();
}

__global__ __launch_bounds__(kBlock) void pcoa_rows_kernel(const double *__restrict__ kr, const uint32_t *__restrict__ used,
                                                           uint32_t num_samples, uint32_t L, double *__restrict__ r)
{
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < L; i += gridDim.x * kBlock) r[i] = gower_row_mean(kr, used, num_samples, L, i);
}

__global__ __launch_bounds__(kBlock) void pcoa_scale_kernel(const double *__restrict__ kr, const uint32_t *__restrict__ used,
                                                            uint32_t num_samples, uint32_t L, const double *__restrict__ r,
                                                            double *__restrict__ gs, double *__restrict__ V,
                                                            uint32_t *__restrict__ counters)
{
    const uint64_t cells = (uint64_t)L * L;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock)
        V[e] = e / L == e % L ? 1.0 : 0.0;
    if (blockIdx.x == 0 && threadIdx.x < kJacobiMaxSweeps) counters[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const double g = gower_mean_of_means(r, L);
        double scale = 0.0, trace = 0.0;
        for (uint32_t j = 0; j < L; ++j) {
            const uint32_t s = used[j];
            const double b = gower_centred(kr[(uint64_t)s * num_samples + s], r[j], r[j], g);
            if (fabs(b) > scale) scale = fabs(b);
            trace = __dadd_rn(trace, b);
        }
        gs[0] = scale, gs[1] = trace, gs[2] = __dmul_rn(0x1p-52, scale), gs[3] = g;
    }
}

__global__ __launch_bounds__(kBlock) void pcoa_centre_kernel(const double *__restrict__ kr, const uint32_t *__restrict__ used,
                                                             uint32_t num_samples, uint32_t L, const double *__restrict__ r,
                                                             const double *__restrict__ gs, double *__restrict__ B)
{
    gower_centre_cells(kr, used, num_samples, L, r, gs[3], B);
}

__global__ __launch_bounds__(kBlock) void pcoa_order_kernel(const double *__restrict__ A, const double *__restrict__ V, uint32_t L,
                                                            uint32_t num_samples, uint32_t Kc, const double *__restrict__ gs,
                                                            uint32_t *column, uint32_t *real_k, double *__restrict__ root,
                                                            double *__restrict__ sign, double *__restrict__ pn, double *mu)
{
    const double floor_mu = __dmul_rn(0x1p-40, gs[0]);
    for (uint32_t j = threadIdx.x; j < L; j += kBlock) {
        const double mine = A[(uint64_t)j * L + j];
        uint32_t rank = 0;
        for (uint32_t i = 0; i < L; ++i) {
            const double other = A[(uint64_t)i * L + i];
            rank += other > mine || (other == mine && i < j) ? 1u : 0u;
        }
        mu[rank] = mine;  // (the ranks are a permutation of 0 .. L - 1: every mu[k], k < L, is written once)
        if (rank < Kc) {
            const bool real = mine > floor_mu;
            column[rank] = j, real_k[rank] = real ? 1u : 0u;
            root[rank] = real ? __dsqrt_rn(mine) : 0.0;
        }
    }
    for (uint32_t k = L + threadIdx.x; k < num_samples; k += kBlock) mu[k] = 0.0;
    __syncthreads();  // (one workgroup: mu, column and real_k are complete)
    if (threadIdx.x < Kc) {
        const uint32_t k = threadIdx.x;
        double s = 1.0;
        if (real_k[k]) {
            const double *v = V + column[k];
            double best = v[0];
            for (uint32_t j = 1; j < L; ++j) {  // (ascending, strict >: the first of the largest)
                const double x = v[(uint64_t)j * L];
                if (fabs(x) > fabs(best)) best = x;
            }
            s = best < 0.0 ? -1.0 : 1.0;
        }
        sign[k] = s;
    }
    if (threadIdx.x == kBlock - 1) {
        double pos = 0.0, neg = 0.0;
        for (uint32_t k = 0; k < L; ++k) {  // in rank order: the rule's
            const double m = mu[k];
            if (m > floor_mu) pos = __dadd_rn(pos, m);
            if (m < -floor_mu) neg = __dadd_rn(neg, m);
        }
        pn[0] = pos, pn[1] = neg;
    }
}

__global__ __launch_bounds__(kBlock) void pcoa_coord_kernel(double *__restrict__ coord, const double *__restrict__ V,
                                                            const uint32_t *__restrict__ jof, const uint32_t *__restrict__ column,
                                                            const uint32_t *__restrict__ real_k, const double *__restrict__ root,
                                                            const double *__restrict__ sign, uint32_t num_samples, uint32_t K,
                                                            uint32_t Kc, uint32_t L, const double *__restrict__ gs,
                                                            const double *__restrict__ pn, const uint32_t *status, uint32_t sweeps,
                                                            uint32_t converged, epik_amd_pcoa_info *__restrict__ info)
{
    const uint64_t cells = (uint64_t)num_samples * K;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock) {
        const uint32_t s = (uint32_t)(e / K), k = (uint32_t)(e - (uint64_t)s * K), j = jof[s];
        coord[e] = k < Kc && real_k[k] && j != kCohortNoIndex ? __dmul_rn(sign[k], __dmul_rn(V[(uint64_t)j * L + column[k]], root[k])) : 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *info = epik_amd_pcoa_info{L, Kc, status ? status[0] : sweeps, status ? status[1] : converged, gs[1], gs[0], pn[0], pn[1]};
}

int components_valid(uint32_t K)
{
    if (K < 1 || K > kMaxK) return fail_with(EPIK_AMD_ERR_INVALID, "num_components = " + std::to_string(K) + " is outside [1, 64]");
    return EPIK_AMD_OK;
}

int pcoa_device_impl(epik_amd_cohort *cohort, const void *d_kr, uint32_t K, void *d_mu, void *d_coord, void *d_info, hipStream_t stream)
{
    COHORT_TRY(check_cohort(cohort));
    COHORT_TRY(components_valid(K));
    COHORT_TRY(check_present(d_kr, d_mu, d_coord, d_info));
    COHORT_TRY(check_has_distances(cohort));
    HIP_TRY(hipSetDevice(cohort->device));
    HIP_TRY(hipDeviceSynchronize());  // (the distances enqueued on whatever stream, and an earlier call that reads the workspace)
    const uint32_t S = cohort->num_samples;
    COHORT_TRY(cohort_space_ensure(cohort, kSpacePcoa, pcoa_space(nullptr, S, nullptr)));
    PcoaSpace sp;
    pcoa_space(cohort->space[kSpacePcoa].d, S, &sp);
    const uint64_t cap = cohort->max_blocks_cap ? cohort->max_blocks_cap : ~0ull;  // (the eigensolver's)
    const auto *kr = static_cast<const double *>(d_kr);
    COHORT_TRY(cohort_used_index_enqueue(cohort, sp.used, sp.jof, sp.count, stream));
    uint32_t L = 0;
    HIP_TRY(hipMemcpyAsync(&L, sp.count, sizeof L, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (L > S) return fail_with(EPIK_AMD_ERR_HIP, "cohort_pcoa: the device counted more used samples than there are samples");
    const uint32_t Kc = std::min(K, L);
    const uint64_t cells = (uint64_t)L * L;
    if (L) hipLaunchKernelGGL(pcoa_rows_kernel, cohort_grid_per(cohort, L, kBlock, kMaxBlocks), dim3(kBlock), 0, stream, kr, sp.used, S, L, sp.r);
    hipLaunchKernelGGL(pcoa_scale_kernel, cohort_grid_per(cohort, cells, kBlock, kMaxBlocks), dim3(kBlock), 0, stream, kr, sp.used, S, L, sp.r, sp.gs, sp.V, sp.counters);
    if (L) hipLaunchKernelGGL(pcoa_centre_kernel, cohort_grid_per(cohort, cells, kBlock, kMaxBlocks), dim3(kBlock), 0, stream, kr, sp.used, S, L, sp.r, sp.gs, sp.A);
    HIP_TRY(hipGetLastError());
    const bool lds = lds_switch("EPIK_AMD_PCOA_LDS", L, kJacobiLdsSide);  // (=0, tests: the eigensolver's global path whatever L)
    uint32_t sweeps = 1, converged = 1;  // (L = 0: one empty sweep)
    if (L) {
        const JacobiSpace js{sp.A, sp.A1, sp.V, sp.cs, sp.sn, sp.gs, sp.partner, sp.counters, sp.status};
        COHORT_TRY(jacobi_sweeps(js, L, lds, cap, stream, sweeps, converged));
    }
    hipLaunchKernelGGL(pcoa_order_kernel, dim3(1), dim3(kBlock), 0, stream, sp.A, sp.V, L, S, Kc, sp.gs, sp.column, sp.real_k, sp.root,
                       sp.sign, sp.pn, static_cast<double *>(d_mu));
    hipLaunchKernelGGL(pcoa_coord_kernel, cohort_grid_per(cohort, (uint64_t)S * K, kBlock, kMaxBlocks), dim3(kBlock), 0, stream,
                       static_cast<double *>(d_coord), sp.V, sp.jof,
                       sp.column, sp.real_k, sp.root, sp.sign, S, K, Kc, L, sp.gs, sp.pn, L && lds ? sp.status : nullptr, sweeps,
                       converged, static_cast<epik_amd_pcoa_info *>(d_info));
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

}  // namespace

extern "C" {

int epik_amd_cohort_pcoa_device(epik_amd_cohort *cohort, const void *d_kr, uint32_t num_components, void *d_mu, void *d_coord,
                                void *d_info, void *stream)
{
    return guarded("cohort_pcoa_device", [&]() -> int {
        return pcoa_device_impl(cohort, d_kr, num_components, d_mu, d_coord, d_info, static_cast<hipStream_t>(stream));
    });
}

int epik_amd_cohort_pcoa(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t num_components,
                         double *mu, double *coord, epik_amd_pcoa_info *info)
{
    return epik_amd_cohort_pcoa_metric(cohort, tree, branch_length, EPIK_AMD_DISTANCE_KR, num_components, mu, coord, info);
}

int epik_amd_cohort_pcoa_metric(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                                uint32_t num_components, double *mu, double *coord, epik_amd_pcoa_info *info)
{
    return guarded("cohort_pcoa", [&]() -> int {
        COHORT_TRY(check_cohort(cohort));
        COHORT_TRY(components_valid(num_components));
        COHORT_TRY(check_present(mu, coord, info));
        const size_t K = num_components, S = cohort->num_samples;
        HIP_TRY(hipSetDevice(cohort->device));
        DeviceResult kr, m;
        const size_t doubles = S + S * K;  // mu | coord, then the info block
        COHORT_TRY(kr.alloc(S * S * sizeof(double)));
        COHORT_TRY(m.alloc(doubles * sizeof(double) + sizeof(epik_amd_pcoa_info)));
        COHORT_TRY(cohort_distance_enqueue(cohort, tree, branch_length, metric, kr.d, nullptr));
        double *d = static_cast<double *>(m.d);
        COHORT_TRY(pcoa_device_impl(cohort, kr.d, num_components, d, d + S, d + doubles, nullptr));
        COHORT_TRY(m.copy_to(mu, S * sizeof(double)));
        COHORT_TRY(m.copy_to(coord, S * K * sizeof(double), S * sizeof(double)));
        return m.copy_to(info, sizeof *info, doubles * sizeof(double));
    });
}

int epik_amd_cohort_pcoa_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                              const double *branch_length, uint32_t num_components, double *mu, double *coord,
                              epik_amd_pcoa_info *info)
{
    return epik_amd_cohort_pcoa_metric_host(mass, num_samples, num_branches, first, branch_length, EPIK_AMD_DISTANCE_KR, num_components, mu,
                                            coord, info);
}

int epik_amd_cohort_pcoa_metric_host(const uint64_t *mass, uint32_t num_samples, uint32_t num_branches, const uint32_t *first,
                                     const double *branch_length, uint32_t metric, uint32_t num_components, double *mu, double *coord,
                                     epik_amd_pcoa_info *info)
{
    return guarded("cohort_pcoa_host", [&]() -> int {
        COHORT_TRY(check_host_shape(num_samples, num_branches));
        COHORT_TRY(check_present(mass, first, branch_length, mu, coord, info));
        std::string err;
        return rule_result(pcoa_components(mass, num_samples, num_branches, first, branch_length, num_components, mu, coord, info, err, metric),
                           err);
    });
}

int epik_amd_cohort_pcoa_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, uint32_t num_components, double *mu,
                                 double *coord, epik_amd_pcoa_info *info)
{
    return guarded("cohort_pcoa_kr_host", [&]() -> int {
        COHORT_TRY(check_host_samples(num_samples));
        COHORT_TRY(check_present(kr, totals, mu, coord, info));
        std::string err;
        return rule_result(pcoa_components_of_kr(kr, totals, num_samples, num_components, mu, coord, info, err), err);
    });
}

}  // extern "C"
