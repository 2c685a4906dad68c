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
#include <cstdlib>
#include <cstring>
#include <string>

#include "../host/cohort.hpp"
#include "cohort_device.hpp"
#include "host_entry.hpp"
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
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        const size_t offset = at;
        at += (bytes + 15) / 16 * 16;
        return offset;
    };
    const size_t dd = sizeof(double), uu = sizeof(uint32_t), SS = (size_t)S * S;
    const size_t A = take(SS * dd), A1 = take(SS * dd), V = take(SS * dd), r = take(S * dd), cs = take(S * dd), sn = take(S * dd);
    const size_t gs = take(4 * dd), pn = take(2 * dd), root = take(kMaxK * dd), sign = take(kMaxK * dd);
    const size_t used = take(S * uu), jof = take(S * uu), partner = take(S * uu), count = take(uu);
    const size_t counters = take(kJacobiMaxSweeps * uu), status = take(2 * uu), column = take(kMaxK * uu), real_k = take(kMaxK * uu);
    if (sp) {
        char *b = static_cast<char *>(base);
        const auto d = [&](size_t o) { return reinterpret_cast<double *>(b + o); };
        const auto u = [&](size_t o) { return reinterpret_cast<uint32_t *>(b + o); };
        *sp = PcoaSpace{d(A), d(A1), d(V), d(r), d(cs), d(sn), d(gs), d(pn), d(root), d(sign), u(used), u(jof), u(partner),
                        u(count), u(counters), u(status), u(column), u(real_k)};
    }
    return at;
}

__global__ __launch_bounds__(kBlock) void pcoa_rows_kernel(const double *__restrict__ kr, const uint32_t *__restrict__ used,
                                                           uint32_t num_samples, uint32_t L, double *__restrict__ r)
{
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < L; i += gridDim.x * kBlock) {
        const double *column = kr + used[i];  // KR[u_j][u_i] = KR[u_i][u_j]
        double acc = 0.0;
#pragma unroll 4  // (the reads of four values are in flight ahead of the dependent adds)
        for (uint32_t j = 0; j < L; ++j) {  // ascending: the rule's order
            const double d = column[(uint64_t)used[j] * num_samples];
            acc = __dadd_rn(acc, __dmul_rn(d, d));
        }
        r[i] = __ddiv_rn(acc, (double)L);
    }
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
        double g = 0.0;
        for (uint32_t i = 0; i < L; ++i) g = __dadd_rn(g, r[i]);  // ascending: the rule's order
        if (L) g = __ddiv_rn(g, (double)L);
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
    const uint64_t cells = (uint64_t)L * L;
    const double g = gs[3];
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock) {
        const uint32_t i = (uint32_t)(e / L), j = (uint32_t)(e - (uint64_t)i * L), lo = i < j ? i : j, hi = i < j ? j : i;
        B[e] = gower_centred(kr[(uint64_t)used[lo] * num_samples + used[hi]], r[lo], r[hi], g);
    }
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
    if (!cohort) return fail_with(EPIK_AMD_ERR_INVALID, "null cohort");
    if (const int rc = components_valid(K); rc != EPIK_AMD_OK) return rc;
    if (!d_kr || !d_mu || !d_coord || !d_info) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
    if (!cohort->d_total)
        return fail_with(EPIK_AMD_ERR_INVALID, "the cohort has no distances yet: d_kr must be what kr_device wrote for this cohort");
    HIP_TRY(hipSetDevice(cohort->device));
    HIP_TRY(hipDeviceSynchronize());  // (the distances enqueued on whatever stream, and an earlier call that reads the workspace)
    const uint32_t S = cohort->num_samples;
    if (!cohort->d_pcoa) HIP_TRY(hipMalloc(&cohort->d_pcoa, pcoa_space(nullptr, S, nullptr)));
    PcoaSpace sp;
    pcoa_space(cohort->d_pcoa, S, &sp);
    const uint64_t cap = cohort->max_blocks_cap ? cohort->max_blocks_cap : ~0ull;
    const auto blocks = [&](uint64_t units) {
        return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(units + kBlock - 1) / kBlock, kMaxBlocks, cap})));
    };
    const auto *kr = static_cast<const double *>(d_kr);
    if (const int rc = cohort_used_index_enqueue(cohort, sp.used, sp.jof, sp.count, stream); rc != EPIK_AMD_OK) return rc;
    uint32_t L = 0;
    HIP_TRY(hipMemcpyAsync(&L, sp.count, sizeof L, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (L > S) return fail_with(EPIK_AMD_ERR_HIP, "cohort_pcoa: the device counted more used samples than there are samples");
    const uint32_t Kc = std::min(K, L);
    const uint64_t cells = (uint64_t)L * L;
    if (L) hipLaunchKernelGGL(pcoa_rows_kernel, blocks(L), dim3(kBlock), 0, stream, kr, sp.used, S, L, sp.r);
    hipLaunchKernelGGL(pcoa_scale_kernel, blocks(cells), dim3(kBlock), 0, stream, kr, sp.used, S, L, sp.r, sp.gs, sp.V, sp.counters);
    if (L) hipLaunchKernelGGL(pcoa_centre_kernel, blocks(cells), dim3(kBlock), 0, stream, kr, sp.used, S, L, sp.r, sp.gs, sp.A);
    HIP_TRY(hipGetLastError());
    // EPIK_AMD_PCOA_LDS=0 (tests), read at the call: the eigensolver's global path whatever L
    const char *env = std::getenv("EPIK_AMD_PCOA_LDS");
    const bool lds = L <= kJacobiLdsSide && !(env && std::strcmp(env, "0") == 0);
    uint32_t sweeps = 1, converged = 1;  // (L = 0: one empty sweep)
    if (L) {
        const JacobiSpace js{sp.A, sp.A1, sp.V, sp.cs, sp.sn, sp.gs, sp.partner, sp.counters, sp.status};
        if (const int rc = jacobi_sweeps(js, L, lds, cap, stream, sweeps, converged); rc != EPIK_AMD_OK) return rc;
    }
    hipLaunchKernelGGL(pcoa_order_kernel, dim3(1), dim3(kBlock), 0, stream, sp.A, sp.V, L, S, Kc, sp.gs, sp.column, sp.real_k, sp.root,
                       sp.sign, sp.pn, static_cast<double *>(d_mu));
    hipLaunchKernelGGL(pcoa_coord_kernel, blocks((uint64_t)S * K), dim3(kBlock), 0, stream, static_cast<double *>(d_coord), sp.V, sp.jof,
                       sp.column, sp.real_k, sp.root, sp.sign, S, K, Kc, L, sp.gs, sp.pn, L && lds ? sp.status : nullptr, sweeps,
                       converged, static_cast<epik_amd_pcoa_info *>(d_info));
    HIP_TRY(hipGetLastError());
    return EPIK_AMD_OK;
}

// a result in device memory for the synchronous entry, freed however the call ends
struct Result {
    void *d = nullptr;
    ~Result()
    {
        if (d) (void)hipDeviceSynchronize(), (void)hipFree(d);
    }
};

}  // namespace

extern "C" {

int epik_amd_cohort_pcoa_device(epik_amd_cohort *cohort, const void *d_kr, uint32_t num_components, void *d_mu, void *d_coord,
                                void *d_info, void *stream)
{
    try {
        return pcoa_device_impl(cohort, d_kr, num_components, d_mu, d_coord, d_info, static_cast<hipStream_t>(stream));
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("cohort_pcoa_device: ") + e.what());
    }
}

int epik_amd_cohort_pcoa(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t num_components,
                         double *mu, double *coord, epik_amd_pcoa_info *info)
{
    return epik_amd_cohort_pcoa_metric(cohort, tree, branch_length, EPIK_AMD_DISTANCE_KR, num_components, mu, coord, info);
}

int epik_amd_cohort_pcoa_metric(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, uint32_t metric,
                                uint32_t num_components, double *mu, double *coord, epik_amd_pcoa_info *info)
{
    try {
        if (!cohort) return fail_with(EPIK_AMD_ERR_INVALID, "null cohort");
        if (const int rc = components_valid(num_components); rc != EPIK_AMD_OK) return rc;
        if (!mu || !coord || !info) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
        const size_t K = num_components, S = cohort->num_samples;
        HIP_TRY(hipSetDevice(cohort->device));
        Result kr, m;
        const size_t doubles = S + S * K;  // mu | coord, then the info block
        HIP_TRY(hipMalloc(&kr.d, S * S * sizeof(double)));
        HIP_TRY(hipMalloc(&m.d, doubles * sizeof(double) + sizeof(epik_amd_pcoa_info)));
        if (const int rc = cohort_distance_enqueue(cohort, tree, branch_length, metric, kr.d, nullptr); rc != EPIK_AMD_OK) return rc;
        double *d = static_cast<double *>(m.d);
        if (const int rc = pcoa_device_impl(cohort, kr.d, num_components, d, d + S, d + doubles, nullptr); rc != EPIK_AMD_OK) return rc;
        HIP_TRY(hipMemcpy(mu, d, S * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(coord, d + S, S * K * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(info, d + doubles, sizeof *info, hipMemcpyDeviceToHost));
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("cohort_pcoa: ") + e.what());
    }
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
    try {
        if (num_samples == 0) return fail_with(EPIK_AMD_ERR_INVALID, "a cohort has at least one sample (num_samples is 0)");
        if (num_branches == 0) return fail_with(EPIK_AMD_ERR_INVALID, "a tree has at least one branch");
        if (!mass || !first || !branch_length || !mu || !coord || !info) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
        std::string err;
        if (const int rc = pcoa_components(mass, num_samples, num_branches, first, branch_length, num_components, mu, coord, info, err, metric);
            rc != EPIK_AMD_OK)
            return fail_with(rc, err);
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("cohort_pcoa_host: ") + e.what());
    }
}

int epik_amd_cohort_pcoa_kr_host(const double *kr, const uint64_t *totals, uint32_t num_samples, uint32_t num_components, double *mu,
                                 double *coord, epik_amd_pcoa_info *info)
{
    try {
        if (num_samples == 0) return fail_with(EPIK_AMD_ERR_INVALID, "a cohort has at least one sample (num_samples is 0)");
        if (!kr || !totals || !mu || !coord || !info) return fail_with(EPIK_AMD_ERR_INVALID, "null argument");
        std::string err;
        if (const int rc = pcoa_components_of_kr(kr, totals, num_samples, num_components, mu, coord, info, err); rc != EPIK_AMD_OK)
            return fail_with(rc, err);
        return EPIK_AMD_OK;
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string("cohort_pcoa_kr_host: ") + e.what());
    }
}

}  // extern "C"
