// jacobi_place.hip -- the eigensolver that epca_place.hip and pcoa_place.hip share (jacobi_device.hpp): the cyclic Jacobi
// iteration in round-robin order of the edge-PCA rule (include/epik_amd.h), on a symmetric L x L matrix in device memory.  It
// knows nothing of what the matrix is: it takes the matrix, V and the workspace.  One translation unit, so that the library
// holds one copy of every kernel.
//
// Two paths that give the same bits (every element of a phase is one expression of the matrix before that phase, whoever
// computes it):
//   jacobi_lds_kernel    L <= 64: one workgroup, A and V in LDS (2 * 32 KB), all rounds and sweeps in one launch.  A
//                        phase computes its 16 elements a lane into registers, a barrier, the write-back, a barrier.
//   jacobi_params_kernel / jacobi_column_kernel / jacobi_row_kernel  any L: three launches a round, grid-stride.  The
//                        column kernel goes from A to a second matrix and turns V in place (a lane owns both columns
//                        of a pair), the row kernel goes back to A: every (i, j) from (min, max) -- the mirror.  The
//                        host reads the sweep's rotation counter, 4 bytes, once a sweep.
// Nothing is fused (__dmul_rn / __dadd_rn / __dsub_rn / __ddiv_rn / __dsqrt_rn; the file is built with -ffp-contract=off as
// well).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "epik_amd.h"
#include "host_entry.hpp"
#include "jacobi_device.hpp"

namespace {

using namespace epik_amd;

constexpr uint32_t kJacobiNone = 0xffffffffu;                                  // partner[]: the index does not rotate in the round
constexpr uint32_t kJacobiLdsHeld = kJacobiLdsSide * kJacobiLdsSide / kBlock;  // elements of a matrix a lane holds across a barrier
constexpr uint64_t kJacobiMaxBlocks = 1024;

static_assert(kJacobiLdsHeld * kBlock == kJacobiLdsSide * kJacobiLdsSide);

// pair i of round r of the round-robin schedule over m indices (m even), ordered
__device__ inline void pair_of(uint32_t m, uint32_t r, uint32_t i, uint32_t &p, uint32_t &q)
{
    const uint32_t x = i ? (r + i) % (m - 1) : r, y = i ? (r + m - 1 - i) % (m - 1) : m - 1;
    p = x < y ? x : y, q = x < y ? y : x;
}

// the rotation of a pair from A as it is at the start of the round; whether it rotates
__device__ inline bool rotation_of(double app, double aqq, double apq, double tol, double &c, double &s)
{
    if (!(fabs(apq) > tol)) return false;
    const double theta = __ddiv_rn(__dsub_rn(aqq, app), __dmul_rn(2.0, apq));
    double t = __ddiv_rn(1.0, __dadd_rn(fabs(theta), __dsqrt_rn(__dadd_rn(__dmul_rn(theta, theta), 1.0))));
    if (theta < 0.0) t = -t;
    c = __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(__dmul_rn(t, t), 1.0)));
    s = __dmul_rn(t, c);
    return true;
}

// c * a - s * b: two products, then one subtraction
__device__ inline double turned(double c, double a, double s, double b) { return __dsub_rn(__dmul_rn(c, a), __dmul_rn(s, b)); }

__global__ __launch_bounds__(kBlock) void jacobi_lds_kernel(double *__restrict__ A_g, double *__restrict__ V_g, uint32_t L,
                                                            const double *__restrict__ gs, uint32_t *__restrict__ status)
{
    extern __shared__ double lds_matrices[];  // A[L][L] | V[L][L]
    __shared__ double cs[kJacobiLdsSide], sn[kJacobiLdsSide];
    __shared__ uint32_t partner[kJacobiLdsSide];
    __shared__ uint32_t rotated;
    const uint32_t cells = L * L, m = L + L % 2, tid = threadIdx.x;
    double *A = lds_matrices, *V = lds_matrices + cells;
    for (uint32_t e = tid; e < cells; e += kBlock) A[e] = A_g[e], V[e] = e / L == e % L ? 1.0 : 0.0;
    if (tid == 0) rotated = 0;
    const double tol = gs[2];
    __syncthreads();
    uint32_t sweeps = 0, converged = 0;
    while (sweeps < kJacobiMaxSweeps && !converged) {  // (uniform: every lane reads the same counter)
        ++sweeps;
        for (uint32_t r = 0; r + 1 < m; ++r) {
            if (tid < m / 2) {  // every index below L is in exactly one pair of the round: partner[] is written whole
                uint32_t p, q;
                pair_of(m, r, tid, p, q);
                if (q >= L) {
                    partner[p] = kJacobiNone;
                } else {
                    double c = 1.0, s = 0.0;
                    const bool turn = rotation_of(A[p * L + p], A[q * L + q], A[p * L + q], tol, c, s);
                    partner[p] = turn ? q : kJacobiNone, partner[q] = turn ? p : kJacobiNone;
                    cs[p] = c, cs[q] = c, sn[p] = s, sn[q] = -s;
                    if (turn) atomicAdd(&rotated, 1u);
                }
            }
            __syncthreads();
            double a[kJacobiLdsHeld], v[kJacobiLdsHeld];
#pragma unroll
            for (uint32_t k = 0; k < kJacobiLdsHeld; ++k) {  // the column phase, into registers
                const uint32_t e = tid + k * kBlock;
                if (e >= cells) continue;
                const uint32_t i = e / L, j = e - i * L, jp = partner[j];
                a[k] = jp != kJacobiNone ? turned(cs[j], A[e], sn[j], A[i * L + jp]) : A[e];
                v[k] = jp != kJacobiNone ? turned(cs[j], V[e], sn[j], V[i * L + jp]) : V[e];
            }
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < kJacobiLdsHeld; ++k) {
                const uint32_t e = tid + k * kBlock;
                if (e < cells) A[e] = a[k], V[e] = v[k];
            }
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < kJacobiLdsHeld; ++k) {  // the row phase on (min, max): the mirror
                const uint32_t e = tid + k * kBlock;
                if (e >= cells) continue;
                const uint32_t i = e / L, j = e - i * L, lo = i < j ? i : j, hi = i < j ? j : i, lp = partner[lo];
                a[k] = lp == kJacobiNone ? A[lo * L + hi] : lp == hi ? 0.0 : turned(cs[lo], A[lo * L + hi], sn[lo], A[lp * L + hi]);
            }
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < kJacobiLdsHeld; ++k) {
                const uint32_t e = tid + k * kBlock;
                if (e < cells) A[e] = a[k];
            }
            __syncthreads();  // (and partner[] may be written again)
        }
        converged = rotated == 0 ? 1u : 0u;
        __syncthreads();
        if (tid == 0) rotated = 0;
        __syncthreads();
    }
    for (uint32_t e = tid; e < cells; e += kBlock) A_g[e] = A[e], V_g[e] = V[e];
    if (tid == 0) status[0] = sweeps, status[1] = converged;
}

__global__ __launch_bounds__(kBlock) void jacobi_params_kernel(const double *__restrict__ A, uint32_t L, uint32_t m, uint32_t r,
                                                               const double *__restrict__ gs, double *__restrict__ cs,
                                                               double *__restrict__ sn, uint32_t *__restrict__ partner,
                                                               uint32_t *__restrict__ counter)
{
    const double tol = gs[2];
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < m / 2; i += gridDim.x * kBlock) {
        uint32_t p, q;
        pair_of(m, r, i, p, q);
        if (q >= L) {
            partner[p] = kJacobiNone;
            continue;
        }
        double c = 1.0, s = 0.0;
        const bool turn = rotation_of(A[(uint64_t)p * L + p], A[(uint64_t)q * L + q], A[(uint64_t)p * L + q], tol, c, s);
        partner[p] = turn ? q : kJacobiNone, partner[q] = turn ? p : kJacobiNone;
        cs[p] = c, cs[q] = c, sn[p] = s, sn[q] = -s;
        if (turn) atomicAdd(counter, 1u);
    }
}

__global__ __launch_bounds__(kBlock) void jacobi_column_kernel(const double *__restrict__ A, double *__restrict__ A1,
                                                               double *__restrict__ V, uint32_t L, const double *__restrict__ cs,
                                                               const double *__restrict__ sn, const uint32_t *__restrict__ partner)
{
    const uint64_t cells = (uint64_t)L * L;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock) {
        const uint32_t i = (uint32_t)(e / L), j = (uint32_t)(e - (uint64_t)i * L), jp = partner[j];
        if (jp == kJacobiNone) {
            A1[e] = A[e];
            continue;
        }
        const uint64_t other = (uint64_t)i * L + jp;
        A1[e] = turned(cs[j], A[e], sn[j], A[other]);
        if (j < jp) {  // V in place: this lane owns both columns of the pair in row i
            const double vj = V[e], vp = V[other];
            V[e] = turned(cs[j], vj, sn[j], vp);
            V[other] = turned(cs[jp], vp, sn[jp], vj);
        }
    }
}

__global__ __launch_bounds__(kBlock) void jacobi_row_kernel(const double *__restrict__ A1, double *__restrict__ A, uint32_t L,
                                                            const double *__restrict__ cs, const double *__restrict__ sn,
                                                            const uint32_t *__restrict__ partner)
{
    const uint64_t cells = (uint64_t)L * L;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < cells; e += (uint64_t)gridDim.x * kBlock) {
        const uint32_t i = (uint32_t)(e / L), j = (uint32_t)(e - (uint64_t)i * L);
        const uint32_t lo = i < j ? i : j, hi = i < j ? j : i, lp = partner[lo];
        const uint64_t at = (uint64_t)lo * L + hi;
        A[e] = lp == kJacobiNone ? A1[at] : lp == hi ? 0.0 : turned(cs[lo], A1[at], sn[lo], A1[(uint64_t)lp * L + hi]);
    }
}

}  // namespace

namespace epik_amd {

// The sweeps of an L x L matrix on `stream`, L >= 1: with `lds` (L <= kJacobiLdsSide) one launch that leaves sweeps and
// converged in sp.status, the host's copies untouched; else the round-robin loop, one readback a sweep, `sweeps` and
// `converged` on return.  `cap`: the most workgroups of a launch.
int jacobi_sweeps(const JacobiSpace &sp, uint32_t L, bool lds, uint64_t cap, hipStream_t stream, uint32_t &sweeps,
                         uint32_t &converged)
{
    const uint64_t cells = (uint64_t)L * L;
    const uint32_t m = L + L % 2;
    if (lds) {
        const size_t lds_bytes = 2 * (size_t)cells * sizeof(double);
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&jacobi_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(2 * kJacobiLdsSide * kJacobiLdsSide * sizeof(double))));
        hipLaunchKernelGGL(jacobi_lds_kernel, dim3(1), dim3(kBlock), lds_bytes, stream, sp.A, sp.V, L, sp.gs, sp.status);
        HIP_TRY(hipGetLastError());
        return EPIK_AMD_OK;
    }
    const auto blocks = [&](uint64_t units) {
        return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(units + kBlock - 1) / kBlock, kJacobiMaxBlocks, cap})));
    };
    const dim3 pair_grid = blocks(m / 2), cell_grid = blocks(cells);
    sweeps = 0, converged = 0;
    while (sweeps < kJacobiMaxSweeps && !converged) {
        for (uint32_t r = 0; r + 1 < m; ++r) {
            hipLaunchKernelGGL(jacobi_params_kernel, pair_grid, dim3(kBlock), 0, stream, sp.A, L, m, r, sp.gs, sp.cs, sp.sn, sp.partner,
                               sp.counters + sweeps);
            hipLaunchKernelGGL(jacobi_column_kernel, cell_grid, dim3(kBlock), 0, stream, sp.A, sp.A1, sp.V, L, sp.cs, sp.sn, sp.partner);
            hipLaunchKernelGGL(jacobi_row_kernel, cell_grid, dim3(kBlock), 0, stream, sp.A1, sp.A, L, sp.cs, sp.sn, sp.partner);
        }
        HIP_TRY(hipGetLastError());
        uint32_t rotated = 0;  // the one readback of a sweep
        HIP_TRY(hipMemcpyAsync(&rotated, sp.counters + sweeps, sizeof rotated, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        ++sweeps;
        converged = rotated == 0 ? 1u : 0u;
    }
    return EPIK_AMD_OK;
}

}  // namespace epik_amd
