// jacobi_device.hpp -- what epca_place.hip and pcoa_place.hip take of the eigensolver (jacobi_place.hip): the cyclic Jacobi
// iteration in round-robin order of the edge-PCA rule (include/epik_amd.h), on a symmetric L x L matrix in device memory.  It
// knows nothing of what the matrix is: it takes the matrix, V and the workspace.
#ifndef EPIK_AMD_JACOBI_DEVICE_HPP
#define EPIK_AMD_JACOBI_DEVICE_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "epik_amd.h"

namespace epik_amd {

constexpr uint32_t kJacobiMaxSweeps = EPIK_AMD_JACOBI_MAX_SWEEPS;
constexpr uint32_t kJacobiLdsSide = 64;  // the LDS path: A and V of up to 64 x 64 doubles

// what the eigensolver takes: the matrix and V, and the workspace
struct JacobiSpace {
    double *A, *A1;       // [L][L] each: the matrix, and the matrix after the column phase
    double *V;            // [L][L]: the identity on entry (the LDS path sets it itself)
    double *cs, *sn;      // [L]: c_j, s_j of the round at hand
    const double *gs;     // gs[2] is tol
    uint32_t *partner;    // [L]: the eigensolver's own
    uint32_t *counters;   // [kJacobiMaxSweeps]: the rotations of a sweep, zero on entry (the global path)
    uint32_t *status;     // sweeps, converged (the LDS path)
};

// The sweeps of an L x L matrix on `stream`, L >= 1: with `lds` (L <= kJacobiLdsSide) one launch that leaves sweeps and
// converged in sp.status, the host's copies untouched; else the round-robin loop, one readback a sweep, `sweeps` and
// `converged` on return.  `cap`: the most workgroups of a launch.
int jacobi_sweeps(const JacobiSpace &sp, uint32_t L, bool lds, uint64_t cap, hipStream_t stream, uint32_t &sweeps,
                  uint32_t &converged);

}  // namespace epik_amd
#endif
