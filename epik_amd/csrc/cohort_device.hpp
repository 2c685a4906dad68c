// cohort_device.hpp -- what cohort_place.hip, squash_place.hip, epca_place.hip, kmeans_place.hip, diversity_place.hip, correlation_place.hip and permanova_place.hip share of a device cohort: the object
// itself and the launch of the normalise and distance kernels (cohort_place.hip), which the squash clustering and the
// edge principal components start from.
#ifndef EPIK_AMD_COHORT_DEVICE_HPP
#define EPIK_AMD_COHORT_DEVICE_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "epik_amd.h"

struct epik_amd_cohort {
    int device = 0;
    uint32_t num_samples = 0, num_branches = 0, keep = 0;
    bool lds = false;             // latched at create(): the LDS path
    uint32_t lds_blocks = 0;      // ... and its grid: kMaxBlocks, or a workgroup per CU for the trees beyond kLdsBudget
    uint32_t max_blocks_cap = 0;  // the placer's EPIK_AMD_MAX_BLOCKS
    uint64_t *d_cells = nullptr;  // [S] x (mass[N] | best[N] | totals[kTotals]) | bad_samples
    // the workspace of the KR distance, allocated by the first kr_device:
    uint64_t *d_prefix = nullptr;  // [S][N]: inclusive prefix sums of mass
    uint64_t *d_total = nullptr;   // [S]: T_s
    double *d_planes = nullptr;    // C[N][Sp] | B[N][Sp]
    double *d_half = nullptr;      // [N]: 0.5 * branch_length
    // the workspace of the squash clustering, allocated by the first squash_device (squash_place.hip):
    void *d_squash = nullptr;
    // the workspace of the edge principal components, allocated by the first epca_device (epca_place.hip):
    void *d_epca = nullptr;
    // the workspace of the phylogenetic k-means, allocated by the first kmeans_device (kmeans_place.hip):
    void *d_kmeans = nullptr;
    // the workspace of the alpha diversity and the rarefaction curves (diversity_place.hip): the counts and the alpha
    // partials, allocated by the first alpha_device or rarefy_device; the curve's partials, for rarefy_depths depths
    void *d_diversity = nullptr;
    void *d_rarefy = nullptr;
    uint32_t rarefy_depths = 0;
    // the workspace of the edge correlation and dispersion, allocated by the first correlation_device or dispersion_device
    // (correlation_place.hip):
    void *d_correlation = nullptr;
    // the workspace of PERMANOVA, allocated by the first permanova_device and grown by a call that needs more
    // (permanova_place.hip):
    void *d_permanova = nullptr;
    size_t permanova_bytes = 0;
};

namespace epik_amd {

constexpr uint32_t kCohortTile = 32;  // samples a side of a tile of pairs: the planes' sample pitch is a multiple of it
inline uint32_t cohort_padded_samples(const epik_amd_cohort *cohort)
{
    return (cohort->num_samples + kCohortTile - 1) / kCohortTile * kCohortTile;
}

// the checks of the cohort and the tree (device, N), the device drained, the workspace of the planes, then the normalise
// kernel on `stream`: T_s in d_total, C and B in d_planes; *d_first: the tree's first[] on the device
int cohort_normalise_enqueue(epik_amd_cohort *cohort, const epik_amd_tree *tree, hipStream_t stream, const uint32_t **d_first);

// epik_amd_cohort_kr_device: the checks, the workspace, the lengths, then the normalise and distance kernels on `stream`
int cohort_kr_enqueue(epik_amd_cohort *cohort, const epik_amd_tree *tree, const double *branch_length, void *d_out,
                      hipStream_t stream);

}  // namespace epik_amd
#endif
