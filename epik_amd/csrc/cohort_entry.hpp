// cohort_entry.hpp -- the host side that the cohort analyses share (cohort_place.hip and every *_place.hip of an analysis):
// the guard and the argument checks of the C entries, the grid clamp, the switch to an analysis' general path, the result
// buffer of a synchronous entry, the cohort's workspace slots, and the labels by column.  Host only; the device code they
// share is in cohort_device.hpp, the carver of a workspace in carve.hpp.
#ifndef EPIK_AMD_COHORT_ENTRY_HPP
#define EPIK_AMD_COHORT_ENTRY_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "carve.hpp"
#include "cohort_device.hpp"
#include "host_entry.hpp"

// a check or a step that returns a status: the entry returns the first that is not EPIK_AMD_OK
#define COHORT_TRY(expr)                                          \
    do {                                                          \
        if (const int rc_ = (expr); rc_ != EPIK_AMD_OK) return rc_; \
    } while (0)

// (internal to the library: what the compiler does not inline must not join the exported symbols)
#pragma GCC visibility push(hidden)
namespace epik_amd {

// A C entry's body: nothing may leave through the C ABI (std::vector, std::string), so an exception becomes
// EPIK_AMD_ERR_INVALID with the entry's name, e.g. guarded("cohort_permanova", [&]() -> int { ... }).
template <class Body>
int guarded(const char *name, Body body)
{
    try {
        return body();
    } catch (const std::exception &e) {
        return fail_with(EPIK_AMD_ERR_INVALID, std::string(name) + ": " + e.what());
    }
}

inline int check_cohort(const epik_amd_cohort *cohort)
{
    return cohort ? EPIK_AMD_OK : fail_with(EPIK_AMD_ERR_INVALID, "null cohort");
}
template <class... Pointers>
int check_present(const Pointers *...pointers)
{
    return (... && pointers) ? EPIK_AMD_OK : fail_with(EPIK_AMD_ERR_INVALID, "null argument");
}
// the columns of labels or metadata of a call: every analysis takes up to 64
inline int check_columns(uint32_t M)
{
    if (M < 1 || M > 64) return fail_with(EPIK_AMD_ERR_INVALID, "num_columns = " + std::to_string(M) + " is outside [1, 64]");
    return EPIK_AMD_OK;
}
inline int check_host_samples(uint32_t S)
{
    return S ? EPIK_AMD_OK : fail_with(EPIK_AMD_ERR_INVALID, "a cohort has at least one sample (num_samples is 0)");
}
// the shape of a _host entry's cells
inline int check_host_shape(uint32_t S, uint32_t N)
{
    COHORT_TRY(check_host_samples(S));
    return N ? EPIK_AMD_OK : fail_with(EPIK_AMD_ERR_INVALID, "a tree has at least one branch");
}
// an analysis of distances: the cohort's T_s must be those of the matrix
inline int check_has_distances(const epik_amd_cohort *cohort)
{
    if (cohort->d_total) return EPIK_AMD_OK;
    return fail_with(EPIK_AMD_ERR_INVALID, "the cohort has no distances yet: d_kr must be what kr_device wrote for this cohort");
}
// what a rule of epik_amd/host/cohort.hpp returned, with its message
inline int rule_result(int rc, const std::string &err) { return rc == EPIK_AMD_OK ? rc : fail_with(rc, err); }

// half[b] = 0.5 * branch_length[b] of the N branches; a length that is negative or not finite is refused
inline int half_branch_lengths(const double *branch_length, uint32_t N, std::vector<double> &half)
{
    half.resize(N);
    for (uint32_t b = 0; b < N; ++b) {
        if (!(branch_length[b] >= 0.0) || !std::isfinite(branch_length[b]))
            return fail_with(EPIK_AMD_ERR_INVALID, "branch " + std::to_string(b) + ": the branch length is negative or not finite");
        half[b] = 0.5 * branch_length[b];
    }
    return EPIK_AMD_OK;
}

// workgroups for `units` units of work: at least one, at most `most` and the placer's EPIK_AMD_MAX_BLOCKS (the kernels stride
// over the rest); the second form for units that a workgroup takes `per` of
inline dim3 cohort_grid(const epik_amd_cohort *cohort, uint64_t units, uint64_t most)
{
    const uint64_t cap = cohort->max_blocks_cap ? cohort->max_blocks_cap : ~0ull;
    return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({units, most, cap})));
}
inline dim3 cohort_grid_per(const epik_amd_cohort *cohort, uint64_t units, uint64_t per, uint64_t most)
{
    return cohort_grid(cohort, (units + per - 1) / per, most);
}

// EPIK_AMD_<ANALYSIS>_LDS=0 and the like (tests): read at every call, never latched
inline bool env_is_zero(const char *name)
{
    const char *env = std::getenv(name);
    return env && std::strcmp(env, "0") == 0;
}
// the LDS path of an analysis: up to `limit` samples or positions, unless the switch `name` forces the general path
inline bool lds_switch(const char *name, uint32_t S, uint32_t limit) { return S <= limit && !env_is_zero(name); }

// A result in device memory for a synchronous entry, freed after the device has drained, however the call ends.  An
// optional output that the caller did not ask for (wanted = false) is not allocated: d stays null, the device entry is
// handed the null pointer, and copy_to copies nothing.
struct DeviceResult {
    void *d = nullptr;
    DeviceResult() = default;
    DeviceResult(const DeviceResult &) = delete;
    DeviceResult &operator=(const DeviceResult &) = delete;
    ~DeviceResult()
    {
        if (d) (void)hipDeviceSynchronize(), (void)hipFree(d);
    }
    int alloc(size_t bytes, bool wanted = true)
    {
        if (wanted) HIP_TRY(hipMalloc(&d, bytes));
        return EPIK_AMD_OK;
    }
    int copy_to(void *host, size_t bytes, size_t offset = 0) const
    {
        if (d) HIP_TRY(hipMemcpy(host, static_cast<const char *>(d) + offset, bytes, hipMemcpyDeviceToHost));
        return EPIK_AMD_OK;
    }
    char *at(size_t offset) const { return static_cast<char *>(d) + offset; }
};

// The workspace `which` of the cohort with room for `bytes`: kept unless more is needed, else freed and allocated again
// (*fresh: whether it was, so its contents are undefined).  An analysis whose size never changes asks for that size at every
// call and is allocated once.  The caller has drained the device before: through hipDeviceSynchronize(), or through
// cohort_normalise_enqueue / cohort_mass_plane_enqueue, which do -- no earlier call still reads the buffer that is freed here,
// and nothing here synchronises.
inline int cohort_space_ensure(epik_amd_cohort *cohort, CohortSpaceId which, size_t bytes, bool *fresh = nullptr)
{
    CohortSpace &space = cohort->space[which];
    const bool grow = bytes > space.bytes;
    if (fresh) *fresh = grow;
    if (!grow) return EPIK_AMD_OK;
    (void)hipFree(space.d);
    space = CohortSpace{};
    HIP_TRY(hipMalloc(&space.d, bytes));
    space.bytes = bytes;
    return EPIK_AMD_OK;
}

// labels[S][M] by column into d_lab[M][padded] on the device, the padding `missing` (PERMANOVA, PERMDISP, the edge test)
inline int upload_labels_by_column(const uint32_t *labels, uint32_t S, uint32_t M, uint32_t padded, uint32_t missing, uint32_t *d_lab)
{
    std::vector<uint32_t> lab((size_t)M * padded, missing);
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t c = 0; c < M; ++c) lab[(size_t)c * padded + s] = labels[(size_t)s * M + c];
    HIP_TRY(hipMemcpy(d_lab, lab.data(), lab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return EPIK_AMD_OK;
}

// strata[S] (host; any uint32 is an id) into d_strata[padded] on the device, the padding 0: the strata rule's input by sample
inline int upload_strata(const uint32_t *strata, uint32_t S, uint32_t padded, uint32_t *d_strata)
{
    std::vector<uint32_t> h(padded, 0);
    std::copy(strata, strata + S, h.begin());
    HIP_TRY(hipMemcpy(d_strata, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return EPIK_AMD_OK;
}

// the most distinct labels (each below 32, or `missing`) of a column of labels[S][M]: a bound of the column's G; *distinct: of
// every column
inline uint32_t most_distinct_labels(const uint32_t *labels, uint32_t S, uint32_t M, uint32_t missing,
                                     std::vector<uint32_t> *distinct = nullptr)
{
    uint32_t most = 0;
    if (distinct) distinct->assign(M, 0);
    for (uint32_t c = 0; c < M; ++c) {
        uint32_t seen = 0;
        for (uint32_t s = 0; s < S; ++s)
            if (const uint32_t v = labels[(size_t)s * M + c]; v != missing) seen |= 1u << v;
        const uint32_t count = (uint32_t)__builtin_popcount(seen);
        most = std::max(most, count);
        if (distinct) (*distinct)[c] = count;
    }
    return most;
}

}  // namespace epik_amd
#pragma GCC visibility pop
#endif
