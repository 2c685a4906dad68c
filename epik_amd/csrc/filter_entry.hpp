// filter_entry.hpp -- what build_place.hip takes of filter_place.hip: the ranking of a CSR database that already lies
// on a device (epik_amd_builder_rank runs it on the builder's own arrays).  Internal to libepik_amd.
#ifndef EPIK_AMD_FILTER_ENTRY_HPP
#define EPIK_AMD_FILTER_ENTRY_HPP
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "epik_amd.h"

namespace epik_amd {

// device memory a handle keeps between calls: grown when a call needs more, freed by its owner (filter_scratch_free)
struct FilterScratch {
    void *base = nullptr;
    size_t bytes = 0;
};
int filter_scratch_reserve(FilterScratch &scratch, size_t bytes, hipStream_t stream);
void filter_scratch_free(FilterScratch &scratch);

// epik_amd_filter_rank_device once the device is known to exist: checks, value kernel, sort; returns after `stream` has
// drained.  d_value and d_order are device arrays [K].  The scratch of the call (20 bytes a key and hipCUB's own) is taken
// from `kept` when the caller has a handle to keep it on, and allocated for the call otherwise.
int filter_rank_on_device(int device, uint32_t num_branches, float log_thr, const uint32_t *d_keys, const uint64_t *d_offsets,
                          const epik_amd_pkdb_value *d_values, uint64_t K, uint32_t filter, uint64_t seed, double *d_value,
                          uint32_t *d_order, hipStream_t stream, FilterScratch *kept = nullptr);

}  // namespace epik_amd
#endif
