// build.hpp -- the rule of a phylo-k-mer database built from ancestral posteriors (include/epik_amd.h, "Building a
// phylo-k-mer database"), on the host: what epik_amd_build_host runs, and the checks and the pruning threshold that the
// device builder (csrc/build_place.hip) shares with it.  Plain C++, no device.
#ifndef EPIK_AMD_HOST_BUILD_HPP
#define EPIK_AMD_HOST_BUILD_HPP
#include <cstdint>
#include <string>
#include <vector>

#include "epik_amd.h"

namespace epik_amd {

constexpr uint32_t kBuildMaxK = 15;

// a finished database in the sparse CSR form
struct build_result {
    std::vector<uint32_t> keys;
    std::vector<uint64_t> offsets{0};
    std::vector<epik_amd_pkdb_value> values;
};

// (key, branch) in one word: the order of the result is the order of these
inline uint64_t build_pack(uint32_t key, uint32_t branch) { return (uint64_t)key << 32 | branch; }

// sigma, k, N and log_thr of a build: EPIK_AMD_OK, or EPIK_AMD_ERR_INVALID with `err`
int build_check_params(uint32_t sigma, uint32_t k, uint32_t num_branches, float log_thr, std::string &err);
// L of a chunk against k and the first chunk's (first_L 0: none yet)
int build_check_length(uint64_t L, uint32_t k, uint64_t first_L, std::string &err);
// the values of a host chunk: the first NaN or value above 0, the first branch_of[g] >= N
int build_check_chunk(const float *logp, const uint32_t *branch_of, uint64_t G, uint64_t L, uint32_t sigma,
                      uint32_t num_branches, std::string &err);
// the messages of those two, from the flat index of the value / the ghost node (the device builder finds them in a kernel)
std::string build_bad_value(uint64_t flat, uint64_t L, uint32_t sigma, float value);
std::string build_bad_branch(uint64_t g, uint32_t branch, uint32_t num_branches);

// the threshold of the cut: log_thr (1 + 16 k 2^-24), rounded away from 0
float build_prune_threshold(float log_thr, uint32_t k);

// the rule over one chunk on `num_threads` threads (0: one); the chunk has been checked
int build_rule_host(uint32_t sigma, uint32_t k, float log_thr, const float *logp, const uint32_t *branch_of, uint64_t G,
                    uint64_t L, uint32_t num_threads, build_result &out, std::string &err);

}  // namespace epik_amd
#endif
