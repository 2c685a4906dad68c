// ancestral.hpp -- ancestral posteriors of the ghost nodes of a reference tree (include/epik_amd.h, "Reconstructing
// ancestral posteriors"), on the host: what epik_amd_ancestral_host runs, the checks and the tree tables that the device
// handle (csrc/ancestral_place.hip) shares with it, and the model side (transition matrices, discrete-gamma rates),
// which is host-only and not under the bit-for-bit rule.  Plain C++, no device.
#ifndef EPIK_AMD_HOST_ANCESTRAL_HPP
#define EPIK_AMD_HOST_ANCESTRAL_HPP
#include <cstdint>
#include <string>
#include <vector>

#include "epik_amd.h"

namespace epik_amd {

constexpr uint32_t kAncestralMaxCategories = 8;
constexpr uint32_t kAncestralNone = 0xffffffffu;

// What follows from parent[] alone
struct ancestral_tree {
    uint32_t N = 0, n_leaves = 0, n_inner = 0;
    std::vector<uint32_t> left, right;  // per node its two children (kAncestralNone: a leaf)
    std::vector<uint32_t> sibling;      // per node but the root
    std::vector<uint32_t> leaf_row;     // per leaf its row of the masks: its rank among the leaves by node id
    std::vector<uint32_t> inner_slot;   // per inner node its rank among the inner nodes
    std::vector<std::vector<uint32_t>> down_levels;  // inner nodes by height, 1 first
    std::vector<std::vector<uint32_t>> up_levels;    // nodes but the root by depth, 1 first
};

// the descriptor's sizes, parent[], weights, frequencies and tables: EPIK_AMD_OK and `tree`, or EPIK_AMD_ERR_INVALID with `err`
int ancestral_check(const epik_amd_ancestral_desc &d, ancestral_tree &tree, std::string &err);
// L and the ghost choice of a call
int ancestral_check_call(const void *masks, uint64_t L, uint32_t ghosts, std::string &err);
// ghost nodes of a choice: N - 1, or 2 (N - 1) for both
inline uint64_t ancestral_ghost_count(uint32_t N, uint32_t ghosts) { return (uint64_t)(N - 1) * (ghosts == EPIK_AMD_GHOSTS_BOTH ? 2 : 1); }
// branch_of[G] of a choice: midpoints first, pendant nodes after them
void ancestral_branch_of(uint32_t N, uint32_t ghosts, uint32_t *branch_of);

// the rule over all sites on `num_threads` threads (0: one); everything has been checked
void ancestral_rule_host(const epik_amd_ancestral_desc &d, const ancestral_tree &tree, const uint32_t *masks, uint64_t L,
                         uint32_t ghosts, uint32_t num_threads, float *post, uint64_t *dead_sites);

// ---- the model side ---------------------------------------------------------------------------------------------------
// P(t) for every t of times[n] from the exchangeabilities (upper triangle, row by row) and the frequencies
int model_pmatrices(uint32_t sigma, const double *exchange, const double *pi, const double *times, uint64_t n, double *out,
                    std::string &err);
// the K category means of a gamma distribution of shape and rate alpha (Yang 1994)
int model_gamma_rates(double alpha, uint32_t K, double *rates, std::string &err);
// regularised lower incomplete gamma function P(a, x) and its inverse in x
double gamma_p(double a, double x);
double gamma_p_inverse(double a, double p);

}  // namespace epik_amd
#endif
