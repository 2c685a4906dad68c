// profile.hpp -- the abundance profile of a sample on the host: the rule of include/epik_amd.h (epik_amd_profile) over
// rows that are in host memory anyway (epik-dna --profile writes the jplace from them), the sum of profiles, the clade
// columns and the TSV.  libepik_amd's profile_kernel is the same rule on the device; both give the same bits.
// No reference counterpart: the reference leaves the sums over a jplace to a second tool.
#ifndef EPIK_AMD_HOST_PROFILE_HPP
#define EPIK_AMD_HOST_PROFILE_HPP

#include <cstdint>
#include <string>
#include <vector>

#include "epik_amd.h"
#include "placer.hpp"

namespace epik_amd {

/// q(x) = llrint(x * 2^EPIK_AMD_PROFILE_LWR_BITS), round half to even (the default rounding mode)
uint64_t profile_q(double lwr);

struct sample_profile {
    std::vector<uint64_t> mass;  // [num_branches]: sum of w * q(lwr) over the rows on the branch
    std::vector<uint64_t> best;  // [num_branches]: sum of w over the placed reads whose first row is on it
    epik_amd_profile_totals totals{};

    explicit sample_profile(size_t num_branches = 0) : mass(num_branches, 0), best(num_branches, 0) {}
    size_t num_branches() const noexcept { return mass.size(); }
    /// FASTA records behind the profile (every read falls in exactly one class)
    uint64_t records() const noexcept { return totals.placed + totals.no_hit + totals.too_short + totals.too_narrow; }

    /// n reads in the form of the C ABI: rows[n][keep], n_rows[n], kmer_counts[n][keep], weights[n] (nullptr: 1)
    void add_rows(const epik_amd_placement* rows, const uint32_t* n_rows, const uint32_t* kmer_counts,
                  const uint32_t* weights, uint64_t n, uint32_t keep);
    /// a placed batch of the driver: every unique sequence with the number of its records as weight
    void add(const impl::placed_batch& batch);
    /// what a device profile holds (epik_amd_profile_read), or another host profile: integer sums
    void add_sums(const uint64_t* other_mass, const uint64_t* other_best, const epik_amd_profile_totals& other_totals);
    void merge(const sample_profile& other) { add_sums(other.mass.data(), other.best.data(), other.totals); }
};

/// Sums over subtrees: with post-order ids the subtree of branch b is the id range [b - subtree_num_nodes[b] + 1, b]
/// (phylo_tree.hpp), so out[b] is a difference of the prefix sum of `per_branch`.  Throws on a size that is no such range.
std::vector<uint64_t> clade_sums(const std::vector<uint64_t>& per_branch, const std::vector<size_t>& subtree_num_nodes);

/// <output_dir>/profile_<basename(query)>.tsv
std::string make_profile_filename(const std::string& input_file, const std::string& output_dir);

/// "# epik_amd profile v1 ..." line, the column names, then one line per branch in id order; edge_num is the branch's
/// post-order id, the number the jplace carries for it (jplace.cpp: edge_num).  mass = mass_q / 2^30 as %.9f.
std::string format_profile_tsv(const sample_profile& profile, const std::vector<size_t>& subtree_num_nodes);
void write_profile_tsv(const std::string& filename, const sample_profile& profile,
                       const std::vector<size_t>& subtree_num_nodes);

}  // namespace epik_amd
#endif
