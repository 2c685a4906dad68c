// confidence.hpp -- per-read placement confidence on the host: the rule of include/epik_amd.h (epik_amd_tree,
// epik_amd_confidence) over rows in host memory, the tree of the rule from a phylo_tree, the per-clade sums of the records
// and the two TSVs of --assign.  libepik_amd's confidence_kernel is the same rule on the device; both give the same bits.
// The drivers take the records from the device; this mirror is what the CPU tests hold the rule against.
// No reference counterpart: the reference leaves EDPL and LCA assignment over a jplace to a second tool.
#ifndef EPIK_AMD_HOST_CONFIDENCE_HPP
#define EPIK_AMD_HOST_CONFIDENCE_HPP

#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

#include "epik_amd.h"
#include "phylo_tree.hpp"

namespace epik_amd {

/// The tree of the rule: N nodes with post-order ids, branch b joining node b to parent[b].
struct confidence_tree {
    std::vector<uint32_t> parent;  // EPIK_AMD_TREE_NO_PARENT for the root, as the C ABI takes it
    std::vector<double> length;
    std::vector<uint32_t> size;    // nodes of the subtree of b, b included
    std::vector<uint32_t> first;   // b - size[b] + 1: x lies in the clade of b <=> first[b] <= x <= b
    std::vector<double> depth;     // depth[parent[b]] + length[b], the root's parent at 0; one add each, from the root down
    std::vector<double> mid;       // depth[b] - length[b] / 2: where a placement on b sits

    /// Validates as epik_amd_tree_create does, in its order; throws std::runtime_error "branch <b>: ...".
    confidence_tree(std::vector<uint32_t> parents, std::vector<double> lengths);
    explicit confidence_tree(const phylo_tree& tree);

    size_t num_branches() const noexcept { return parent.size(); }
    bool inside(uint32_t x, uint32_t b) const noexcept { return first[b] <= x && x <= b; }
    /// the ancestor-or-self c of max(a, b), lowest in the tree, with first[c] <= min(first[a], first[b]): a walk up
    uint32_t lca(uint32_t a, uint32_t b) const noexcept;
    double distance(uint32_t a, uint32_t b) const noexcept;
    std::vector<size_t> subtree_num_nodes() const { return std::vector<size_t>(size.begin(), size.end()); }
};

/// --assign-mass as the rule takes it: llrint(tau * 2^30); throws unless tau lies in [0, 1]
uint32_t assign_tau_q(double tau);

/// The record of one read: its keep row slots, its n_rows and the k-mer count of its first slot.
epik_amd_confidence confidence_of(const confidence_tree& tree, const epik_amd_placement* rows, uint32_t n_rows,
                                  uint32_t first_count, uint32_t keep, uint32_t tau_q);
/// n reads in the form of the C ABI: rows[n][keep], n_rows[n], kmer_counts[n][keep] -> out[n]
void confidence_rows(const confidence_tree& tree, const epik_amd_placement* rows, const uint32_t* n_rows,
                     const uint32_t* kmer_counts, uint64_t n, uint32_t keep, uint32_t tau_q, epik_amd_confidence* out);

/// What assign_clades_<input>.tsv sums: the records assigned to each branch, and those of each class.
struct assign_summary {
    std::vector<uint64_t> assigned;  // [num_branches]
    uint64_t too_narrow = 0, too_short = 0, no_hit = 0, bad_row = 0;
    explicit assign_summary(size_t num_branches = 0) : assigned(num_branches, 0) {}
    /// a record standing for `weight` input records
    void add(const epik_amd_confidence& record, uint64_t weight);
    uint64_t records() const noexcept;
};

/// <output_dir>/assign_<basename(query)>.tsv and <output_dir>/assign_clades_<basename(query)>.tsv
std::string make_assign_filename(const std::string& input_file, const std::string& output_dir);
std::string make_assign_clades_filename(const std::string& input_file, const std::string& output_dir);

/// "# epik_amd assign v1<TAB>tau_q=...<TAB>records=..." and the line of one input record:
/// name, edge_num (the clade's post-order id, or too_narrow | too_short | no_hit | bad_row with zeros behind it),
/// clade_size, clade_mass = clade_mass_q / 2^30 as %.9f, edpl as %.17g.  Both end in a newline.
std::string format_assign_header(uint32_t tau_q, uint64_t records);
std::string format_assign_line(std::string_view name, const epik_amd_confidence& record, const confidence_tree& tree);
/// the header with the class totals, the column names, then edge_num, assigned, clade_assigned per branch in id order
std::string format_assign_clades_tsv(const assign_summary& summary, const confidence_tree& tree, uint32_t tau_q);
void write_text_file(const std::string& filename, const std::string& text);

}  // namespace epik_amd
#endif
