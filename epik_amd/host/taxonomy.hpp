// taxonomy.hpp -- taxonomic assignment on the host (include/epik_amd.h: epik_amd_taxonomy): the parser of the taxonomy
// file, the numbering of its taxa, the labels of the branches, and the rule of the records and the cells -- the mirror
// of taxa_place.hip, worded after the header and agreeing with it bit for bit.
// Needs nothing but the C header: libepik_amd compiles taxonomy.cpp too (epik_amd_taxonomy_assign_host is that code).
#ifndef EPIK_AMD_HOST_TAXONOMY_HPP
#define EPIK_AMD_HOST_TAXONOMY_HPP
#include <cstdint>
#include <istream>
#include <string>
#include <vector>

#include "epik_amd.h"

namespace epik_amd {

/// The taxa of a taxonomy file: post-order ids over the trie of the taxopaths, children in bytewise order of their names
struct taxonomy {
    std::vector<uint32_t> parent;       ///< [T]; EPIK_AMD_TREE_NO_PARENT for the root, T - 1
    std::vector<uint32_t> first;        ///< [T]: the clade of t is [first[t], t]
    std::vector<std::string> path;      ///< [T]: the taxopath, elements joined by ';'; "" for the root
    std::vector<std::string> leaf;      ///< the leaf labels of the file, in file order
    std::vector<uint32_t> leaf_taxon;   ///< ... their taxa
    std::vector<uint64_t> leaf_line;    ///< ... and their lines (from 1)
    uint32_t num_taxa() const { return (uint32_t)parent.size(); }
};

/// Reads a taxonomy file.  0, or EPIK_AMD_ERR_INVALID with `err` naming the line ("line <n>: ...").
int parse_taxonomy(std::istream& in, taxonomy& out, std::string& err);

/// first[] of a taxonomy given as parent[], with the checks, in the order and the words, of tree_build
/// (epik_amd/csrc/tree_tables.hpp), which libepik_amd itself uses for a taxonomy (taxa_place.hip).  That header is HIP
/// code (__host__ __device__, <hip/hip_runtime.h>), and this file is also built by plain g++ into the drivers and the
/// test programs, which have no ROCm headers: hence this copy.  tests/test_taxa_cpu.py holds the two to the same
/// refusals.  `what` is the word of the message ("taxon").  0, or EPIK_AMD_ERR_INVALID.
int taxonomy_first(const uint32_t* parent, uint32_t n, const char* what, std::vector<uint32_t>& first, std::string& err);

/// label[N] for the tree parent[N] (post-order ids, EPIK_AMD_TREE_NO_PARENT for the root) whose leaves -- the branches
/// without children -- are named names[b] (the names of inner branches are not looked at).  0, or EPIK_AMD_ERR_INVALID
/// with `err` naming the leaf ("leaf <name>: ...") or the line of the file.
int label_branches(const taxonomy& taxa, const uint32_t* parent, const std::vector<std::string>& names, uint32_t n,
                   std::vector<uint32_t>& label, std::string& err);

/// The groups painting by windows calls (include/epik_amd.h), cut at `depth` >= 1 elements of the taxopath: group[b] is
/// the depth-`depth` ancestor of label[b] when that label is at least so deep, else EPIK_AMD_WINDOW_NO_GROUP; group ids
/// number the taxa of that depth in ascending taxon id, group_taxa[g] the taxon of group g.
void groups_at_rank(const taxonomy& taxa, const std::vector<uint32_t>& label, uint32_t depth, std::vector<uint32_t>& group,
                    std::vector<uint32_t>& group_taxa);

/// The cells of `num_samples` samples over `num_taxa` taxa, and the rule that fills them
struct taxa_cells {
    taxa_cells() = default;
    taxa_cells(uint32_t num_samples, uint32_t num_taxa)
        : samples(num_samples), taxa(num_taxa), direct((size_t)num_samples * num_taxa, 0),
          assigned((size_t)num_samples * num_taxa, 0), totals(num_samples, epik_amd_taxa_totals{0, 0, 0, 0, 0, 0})
    {
    }
    uint32_t samples = 0, taxa = 0;
    std::vector<uint64_t> direct, assigned;  ///< [S][T]
    std::vector<epik_amd_taxa_totals> totals;
    uint64_t bad_samples = 0;
};

/// The rule over n reads: records[n] (may be null) and the adds into `cells` (may be null).  weights, samples: may be
/// null.  tau_q must lie in (2^29, 2^30] (not checked here).
void taxa_assign(const uint32_t* taxon_parent, uint32_t num_taxa, const uint32_t* label,
                 uint32_t num_branches, uint32_t keep, const epik_amd_placement* rows, const uint32_t* n_rows,
                 const uint32_t* kmer_counts, const uint32_t* weights, const uint32_t* samples, uint64_t n, uint32_t tau_q,
                 epik_amd_taxon_record* records, taxa_cells* cells);

/// clade[t] = the sum of cells[first[t] .. t], wrapping: differences of one prefix sum
std::vector<uint64_t> clade_sums(const uint64_t* cells, const uint32_t* first, uint32_t num_taxa);

/// taxa_<input>.tsv of one sample (row `sample` of `cells`): the header and totals lines, the column names, then a line
/// for every taxon whose clade has a non-zero cell, in id order; the root's taxopath is `-`
std::string format_taxa_tsv(const taxa_cells& cells, uint32_t sample, const taxonomy& taxa, uint32_t tau_q);

/// cohort_taxa_<list>.tsv: long format, list order, then taxon id, a line for every non-zero clade cell
std::string format_cohort_taxa_tsv(const std::vector<std::string>& names, const taxa_cells& cells, const taxonomy& taxa, uint32_t tau_q);

/// taxa_reads_<input>.tsv: its two head lines for `records` records, and the line of one record
std::string format_taxa_reads_header(uint32_t tau_q, uint64_t records);
std::string format_taxa_reads_line(const std::string& name, const epik_amd_taxon_record& record, const taxonomy& taxa);

}  // namespace epik_amd
#endif
