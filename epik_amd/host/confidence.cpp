#include "confidence.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <stdexcept>

// The rule of include/epik_amd.h, read by read and pair by pair, with the lca as a walk up parent[]: nothing here is
// shared with libepik_amd's tables or kernel but that text.  Built without contraction (Makefile: -ffp-contract=off):
// the EDPL's multiplies and adds are never fused.
namespace epik_amd {

namespace {

uint64_t q_of(double lwr) { return (uint64_t)std::llrint(lwr * (double)(1u << EPIK_AMD_PROFILE_LWR_BITS)); }

[[noreturn]] void bad_branch(size_t b, const std::string& what)
{
    throw std::runtime_error("branch " + std::to_string(b) + ": " + what);
}

const char* class_name(uint32_t clade)
{
    switch (clade) {
    case EPIK_AMD_CLADE_TOO_NARROW: return "too_narrow";
    case EPIK_AMD_CLADE_TOO_SHORT: return "too_short";
    case EPIK_AMD_CLADE_NO_HIT: return "no_hit";
    case EPIK_AMD_CLADE_BAD_ROW: return "bad_row";
    default: return nullptr;
    }
}

std::string in_output_dir(const std::string& prefix, const std::string& input_file, const std::string& output_dir)
{
    const auto slash = input_file.find_last_of('/');
    const std::string base = slash == std::string::npos ? input_file : input_file.substr(slash + 1);
    std::string dir = output_dir;
    if (!dir.empty() && dir.back() != '/') dir.push_back('/');
    return dir + prefix + base + ".tsv";
}

}  // namespace

confidence_tree::confidence_tree(std::vector<uint32_t> parents, std::vector<double> lengths)
    : parent(std::move(parents)), length(std::move(lengths))
{
    const size_t n = parent.size();
    if (n == 0 || length.size() != n) throw std::runtime_error("a tree has at least one branch, and a length for each");
    size.assign(n, 1);
    first.resize(n);
    std::vector<uint32_t> lowest(n);  // the lowest id among the descendants of b, b included
    for (size_t b = 0; b < n; ++b) lowest[b] = (uint32_t)b;
    for (size_t b = 0; b < n; ++b) {  // children come before their parent: size and lowest of b are final here
        if (!(length[b] >= 0.0) || !std::isfinite(length[b])) bad_branch(b, "the branch length is negative or not finite");
        if (b + 1 < n) {
            if (parent[b] == EPIK_AMD_TREE_NO_PARENT) bad_branch(b, "a second root");
            if (parent[b] <= b || parent[b] >= n) bad_branch(b, "the parent is not above its child");
        } else if (parent[b] != EPIK_AMD_TREE_NO_PARENT) {
            bad_branch(b, "the root has a parent");
        }
        first[b] = (uint32_t)b - size[b] + 1;
        if (lowest[b] != first[b]) bad_branch(b, "its descendants are no range of post-order ids");
        if (b + 1 < n) {
            size[parent[b]] += size[b];
            lowest[parent[b]] = std::min(lowest[parent[b]], lowest[b]);
        }
    }
    depth.assign(n, 0.0);
    mid.assign(n, 0.0);
    for (size_t b = n; b-- > 0;) {
        const double above = b + 1 < n ? depth[parent[b]] : 0.0;
        depth[b] = above + length[b];
        mid[b] = depth[b] - length[b] / 2;
    }
}

namespace {
std::vector<uint32_t> parents_of(const phylo_tree& tree)
{
    std::vector<uint32_t> out;
    for (const auto& node : tree.nodes()) out.push_back(node.parent < 0 ? EPIK_AMD_TREE_NO_PARENT : (uint32_t)node.parent);
    return out;
}
std::vector<double> lengths_of(const phylo_tree& tree)
{
    std::vector<double> out;
    for (const auto& node : tree.nodes()) out.push_back(node.branch_length);
    return out;
}
}  // namespace

confidence_tree::confidence_tree(const phylo_tree& tree) : confidence_tree(parents_of(tree), lengths_of(tree)) {}

uint32_t confidence_tree::lca(uint32_t a, uint32_t b) const noexcept
{
    const uint32_t lo = std::min(first[a], first[b]);
    uint32_t c = std::max(a, b);
    while (first[c] > lo) c = parent[c];
    return c;
}

double confidence_tree::distance(uint32_t a, uint32_t b) const noexcept
{
    if (a == b) return 0.0;
    if (inside(a, b)) return mid[a] - mid[b];
    if (inside(b, a)) return mid[b] - mid[a];
    const uint32_t c = lca(a, b);
    return (mid[a] - depth[c]) + (mid[b] - depth[c]);
}

uint32_t assign_tau_q(double tau)
{
    if (!(tau >= 0.0 && tau <= 1.0)) throw std::runtime_error("--assign-mass must lie in [0, 1]");
    return (uint32_t)std::llrint(tau * (double)(1u << EPIK_AMD_PROFILE_LWR_BITS));
}

epik_amd_confidence confidence_of(const confidence_tree& tree, const epik_amd_placement* rows, uint32_t n_rows,
                                  uint32_t first_count, uint32_t keep, uint32_t tau_q)
{
    epik_amd_confidence out{0, 0, 0.0};
    if (n_rows == EPIK_AMD_ROWS_COUNTS_TOO_NARROW) return out.clade = EPIK_AMD_CLADE_TOO_NARROW, out;
    if (n_rows == 0) return out.clade = EPIK_AMD_CLADE_TOO_SHORT, out;
    if (first_count == 0) return out.clade = EPIK_AMD_CLADE_NO_HIT, out;  // rows fabricated for a read without hits (place.cpp:141-152)
    const uint32_t nr = std::min(n_rows, keep);
    for (uint32_t j = 0; j < nr; ++j)
        if (rows[j].branch >= tree.num_branches()) return out.clade = EPIK_AMD_CLADE_BAD_ROW, out;
    // the shortest prefix of the rows that holds tau of the read's mass, in uint64
    uint64_t total = 0;
    for (uint32_t j = 0; j < nr; ++j) total += q_of(rows[j].lwr);
    uint32_t m = nr;
    uint64_t prefix = 0;
    for (uint32_t j = 0; j < nr; ++j) {
        prefix += q_of(rows[j].lwr);
        if ((prefix << EPIK_AMD_PROFILE_LWR_BITS) >= (uint64_t)tau_q * total) {
            m = j + 1;
            break;
        }
    }
    uint32_t clade = rows[0].branch;
    for (uint32_t j = 1; j < m; ++j) clade = tree.lca(clade, rows[j].branch);
    uint64_t mass = 0;
    for (uint32_t j = 0; j < nr; ++j)
        if (tree.inside(rows[j].branch, clade)) mass += q_of(rows[j].lwr);
    double sum = 0.0;
    for (uint32_t j = 0; j < nr; ++j)
        for (uint32_t l = j + 1; l < nr; ++l) {
            const double product = rows[j].lwr * rows[l].lwr;
            const double term = product * tree.distance(rows[j].branch, rows[l].branch);
            sum = sum + term;
        }
    out.clade = clade;
    out.clade_mass_q = mass > 0xffffffffull ? 0xffffffffu : (uint32_t)mass;
    out.edpl = 2.0 * sum;
    return out;
}

void confidence_rows(const confidence_tree& tree, const epik_amd_placement* rows, const uint32_t* n_rows,
                     const uint32_t* kmer_counts, uint64_t n, uint32_t keep, uint32_t tau_q, epik_amd_confidence* out)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = confidence_of(tree, rows + i * keep, n_rows[i], kmer_counts[i * keep], keep, tau_q);
}

void assign_summary::add(const epik_amd_confidence& record, uint64_t weight)
{
    switch (record.clade) {
    case EPIK_AMD_CLADE_TOO_NARROW: too_narrow += weight; break;
    case EPIK_AMD_CLADE_TOO_SHORT: too_short += weight; break;
    case EPIK_AMD_CLADE_NO_HIT: no_hit += weight; break;
    case EPIK_AMD_CLADE_BAD_ROW: bad_row += weight; break;
    default:
        if (record.clade >= assigned.size()) throw std::runtime_error("assign: a record names clade " + std::to_string(record.clade) + ", outside the tree");
        assigned[record.clade] += weight;
    }
}

uint64_t assign_summary::records() const noexcept
{
    uint64_t total = too_narrow + too_short + no_hit + bad_row;
    for (const uint64_t a : assigned) total += a;
    return total;
}

std::string make_assign_filename(const std::string& input_file, const std::string& output_dir)
{
    return in_output_dir("assign_", input_file, output_dir);
}

std::string make_assign_clades_filename(const std::string& input_file, const std::string& output_dir)
{
    return in_output_dir("assign_clades_", input_file, output_dir);
}

std::string format_assign_header(uint32_t tau_q, uint64_t records)
{
    return "# epik_amd assign v1\ttau_q=" + std::to_string(tau_q) + "\trecords=" + std::to_string(records) + "\n";
}

std::string format_assign_line(std::string_view name, const epik_amd_confidence& record, const confidence_tree& tree)
{
    char tail[128];
    if (const char* cls = class_name(record.clade)) {
        std::snprintf(tail, sizeof tail, "\t%s\t0\t%.9f\t%.17g\n", cls, 0.0, 0.0);
    } else {
        if (record.clade >= tree.num_branches()) throw std::runtime_error("assign: a record names clade " + std::to_string(record.clade) + ", outside the tree");
        std::snprintf(tail, sizeof tail, "\t%u\t%u\t%.9f\t%.17g\n", record.clade, tree.size[record.clade],
                      (double)record.clade_mass_q / (double)(1u << EPIK_AMD_PROFILE_LWR_BITS), record.edpl);
    }
    std::string out(name);
    return out += tail;
}

std::string format_assign_clades_tsv(const assign_summary& summary, const confidence_tree& tree, uint32_t tau_q)
{
    const size_t n = summary.assigned.size();
    if (tree.num_branches() != n) throw std::runtime_error("assign: the tree has another size than the summary");
    std::vector<uint64_t> prefix(n + 1, 0);  // the clade of b is the id range [first[b], b]
    for (size_t b = 0; b < n; ++b) prefix[b + 1] = prefix[b] + summary.assigned[b];
    char line[256];
    std::snprintf(line, sizeof line,
                  "# epik_amd assign_clades v1\ttau_q=%u\trecords=%llu\tassigned_records=%llu\ttoo_narrow=%llu\ttoo_short=%llu\tno_hit=%llu\tbad_row=%llu\n",
                  tau_q, (unsigned long long)summary.records(), (unsigned long long)prefix[n], (unsigned long long)summary.too_narrow,
                  (unsigned long long)summary.too_short, (unsigned long long)summary.no_hit, (unsigned long long)summary.bad_row);
    std::string out = line;
    out += "edge_num\tassigned\tclade_assigned\n";
    for (size_t b = 0; b < n; ++b) {
        std::snprintf(line, sizeof line, "%zu\t%llu\t%llu\n", b, (unsigned long long)summary.assigned[b],
                      (unsigned long long)(prefix[b + 1] - prefix[tree.first[b]]));
        out += line;
    }
    return out;
}

void write_text_file(const std::string& filename, const std::string& text)
{
    std::ofstream out(filename, std::ios::binary);
    out.write(text.data(), (std::streamsize)text.size());
    out.close();
    if (!out) throw std::runtime_error("Could not write " + filename);
}

}  // namespace epik_amd
