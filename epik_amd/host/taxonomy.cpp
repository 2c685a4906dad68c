// taxonomy.cpp -- see taxonomy.hpp.  The rule is stated once, in include/epik_amd.h; nothing here is floating point
// but q(), the profile's.
#include "taxonomy.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include <utility>

namespace epik_amd {

namespace {

constexpr uint32_t kLwrBits = EPIK_AMD_PROFILE_LWR_BITS;
constexpr uint32_t kNoParent = EPIK_AMD_TREE_NO_PARENT;

std::string strip(const std::string& s)
{
    const char* blanks = " \t\r\n\v\f";
    const size_t a = s.find_first_not_of(blanks);
    if (a == std::string::npos) return "";
    return s.substr(a, s.find_last_not_of(blanks) - a + 1);
}

int invalid(std::string& err, const std::string& what)
{
    err = what;
    return (int)EPIK_AMD_ERR_INVALID;
}

// a taxon of the trie while the file is read: std::map orders its children as unsigned bytes (char_traits<char>::lt)
struct Node {
    std::map<std::string, uint32_t> children;
    uint32_t parent = kNoParent;
    std::string name;
};

inline uint64_t q_of(double lwr) { return (uint64_t)std::llrint(lwr * (double)(1u << kLwrBits)); }

}  // namespace

int parse_taxonomy(std::istream& in, taxonomy& out, std::string& err)
{
    out = taxonomy{};
    std::vector<Node> nodes(1);  // (0: the root, while reading)
    std::vector<uint32_t> leaf_node;
    std::map<std::string, uint64_t> seen;
    std::string line;
    for (uint64_t number = 1; std::getline(in, line); ++number) {
        const std::string at = "line " + std::to_string(number) + ": ";
        if (strip(line).empty() || strip(line)[0] == '#') continue;
        const size_t tab = line.find('\t');
        if (tab == std::string::npos) return invalid(err, at + "no tab between the leaf label and the taxopath");
        const std::string leaf = strip(line.substr(0, tab)), whole = strip(line.substr(tab + 1));
        if (leaf.empty()) return invalid(err, at + "an empty leaf label");
        const auto known = seen.find(leaf);
        if (known != seen.end())
            return invalid(err, at + "leaf " + leaf + " is given twice (first on line " + std::to_string(known->second) + ")");
        seen.emplace(leaf, number);
        uint32_t node = 0;
        if (whole != "-") {
            size_t begin = 0;
            for (;;) {
                const size_t end = whole.find(';', begin);
                const std::string name = strip(whole.substr(begin, end == std::string::npos ? std::string::npos : end - begin));
                if (name.empty()) return invalid(err, at + "an empty element in the taxopath of leaf " + leaf);
                const auto child = nodes[node].children.find(name);
                if (child != nodes[node].children.end()) {
                    node = child->second;
                } else {
                    const uint32_t id = (uint32_t)nodes.size();
                    nodes[node].children.emplace(name, id);
                    nodes.emplace_back();
                    nodes.back().parent = node, nodes.back().name = name;
                    node = id;
                }
                if (end == std::string::npos) break;
                begin = end + 1;
            }
        }
        out.leaf.push_back(leaf), out.leaf_line.push_back(number), leaf_node.push_back(node);
    }
    // post-order ids, children in the map's order; no recursion: a chain may be long
    const uint32_t T = (uint32_t)nodes.size();
    std::vector<uint32_t> id(T, 0);
    out.parent.assign(T, kNoParent), out.first.assign(T, 0), out.path.assign(T, "");
    std::vector<std::pair<uint32_t, std::map<std::string, uint32_t>::const_iterator>> stack;
    std::vector<uint32_t> first_of(T, 0);
    uint32_t next = 0;
    stack.emplace_back(0u, nodes[0].children.begin());
    first_of[0] = 0;
    while (!stack.empty()) {
        auto& top = stack.back();
        const uint32_t node = top.first;
        if (top.second != nodes[node].children.end()) {
            const uint32_t child = top.second->second;
            ++top.second;
            first_of[child] = next;
            stack.emplace_back(child, nodes[child].children.begin());
            continue;
        }
        id[node] = next++;
        out.first[id[node]] = first_of[node];
        stack.pop_back();
    }
    for (uint32_t node = 1; node < T; ++node) out.parent[id[node]] = id[nodes[node].parent];
    std::vector<uint32_t> node_of(T);
    for (uint32_t node = 0; node < T; ++node) node_of[id[node]] = node;
    for (uint32_t t = T - 1; t-- > 0;) {  // from the root down: a parent's path is known before its children's
        const std::string& above = out.path[out.parent[t]];
        out.path[t] = above.empty() ? nodes[node_of[t]].name : above + ";" + nodes[node_of[t]].name;
    }
    out.leaf_taxon.resize(leaf_node.size());
    for (size_t k = 0; k < leaf_node.size(); ++k) out.leaf_taxon[k] = id[leaf_node[k]];
    return EPIK_AMD_OK;
}

int taxonomy_first(const uint32_t* parent, uint32_t n, const char* what, std::vector<uint32_t>& first, std::string& err)
{
    if (n == 0) return invalid(err, std::string("a taxonomy has at least one ") + what);
    std::vector<uint32_t> children(n, 0), stack;
    for (uint32_t b = 0; b + 1 < n; ++b)
        if (parent[b] != kNoParent && parent[b] > b && parent[b] < n) ++children[parent[b]];
    first.assign(n, 0);
    for (uint32_t b = 0; b < n; ++b) {
        const std::string at = std::string(what) + " " + std::to_string(b) + ": ";
        if (b + 1 < n) {
            if (parent[b] == kNoParent) return invalid(err, at + "a second root (only the last " + what + " has no parent)");
            if (parent[b] <= b || parent[b] >= n) return invalid(err, at + "the parent " + std::to_string(parent[b]) + " is not above its child");
        } else if (parent[b] != kNoParent) {
            return invalid(err, at + "the last " + what + " is the root and has no parent");
        }
        // post-order: the subtrees finished so far wait on a stack; the children of b are the ones on top
        uint32_t taken = 0, lowest = b;
        while (!stack.empty() && parent[stack.back()] == b) lowest = first[stack.back()], stack.pop_back(), ++taken;
        if (taken != children[b])
            return invalid(err, at + "its descendants are not exactly the post-order ids [" + std::to_string(lowest) + ", " + std::to_string(b) + "]");
        first[b] = lowest;
        stack.push_back(b);
    }
    return EPIK_AMD_OK;
}

int label_branches(const taxonomy& taxa, const uint32_t* parent, const std::vector<std::string>& names, uint32_t n,
                   std::vector<uint32_t>& label, std::string& err)
{
    const uint32_t T = taxa.num_taxa();
    std::vector<uint32_t> depth(T, 0);
    for (uint32_t t = T - 1; t-- > 0;) depth[t] = depth[taxa.parent[t]] + 1;
    // the longest common prefix of two taxa: the deeper one steps up to the other's depth, then both step together
    const auto common = [&](uint32_t a, uint32_t b) {
        while (depth[a] > depth[b]) a = taxa.parent[a];
        while (depth[b] > depth[a]) b = taxa.parent[b];
        while (a != b) a = taxa.parent[a], b = taxa.parent[b];
        return a;
    };
    std::vector<bool> inner(n, false);
    for (uint32_t b = 0; b + 1 < n; ++b)
        if (parent[b] < n) inner[parent[b]] = true;
    std::map<std::string, size_t> entry;
    for (size_t k = 0; k < taxa.leaf.size(); ++k) entry.emplace(taxa.leaf[k], k);
    std::vector<bool> used(taxa.leaf.size(), false);
    constexpr uint32_t kUnset = 0xffffffffu;
    label.assign(n, kUnset);
    for (uint32_t b = 0; b < n; ++b) {
        if (inner[b]) continue;
        const auto found = entry.find(names[b]);
        if (found == entry.end()) return invalid(err, "leaf " + names[b] + ": the taxonomy file does not give it");
        used[found->second] = true;
        label[b] = taxa.leaf_taxon[found->second];
    }
    for (size_t k = 0; k < used.size(); ++k)
        if (!used[k]) return invalid(err, "line " + std::to_string(taxa.leaf_line[k]) + ": " + taxa.leaf[k] + " is no leaf of the tree");
    for (uint32_t b = 0; b + 1 < n; ++b) {  // post-order: a child comes before its parent
        const uint32_t p = parent[b];
        label[p] = label[p] == kUnset ? label[b] : common(label[p], label[b]);
    }
    return EPIK_AMD_OK;
}

void groups_at_rank(const taxonomy& taxa, const std::vector<uint32_t>& label, uint32_t depth, std::vector<uint32_t>& group,
                    std::vector<uint32_t>& group_taxa)
{
    const uint32_t T = taxa.num_taxa();
    std::vector<uint32_t> deep(T, 0), at_depth(T, EPIK_AMD_WINDOW_NO_GROUP);  // at_depth[t]: the GROUP of t's ancestor there
    for (uint32_t t = T - 1; t-- > 0;) deep[t] = deep[taxa.parent[t]] + 1;
    group_taxa.clear();
    for (uint32_t t = 0; t < T; ++t)
        if (depth >= 1 && deep[t] == depth) at_depth[t] = (uint32_t)group_taxa.size(), group_taxa.push_back(t);
    for (uint32_t t = T - 1; t-- > 0;)  // (a parent has the larger id: it is done before its children)
        if (deep[t] > depth) at_depth[t] = at_depth[taxa.parent[t]];
    group.assign(label.size(), EPIK_AMD_WINDOW_NO_GROUP);
    for (size_t b = 0; b < label.size(); ++b)
        if (label[b] < T && depth >= 1 && deep[label[b]] >= depth) group[b] = at_depth[label[b]];
}

void taxa_assign(const uint32_t* taxon_parent, uint32_t num_taxa, const uint32_t* label,
                 uint32_t num_branches, uint32_t keep, const epik_amd_placement* rows, const uint32_t* n_rows,
                 const uint32_t* kmer_counts, const uint32_t* weights, const uint32_t* samples, uint64_t n, uint32_t tau_q,
                 epik_amd_taxon_record* records, taxa_cells* cells)
{
    // (mass(c) is summed up the parents here, not over [first[c], c] as the kernel does: the same set, found another way)
    __extension__ typedef unsigned __int128 u128;
    std::vector<uint64_t> mass(num_taxa, 0);  // mass(c) of the read at hand; zero again after it
    std::vector<uint32_t> touched, t(keep);
    std::vector<uint64_t> qs(keep);
    for (uint64_t i = 0; i < n; ++i) {
        const epik_amd_placement* row = rows + i * keep;
        uint32_t cls = 0, nr = 0;
        if (n_rows[i] == EPIK_AMD_ROWS_COUNTS_TOO_NARROW)
            cls = EPIK_AMD_TAXON_TOO_NARROW;
        else if (n_rows[i] == 0)
            cls = EPIK_AMD_TAXON_TOO_SHORT;
        else if (kmer_counts[i * keep] == 0)
            cls = EPIK_AMD_TAXON_NO_HIT;
        else {
            nr = std::min(n_rows[i], keep);
            for (uint32_t j = 0; j < nr; ++j)
                if (row[j].branch >= num_branches) cls = EPIK_AMD_TAXON_BAD_ROW;
        }
        uint64_t S = 0;
        if (!cls) {
            for (uint32_t j = 0; j < nr; ++j) t[j] = label[row[j].branch], qs[j] = q_of(row[j].lwr), S += qs[j];
            if (S == 0) cls = EPIK_AMD_TAXON_NO_MASS;
        }
        epik_amd_taxon_record rec{cls, 0, 0, 0};
        if (!cls) {
            touched.clear();
            for (uint32_t j = 0; j < nr; ++j)  // every row adds to its taxon and to all above it
                for (uint32_t c = t[j]; c != kNoParent; c = taxon_parent[c]) {
                    if (mass[c] == 0) touched.push_back(c);  // (twice where a row of q = 0 came first: harmless)
                    mass[c] += qs[j];
                }
            uint32_t best = num_taxa - 1;
            const u128 need = (u128)tau_q * S;
            for (const uint32_t c : touched)
                if (c < best && ((u128)mass[c] << kLwrBits) >= need) best = c;
            const uint64_t best_mass = mass[best];
            for (const uint32_t c : touched) mass[c] = 0;
            rec.taxon = best;
            rec.taxon_mass_q = best_mass > 0xffffffffull ? 0xffffffffu : (uint32_t)best_mass;
            rec.first_taxon = t[0];
            rec.total_q = S > 0xffffffffull ? 0xffffffffu : (uint32_t)S;
        }
        if (records) records[i] = rec;
        if (!cells) continue;
        const uint32_t smp = samples ? samples[i] : 0u;
        if (smp >= cells->samples) {
            ++cells->bad_samples;
            continue;
        }
        const uint64_t w = weights ? weights[i] : 1u;
        epik_amd_taxa_totals& tot = cells->totals[smp];
        if (!cls) {
            tot.placed += w;
            cells->assigned[(size_t)smp * num_taxa + rec.taxon] += w;
            for (uint32_t j = 0; j < nr; ++j) cells->direct[(size_t)smp * num_taxa + t[j]] += w * qs[j];
        } else if (cls == EPIK_AMD_TAXON_TOO_NARROW) {
            tot.too_narrow += w;
        } else if (cls == EPIK_AMD_TAXON_TOO_SHORT) {
            tot.too_short += w;
        } else if (cls == EPIK_AMD_TAXON_NO_HIT) {
            tot.no_hit += w;
        } else if (cls == EPIK_AMD_TAXON_NO_MASS) {
            tot.no_mass += w;
        } else {
            tot.bad_reads += 1;
        }
    }
}

std::vector<uint64_t> clade_sums(const uint64_t* cells, const uint32_t* first, uint32_t num_taxa)
{
    std::vector<uint64_t> prefix(num_taxa + 1, 0), out(num_taxa);
    for (uint32_t t = 0; t < num_taxa; ++t) prefix[t + 1] = prefix[t] + cells[t];
    for (uint32_t t = 0; t < num_taxa; ++t) out[t] = prefix[t + 1] - prefix[first[t]];
    return out;
}

namespace {

const std::string& path_or_dash(const taxonomy& taxa, uint32_t t)
{
    static const std::string dash = "-";
    return taxa.path[t].empty() ? dash : taxa.path[t];
}

std::string u64(uint64_t v) { return std::to_string((unsigned long long)v); }

}  // namespace

std::string format_taxa_tsv(const taxa_cells& cells, uint32_t sample, const taxonomy& taxa, uint32_t tau_q)
{
    const uint32_t T = taxa.num_taxa();
    const uint64_t *direct = cells.direct.data() + (size_t)sample * T, *assigned = cells.assigned.data() + (size_t)sample * T;
    const epik_amd_taxa_totals& t = cells.totals[sample];
    const auto clade_a = clade_sums(assigned, taxa.first.data(), T), clade_m = clade_sums(direct, taxa.first.data(), T);
    const double scale = (double)(1u << kLwrBits);
    std::string out = "# epik_amd taxa v1\ttau_q=" + std::to_string(tau_q) + "\ttaxa=" + std::to_string(T) + "\n";
    out += "# records=" + u64(t.placed + t.no_hit + t.too_short + t.too_narrow + t.no_mass) + "\tplaced=" + u64(t.placed) + "\tno_hit=" +
           u64(t.no_hit) + "\ttoo_short=" + u64(t.too_short) + "\ttoo_narrow=" + u64(t.too_narrow) + "\tno_mass=" + u64(t.no_mass) + "\n";
    out += "assigned\tclade_assigned\tmass_q\tclade_mass_q\tmass\tclade_mass\ttaxopath\n";
    char line[160];
    for (uint32_t c = 0; c < T; ++c) {
        if (clade_a[c] == 0 && clade_m[c] == 0) continue;
        std::snprintf(line, sizeof line, "%llu\t%llu\t%llu\t%llu\t%.9f\t%.9f\t", (unsigned long long)assigned[c], (unsigned long long)clade_a[c],
                      (unsigned long long)direct[c], (unsigned long long)clade_m[c], (double)direct[c] / scale, (double)clade_m[c] / scale);
        out += line + path_or_dash(taxa, c) + "\n";
    }
    return out;
}

std::string format_cohort_taxa_tsv(const std::vector<std::string>& names, const taxa_cells& cells, const taxonomy& taxa, uint32_t tau_q)
{
    const uint32_t T = taxa.num_taxa();
    std::string out = "# epik_amd cohort taxa v1\ttau_q=" + std::to_string(tau_q) + "\ttaxa=" + std::to_string(T) + "\tsamples=" +
                      std::to_string(names.size()) + "\n";
    out += "name\tassigned\tclade_assigned\tmass_q\tclade_mass_q\ttaxopath\n";
    for (size_t s = 0; s < names.size(); ++s) {
        const uint64_t *direct = cells.direct.data() + s * T, *assigned = cells.assigned.data() + s * T;
        const auto clade_a = clade_sums(assigned, taxa.first.data(), T), clade_m = clade_sums(direct, taxa.first.data(), T);
        for (uint32_t c = 0; c < T; ++c) {
            if (clade_a[c] == 0 && clade_m[c] == 0) continue;
            out += names[s] + "\t" + u64(assigned[c]) + "\t" + u64(clade_a[c]) + "\t" + u64(direct[c]) + "\t" + u64(clade_m[c]) + "\t" +
                   path_or_dash(taxa, c) + "\n";
        }
    }
    return out;
}

std::string format_taxa_reads_header(uint32_t tau_q, uint64_t records)
{
    return "# epik_amd taxa reads v1\ttau_q=" + std::to_string(tau_q) + "\trecords=" + u64(records) + "\nname\tshare\ttaxopath\tfirst_taxopath\n";
}

std::string format_taxa_reads_line(const std::string& name, const epik_amd_taxon_record& record, const taxonomy& taxa)
{
    const char* word = record.taxon == EPIK_AMD_TAXON_TOO_NARROW ? "too_narrow"
                       : record.taxon == EPIK_AMD_TAXON_TOO_SHORT ? "too_short"
                       : record.taxon == EPIK_AMD_TAXON_NO_HIT    ? "no_hit"
                       : record.taxon == EPIK_AMD_TAXON_BAD_ROW   ? "bad_row"
                       : record.taxon == EPIK_AMD_TAXON_NO_MASS   ? "no_mass"
                                                                  : nullptr;
    if (word) return name + "\t0\t" + word + "\t-\n";
    char share[40];
    std::snprintf(share, sizeof share, "%.17g", (double)record.taxon_mass_q / (double)record.total_q);
    return name + "\t" + share + "\t" + path_or_dash(taxa, record.taxon) + "\t" + path_or_dash(taxa, record.first_taxon) + "\n";
}

}  // namespace epik_amd
