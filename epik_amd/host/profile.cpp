#include "profile.hpp"

#include <cmath>
#include <cstdio>
#include <fstream>
#include <stdexcept>

namespace epik_amd {

uint64_t profile_q(double lwr) { return (uint64_t)std::llrint(lwr * (double)(1u << EPIK_AMD_PROFILE_LWR_BITS)); }

namespace {

// one read of the rule: `row(j)` gives {branch, lwr} of its j-th row
template <typename Row>
void add_read(sample_profile& p, uint32_t n_rows, uint64_t first_count, uint32_t w, Row&& row)
{
    if (n_rows == EPIK_AMD_ROWS_COUNTS_TOO_NARROW) {
        p.totals.too_narrow += w;
    } else if (n_rows == 0) {
        p.totals.too_short += w;
    } else if (first_count == 0) {
        p.totals.no_hit += w;  // rows fabricated for a read without hits (place.cpp:141-152)
    } else {
        p.totals.placed += w;
        for (uint32_t j = 0; j < n_rows; ++j) {
            const auto [branch, lwr] = row(j);
            if (branch >= p.num_branches()) {
                ++p.totals.bad_rows;
                continue;
            }
            p.mass[branch] += (uint64_t)w * profile_q(lwr);
            if (j == 0) p.best[branch] += w;
        }
    }
}

}  // namespace

void sample_profile::add_rows(const epik_amd_placement* rows, const uint32_t* n_rows, const uint32_t* kmer_counts,
                              const uint32_t* weights, uint64_t n, uint32_t keep)
{
    for (uint64_t i = 0; i < n; ++i) {
        // (a row count beyond keep cannot name rows that exist: the rule looks at the read's keep slots only)
        const uint32_t nr = n_rows[i] == EPIK_AMD_ROWS_COUNTS_TOO_NARROW || n_rows[i] <= keep ? n_rows[i] : keep;
        add_read(*this, nr, kmer_counts[i * keep], weights ? weights[i] : 1u, [&](uint32_t j) {
            const auto& r = rows[i * keep + j];
            return std::pair<uint32_t, double>(r.branch, r.lwr);
        });
    }
}

void sample_profile::add(const impl::placed_batch& batch)
{
    for (size_t u = 0; u < batch.size(); ++u) {
        const uint32_t b = batch.row_begin[u], nr = batch.row_begin[u + 1] - b;
        add_read(*this, nr, nr ? batch.rows[b].count : 0, batch.name_begin[u + 1] - batch.name_begin[u], [&](uint32_t j) {
            const auto& r = batch.rows[b + j];
            return std::pair<uint32_t, double>(r.branch_id, r.weight_ratio);
        });
    }
}

void sample_profile::add_sums(const uint64_t* other_mass, const uint64_t* other_best, const epik_amd_profile_totals& t)
{
    for (size_t b = 0; b < mass.size(); ++b) mass[b] += other_mass[b], best[b] += other_best[b];
    totals.placed += t.placed, totals.no_hit += t.no_hit, totals.too_short += t.too_short;
    totals.too_narrow += t.too_narrow, totals.bad_rows += t.bad_rows;
}

std::vector<uint64_t> clade_sums(const std::vector<uint64_t>& per_branch, const std::vector<size_t>& subtree_num_nodes)
{
    const size_t n = per_branch.size();
    if (subtree_num_nodes.size() != n) throw std::runtime_error("profile: the tree index has another size than the profile");
    std::vector<uint64_t> prefix(n + 1, 0), out(n);
    for (size_t b = 0; b < n; ++b) prefix[b + 1] = prefix[b] + per_branch[b];
    for (size_t b = 0; b < n; ++b) {
        if (subtree_num_nodes[b] == 0 || subtree_num_nodes[b] > b + 1)
            throw std::runtime_error("profile: the subtree of branch " + std::to_string(b) + " is no range of post-order ids");
        out[b] = prefix[b + 1] - prefix[b + 1 - subtree_num_nodes[b]];
    }
    return out;
}

std::string make_profile_filename(const std::string& input_file, const std::string& output_dir)
{
    const auto slash = input_file.find_last_of('/');
    const std::string base = slash == std::string::npos ? input_file : input_file.substr(slash + 1);
    std::string dir = output_dir;
    if (!dir.empty() && dir.back() != '/') dir.push_back('/');
    return dir + "profile_" + base + ".tsv";
}

std::string format_profile_tsv(const sample_profile& p, const std::vector<size_t>& subtree_num_nodes)
{
    const auto clade_best = clade_sums(p.best, subtree_num_nodes), clade_mass = clade_sums(p.mass, subtree_num_nodes);
    const double scale = (double)(1u << EPIK_AMD_PROFILE_LWR_BITS);
    char line[256];
    std::snprintf(line, sizeof line, "# epik_amd profile v1\tlwr_bits=%d\trecords=%llu\tplaced=%llu\tno_hit=%llu\ttoo_short=%llu\n",
                  EPIK_AMD_PROFILE_LWR_BITS, (unsigned long long)p.records(), (unsigned long long)p.totals.placed,
                  (unsigned long long)p.totals.no_hit, (unsigned long long)p.totals.too_short);
    std::string out = line;
    out += "edge_num\tbest\tmass_q\tmass\tclade_best\tclade_mass_q\tclade_mass\n";
    for (size_t b = 0; b < p.num_branches(); ++b) {
        std::snprintf(line, sizeof line, "%zu\t%llu\t%llu\t%.9f\t%llu\t%llu\t%.9f\n", b, (unsigned long long)p.best[b],
                      (unsigned long long)p.mass[b], (double)p.mass[b] / scale, (unsigned long long)clade_best[b],
                      (unsigned long long)clade_mass[b], (double)clade_mass[b] / scale);
        out += line;
    }
    return out;
}

void write_profile_tsv(const std::string& filename, const sample_profile& profile, const std::vector<size_t>& subtree_num_nodes)
{
    const std::string text = format_profile_tsv(profile, subtree_num_nodes);
    std::ofstream out(filename, std::ios::binary);
    out.write(text.data(), (std::streamsize)text.size());
    out.close();
    if (!out) throw std::runtime_error("Could not write " + filename);
}

}  // namespace epik_amd
