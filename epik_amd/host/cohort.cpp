#include "cohort.hpp"

#include <cmath>
#include <cstdio>
#include <fstream>
#include <set>
#include <stdexcept>

namespace epik_amd {

namespace {

inline uint64_t cohort_q(double lwr) { return (uint64_t)std::llrint(lwr * (double)(1u << EPIK_AMD_PROFILE_LWR_BITS)); }

}  // namespace

void sample_cohort::add_rows(const epik_amd_placement* rows, const uint32_t* n_rows, const uint32_t* kmer_counts,
                             const uint32_t* weights, const uint32_t* samples, uint64_t n, uint32_t keep)
{
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t s = samples[i];
        if (s >= num_samples) {
            ++bad_samples;
            continue;
        }
        // the profile's rule (profile.cpp: add_read), on row s
        uint64_t* m = mass.data() + (size_t)s * num_branches;
        uint64_t* b = best.data() + (size_t)s * num_branches;
        auto& t = totals[s];
        const uint32_t w = weights ? weights[i] : 1u;
        const uint32_t nr = n_rows[i] == EPIK_AMD_ROWS_COUNTS_TOO_NARROW || n_rows[i] <= keep ? n_rows[i] : keep;
        if (nr == EPIK_AMD_ROWS_COUNTS_TOO_NARROW) {
            t.too_narrow += w;
        } else if (nr == 0) {
            t.too_short += w;
        } else if (kmer_counts[i * keep] == 0) {
            t.no_hit += w;
        } else {
            t.placed += w;
            for (uint32_t j = 0; j < nr; ++j) {
                const auto& r = rows[i * keep + j];
                if (r.branch >= num_branches) {
                    ++t.bad_rows;
                    continue;
                }
                m[r.branch] += (uint64_t)w * cohort_q(r.lwr);
                if (j == 0) b[r.branch] += w;
            }
        }
    }
}

void sample_cohort::add_cells(const uint64_t* other_mass, const uint64_t* other_best, const epik_amd_profile_totals* other_totals)
{
    const size_t cells = (size_t)num_samples * num_branches;
    if (other_mass)
        for (size_t c = 0; c < cells; ++c) mass[c] += other_mass[c];
    if (other_best)
        for (size_t c = 0; c < cells; ++c) best[c] += other_best[c];
    if (other_totals)
        for (uint32_t s = 0; s < num_samples; ++s) {
            totals[s].placed += other_totals[s].placed, totals[s].no_hit += other_totals[s].no_hit;
            totals[s].too_short += other_totals[s].too_short, totals[s].too_narrow += other_totals[s].too_narrow;
            totals[s].bad_rows += other_totals[s].bad_rows;
        }
}

void sample_cohort::merge(const sample_cohort& other)
{
    if (other.num_samples != num_samples || other.num_branches != num_branches)
        throw std::runtime_error("cohorts of different shapes");
    add_cells(other.mass.data(), other.best.data(), other.totals.data());
    bad_samples += other.bad_samples;
}

int kr_matrix(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
              const double* branch_length, double* out, std::string& err)
{
    const size_t S = num_samples, N = num_branches;
    for (size_t b = 0; b < N; ++b) {
        if (first[b] > b) {
            err = "branch " + std::to_string(b) + ": first[b] = " + std::to_string(first[b]) + " is above the branch";
            return EPIK_AMD_ERR_INVALID;
        }
        if (!(branch_length[b] >= 0.0) || !std::isfinite(branch_length[b])) {
            err = "branch " + std::to_string(b) + ": the branch length is negative or not finite";
            return EPIK_AMD_ERR_INVALID;
        }
    }
    // C[s][b], B[s][b]: one conversion each and one division; T_s == 0 leaves the row unused
    std::vector<double> C(S * N), B(S * N), half(N);
    std::vector<uint64_t> prefix(N + 1), total(S);
    for (size_t b = 0; b < N; ++b) half[b] = 0.5 * branch_length[b];
    for (size_t s = 0; s < S; ++s) {
        const uint64_t* m = mass + s * N;
        prefix[0] = 0;
        for (size_t b = 0; b < N; ++b) prefix[b + 1] = prefix[b] + m[b];
        total[s] = prefix[N];
        if (total[s] == 0) continue;
        const double T = (double)total[s];
        for (size_t b = 0; b < N; ++b) {
            const uint64_t clade = prefix[b + 1] - prefix[first[b]], below = clade - m[b];
            C[s * N + b] = (double)clade / T;
            B[s * N + b] = (double)below / T;
        }
    }
    for (size_t s = 0; s < S; ++s) {
        out[s * S + s] = 0.0;
        for (size_t t = s + 1; t < S; ++t) {
            double acc = -1.0;
            if (total[s] != 0 && total[t] != 0) {
                const double *cs = &C[s * N], *ct = &C[t * N], *bs = &B[s * N], *bt = &B[t * N];
                acc = 0.0;
                for (size_t b = 0; b < N; ++b) acc = acc + half[b] * (std::fabs(cs[b] - ct[b]) + std::fabs(bs[b] - bt[b]));
            }
            out[s * S + t] = out[t * S + s] = acc;
        }
    }
    return EPIK_AMD_OK;
}

std::vector<cohort_sample> read_cohort_list(const std::string& list_file)
{
    std::ifstream in(list_file);
    if (!in) throw std::runtime_error("--cohort: cannot open the list of samples " + list_file);
    const auto slash = list_file.find_last_of('/');
    const std::string dir = slash == std::string::npos ? std::string() : list_file.substr(0, slash + 1);
    std::vector<cohort_sample> samples;
    std::set<std::string> names;
    std::string line;
    for (size_t number = 1; std::getline(in, line); ++number) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        const std::string where = "--cohort: " + list_file + " line " + std::to_string(number) + ": ";
        const auto tab = line.find('\t');
        if (tab == std::string::npos) throw std::runtime_error(where + "not a name<TAB>path line");
        cohort_sample sample{line.substr(0, tab), line.substr(tab + 1)};
        if (sample.name.empty() || sample.path.empty() || sample.path.find('\t') != std::string::npos)
            throw std::runtime_error(where + "not a name<TAB>path line");
        if (!names.insert(sample.name).second) throw std::runtime_error(where + "the name '" + sample.name + "' is given twice");
        if (sample.path[0] != '/') sample.path = dir + sample.path;
        if (!std::ifstream(sample.path)) throw std::runtime_error(where + "cannot read " + sample.path);
        samples.push_back(std::move(sample));
    }
    if (samples.empty()) throw std::runtime_error("--cohort: " + list_file + " names no sample");
    return samples;
}

std::string make_cohort_filename(const std::string& what, const std::string& list_file, const std::string& output_dir)
{
    const auto slash = list_file.find_last_of('/');
    const std::string base = slash == std::string::npos ? list_file : list_file.substr(slash + 1);
    std::string dir = output_dir;
    if (!dir.empty() && dir.back() != '/') dir.push_back('/');
    return dir + "cohort_" + what + "_" + base + ".tsv";
}

std::string format_cohort_samples_tsv(const std::vector<cohort_sample>& samples, const sample_cohort& cohort)
{
    std::string out = "name\trecords\tplaced\tno_hit\ttoo_short\ttoo_narrow\ttotal_mass_q\n";
    for (size_t s = 0; s < samples.size(); ++s) {
        const auto& t = cohort.totals[s];
        uint64_t total = 0;
        for (size_t b = 0; b < cohort.num_branches; ++b) total += cohort.mass[s * cohort.num_branches + b];
        out += samples[s].name + '\t' + std::to_string(t.placed + t.no_hit + t.too_short + t.too_narrow) + '\t' +
               std::to_string(t.placed) + '\t' + std::to_string(t.no_hit) + '\t' + std::to_string(t.too_short) + '\t' +
               std::to_string(t.too_narrow) + '\t' + std::to_string(total) + '\n';
    }
    return out;
}

std::string format_cohort_profile_tsv(const std::vector<cohort_sample>& samples, const sample_cohort& cohort)
{
    std::string out = "name\tedge_num\tbest\tmass_q\n";
    for (size_t s = 0; s < samples.size(); ++s)
        for (size_t b = 0; b < cohort.num_branches; ++b) {
            const uint64_t m = cohort.mass[s * cohort.num_branches + b], best = cohort.best[s * cohort.num_branches + b];
            if (m == 0 && best == 0) continue;
            out += samples[s].name + '\t' + std::to_string(b) + '\t' + std::to_string(best) + '\t' + std::to_string(m) + '\n';
        }
    return out;
}

std::string format_cohort_kr_tsv(const std::vector<cohort_sample>& samples, const std::vector<double>& kr)
{
    const size_t S = samples.size();
    std::string out = "name";
    for (const auto& sample : samples) out += '\t' + sample.name;
    out += '\n';
    char text[40];
    for (size_t s = 0; s < S; ++s) {
        out += samples[s].name;
        for (size_t t = 0; t < S; ++t) {
            std::snprintf(text, sizeof text, "%.17g", kr[s * S + t]);
            out += '\t';
            out += text;
        }
        out += '\n';
    }
    return out;
}

void write_through_part(const std::string& filename, const std::string& text)
{
    const std::string part = filename + ".part";
    {
        std::ofstream out(part, std::ios::binary);
        out << text;
        out.close();
        if (!out) throw std::runtime_error("Could not write " + part);
    }
    if (std::rename(part.c_str(), filename.c_str()) != 0) throw std::runtime_error("Could not write " + filename);
}

}  // namespace epik_amd
