// cohort_run.hpp -- what the drivers do for --cohort and its analyses, in the four steps main() calls in this order:
// parse_cohort_options (every refusal of the command line, before anything is opened), read_inputs (the list and the side
// files, before the database or a device is touched), run_and_write (the request to placer::read_cohort and the files) and
// print_summary (the "Cohort ...:" lines of the report).  Every analysis is one row of kAnalyses (cohort_run.cpp).
#ifndef EPIK_AMD_HOST_COHORT_RUN_HPP
#define EPIK_AMD_HOST_COHORT_RUN_HPP

#include <array>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "cohort.hpp"
#include "placer.hpp"

namespace epik_amd {

/// The command line as the drivers parsed it: --name value pairs, a flag's value is "1"
struct options {
    std::map<std::string, std::string> values;
    std::vector<std::string> matrices;  // every --cohort-mantel-matrix, the one flag that may be repeated
    bool has(const std::string& k) const { return values.count(k) != 0; }
    std::string get(const std::string& k, const std::string& def) const
    {
        const auto it = values.find(k);
        return it == values.end() ? def : it->second;
    }
    std::string require(const std::string& k) const
    {
        const auto it = values.find(k);
        if (it == values.end()) throw std::runtime_error("Option '" + k + "' has no value");
        return it->second;
    }
};

/// The rows of kAnalyses, in the order of the summary lines
enum cohort_analysis : size_t {
    COHORT_SQUASH, COHORT_EPCA, COHORT_KMEANS, COHORT_ALPHA, COHORT_RAREFY, COHORT_CORRELATION, COHORT_DISPERSION, COHORT_PERMANOVA,
    COHORT_EDGETEST, COHORT_PERMDISP, COHORT_MANTEL, COHORT_ANOSIM, COHORT_MODEL, COHORT_EDGEMODEL, COHORT_PCOA, NUM_COHORT_ANALYSES
};

struct cohort_plan {
    bool with_cohort = false;
    std::array<bool, NUM_COHORT_ANALYSES> asked{};  ///< by row: a flag that asks for it (the Mantel test has two) is on the command line
    /// the analyses asked for, each with the numbers of its flags; run_and_write adds what read_inputs read
    placer::cohort_request request;

    void read_inputs(const std::string& query_file);
    void run_and_write(placer& devices, const std::string& query_file, const std::string& output_dir);
    void print_summary() const;

    std::vector<cohort_sample> samples;  ///< the list; empty without --cohort

private:
    friend cohort_plan parse_cohort_options(const options& parsed);
    std::string file_of(cohort_analysis analysis, size_t which = 0) const;
    std::string unifrac_file_of(uint32_t metric) const;

    options _parsed;
    cohort_metadata _metadata;
    std::vector<uint32_t> _strata;
    std::string _strata_name;
    cohort_factors _permanova_factors, _edgetest_factors, _permdisp_factors, _anosim_factors;
    cohort_mantel_sides _mantel_sides;
    cohort_design _model_design, _edgemodel_design;
    std::string _query_file, _output_dir;
    /// by row: the warning that follows its summary line; PERMDISP's clipped distances have always been told after the edge
    /// model's warning and before the principal coordinates, wherever those rows stand
    std::array<std::string, NUM_COHORT_ANALYSES> _warnings;
    std::string _permdisp_clipped_warning;
};

/// Every check of --cohort and the --cohort-* flags in their fixed order, ending with what --cohort does not work with;
/// throws std::runtime_error for the first that fails
cohort_plan parse_cohort_options(const options& parsed);

}  // namespace epik_amd
#endif
