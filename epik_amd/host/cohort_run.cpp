#include "cohort_run.hpp"

#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <set>

namespace epik_amd {
namespace {

struct output_file {
    const char* stem = nullptr;  ///< make_cohort_filename's `what`; null: no such file
    const char* label = nullptr;  ///< what the summary calls it
    const char* extension = ".tsv";
};

/// One analysis of a cohort: how the command line asks for it, what it is refused with, what it writes and is called in
/// the summary.  The texts are frozen: they are what the drivers have always said.
struct analysis_row {
    const char* flag;                     ///< the flag that asks for it ...
    const char* also;                     ///< ... and a second one that does (the Mantel test's matrices), or null
    std::vector<const char*> dependents;  ///< the flags that need it
    const char* needs_cohort;             ///< the clause after "--<flag> needs --cohort "
    const char* dependent_needs;          ///< the clause after "--<dependent> needs --<flag> "; null: "(and that needs --cohort )" without --cohort
    output_file files[2];
    bool over_distance;  ///< runs over --cohort-distance
    bool permutes;       ///< permutes samples: within --cohort-strata
};

// in the order of cohort_analysis, which is the order of the summary lines
const analysis_row kAnalyses[NUM_COHORT_ANALYSES] = {
    {"cohort-squash", nullptr, {}, "(it clusters the samples of the list)", nullptr,
     {{"squash", "Cohort clustering"}, {"squash", "Cohort cluster tree", ".nwk"}}, false, false},
    {"cohort-epca", nullptr, {"cohort-epca-components"}, "(it takes the principal components of the samples of the list)",
     "(the flag that computes the components)", {{"epca", "Cohort principal components"}, {"epca_edges", "Cohort component edges"}},
     false, false},
    {"cohort-kmeans", nullptr, {"cohort-kmeans-iterations"}, "(it clusters the samples of the list)", "(the flag that clusters the samples)",
     {{"kmeans", "Cohort k-means"}, {"kmeans_centroids", "Cohort k-means centroids"}}, false, false},
    {"cohort-alpha", nullptr, {}, "(it measures the samples of the list)", nullptr, {{"alpha", "Cohort alpha diversity"}, {}}, false, false},
    {"cohort-rarefy", nullptr, {"cohort-rarefy-step"}, "(it rarefies the samples of the list)", "(the flag that computes the curves)",
     {{"rarefy", "Cohort rarefaction curves"}, {}}, false, false},
    {"cohort-correlation", nullptr, {}, "(it correlates the samples of the list with their metadata)", nullptr,
     {{"correlation", "Cohort edge correlation"}, {}}, false, false},
    {"cohort-dispersion", nullptr, {}, "(it measures the branches across the samples of the list)", nullptr,
     {{"dispersion", "Cohort edge dispersion"}, {}}, false, false},
    {"cohort-permanova", nullptr, {"cohort-permanova-permutations", "cohort-permanova-seed", "cohort-permanova-pairwise"},
     "(it tests the groups of the samples of the list)", nullptr, {{"permanova", "Cohort PERMANOVA"}, {}}, true, true},
    {"cohort-edge-test", nullptr, {"cohort-edge-test-permutations", "cohort-edge-test-seed"},
     "(it tests the branches between the groups of the samples of the list)", nullptr, {{"edgetest", "Cohort edge test"}, {}}, false, true},
    {"cohort-permdisp", nullptr, {"cohort-permdisp-permutations", "cohort-permdisp-seed", "cohort-permdisp-pairwise"},
     "(it tests the dispersions of the groups of the samples of the list)", nullptr, {{"permdisp", "Cohort PERMDISP"}, {}}, true, true},
    {"cohort-mantel", "cohort-mantel-matrix",
     {"cohort-mantel-method", "cohort-mantel-partial", "cohort-mantel-permutations", "cohort-mantel-seed"},
     "(it tests the distances between the samples of the list)", nullptr, {{"mantel", "Cohort Mantel"}, {}}, true, true},
    {"cohort-anosim", nullptr, {"cohort-anosim-permutations", "cohort-anosim-seed"}, "(it tests the distances between the samples of the list)",
     nullptr, {{"anosim", "Cohort ANOSIM"}, {}}, true, true},
    {"cohort-model", nullptr, {"cohort-model-terms", "cohort-model-permutations", "cohort-model-seed"},
     "(it fits a model of the samples of the list)", nullptr, {{"model", "Cohort model"}, {}}, true, true},
    {"cohort-edge-model", nullptr, {"cohort-edge-model-terms", "cohort-edge-model-permutations", "cohort-edge-model-seed"},
     "(it fits a model to the branches of the samples of the list)", nullptr, {{"edgemodel", "Cohort edge model"}, {}}, false, true},
    {"cohort-pcoa", nullptr, {"cohort-pcoa-components"}, "(it takes the principal coordinates of the samples of the list)",
     "(the flag that computes the coordinates)", {{"pcoa", "Cohort principal coordinates"}, {}}, true, false},
};

// ---- the two dialects of a number on the command line: what each accepts and how it words a refusal differ, and both stay ----

/// The std::stoul dialect (a leading blank or + passes): --flag, or `fallback` without it, a whole number in [1, most]
uint32_t whole_number(const options& parsed, const std::string& flag, const std::string& fallback, unsigned long most)
{
    const auto text = parsed.get(flag, fallback);
    size_t used = 0;
    unsigned long v = 0;
    try {
        v = std::stoul(text, &used);
    } catch (const std::exception&) {
        used = 0;
    }
    if (used != text.size() || used == 0 || text[0] == '-' || v < 1 || v > most)
        throw std::runtime_error("--" + flag + " must be a whole number in [1, " + std::to_string(most) + "], not '" + text + "'");
    return (uint32_t)v;
}

/// The strtoull dialect (a digit first, digits to the end): whether `text` is a uint64
bool digits_to_uint64(const std::string& text, uint64_t& v)
{
    if (text.empty() || text[0] < '0' || text[0] > '9') return false;
    char* end = nullptr;
    errno = 0;
    v = std::strtoull(text.c_str(), &end, 10);
    return !*end && errno != ERANGE;
}

constexpr uint32_t kMostPermutations = 999999;  // one cap for every test that permutes, as their messages say
static_assert(EPIK_AMD_PERMANOVA_MAX_PERMUTATIONS == kMostPermutations && EPIK_AMD_PERMDISP_MAX_PERMUTATIONS == kMostPermutations &&
                  EPIK_AMD_EDGETEST_MAX_PERMUTATIONS == kMostPermutations && EPIK_AMD_MODEL_MAX_PERMUTATIONS == kMostPermutations,
              "the tests' caps on the permutations differ: every --cohort-*-permutations needs its own");

/// --<flag>-permutations in [1, 999999] and --<flag>-seed, a uint64, into a test that has its defaults
void permutations_of(const options& parsed, const std::string& flag, placer::cohort_permutation_test& test)
{
    uint64_t v = 0;
    if (parsed.has(flag)) {
        const std::string text = parsed.require(flag);
        if (!digits_to_uint64(text, v) || v < 1 || v > kMostPermutations)
            throw std::runtime_error("--" + flag + " " + text + ": the number must lie in [1, 999999]");
        test.num_permutations = (uint32_t)v;
    }
}
void seed_of(const options& parsed, const std::string& flag, placer::cohort_permutation_test& test)
{
    if (parsed.has(flag)) {
        const std::string text = parsed.require(flag);
        if (!digits_to_uint64(text, test.seed)) throw std::runtime_error("--" + flag + " " + text + ": not a uint64");
    }
}
template <typename Test>
void permutation_test_of(const options& parsed, bool asked, const std::string& flag, std::optional<Test>& test)
{
    if (!asked) return;
    test.emplace();
    permutations_of(parsed, flag + "-permutations", *test);
    seed_of(parsed, flag + "-seed", *test);
}

void said_read(const char* what, const std::string& counts, size_t skipped)
{
    std::cout << "Cohort " << what << ": " << counts << ", " << skipped << " lines of samples that are not in the list skipped" << std::endl;
}

}  // namespace

cohort_plan parse_cohort_options(const options& parsed)
{
    cohort_plan plan;
    plan._parsed = parsed;
    const bool with_cohort = plan.with_cohort = parsed.has("cohort");
    auto& asked = plan.asked;
    auto& request = plan.request;
    for (size_t a = 0; a < NUM_COHORT_ANALYSES; ++a)
        asked[a] = parsed.has(kAnalyses[a].flag) || (kAnalyses[a].also && parsed.has(kAnalyses[a].also));
    const auto needs_cohort = [&](cohort_analysis a) {
        for (const char* flag : {kAnalyses[a].flag, kAnalyses[a].also})
            if (flag && parsed.has(flag) && !with_cohort)
                throw std::runtime_error(std::string("--") + flag + " needs --cohort " + kAnalyses[a].needs_cohort);
    };
    const auto dependents_need = [&](cohort_analysis a) {
        const auto& row = kAnalyses[a];
        for (const char* dependent : row.dependents)
            if (parsed.has(dependent) && !asked[a])
                throw std::runtime_error(std::string("--") + dependent + " needs --" + row.flag + (row.also ? std::string(" or --") + row.also : "") +
                                         (row.dependent_needs ? std::string(" ") + row.dependent_needs
                                          : with_cohort       ? ""
                                          : row.also          ? " (and they need --cohort )"
                                                              : " (and that needs --cohort )"));
    };
    const auto check = [&](cohort_analysis a) {
        needs_cohort(a);
        dependents_need(a);
    };
    // the checks stand in the order the drivers have always made them: the first fault of a command line is the one reported
    needs_cohort(COHORT_SQUASH);
    if (asked[COHORT_SQUASH]) request.squash.emplace();
    check(COHORT_EPCA);
    if (asked[COHORT_EPCA])
        request.epca.emplace().num_components = whole_number(parsed, "cohort-epca-components", "5", EPIK_AMD_EPCA_MAX_COMPONENTS);
    check(COHORT_PCOA);
    if (asked[COHORT_PCOA])
        request.pcoa.emplace().num_components = whole_number(parsed, "cohort-pcoa-components", "5", EPIK_AMD_PCOA_MAX_COMPONENTS);
    check(COHORT_KMEANS);
    if (asked[COHORT_KMEANS]) {
        request.kmeans.emplace().num_clusters = whole_number(parsed, "cohort-kmeans", "", EPIK_AMD_KMEANS_MAX_CLUSTERS);
        request.kmeans->max_iterations = whole_number(parsed, "cohort-kmeans-iterations", "100", EPIK_AMD_KMEANS_MAX_ITERATIONS);
    }
    check(COHORT_ALPHA);
    check(COHORT_RAREFY);
    if (asked[COHORT_ALPHA]) request.alpha.emplace();
    if (asked[COHORT_RAREFY]) {
        auto& rarefy = request.rarefy.emplace();
        const uint32_t deepest = whole_number(parsed, "cohort-rarefy", "", EPIK_AMD_RAREFY_MAX_DEPTH);
        rarefy.depth_step = std::max(1u, (deepest + 63) / 64);
        if (parsed.has("cohort-rarefy-step")) rarefy.depth_step = whole_number(parsed, "cohort-rarefy-step", "", EPIK_AMD_RAREFY_MAX_DEPTH);
        rarefy.num_depths = deepest / rarefy.depth_step;
        if (rarefy.num_depths < 1 || rarefy.num_depths > EPIK_AMD_RAREFY_MAX_DEPTHS)
            throw std::runtime_error("--cohort-rarefy-step " + std::to_string(rarefy.depth_step) + " gives floor(" + std::to_string(deepest) +
                                     " / " + std::to_string(rarefy.depth_step) + ") = " + std::to_string(rarefy.num_depths) +
                                     " depths of --cohort-rarefy: the number must lie in [1, 256]");
    }
    check(COHORT_CORRELATION);
    check(COHORT_DISPERSION);
    if (asked[COHORT_CORRELATION]) request.correlation.emplace();
    if (asked[COHORT_DISPERSION]) request.dispersion.emplace();
    check(COHORT_PERMANOVA);
    permutation_test_of(parsed, asked[COHORT_PERMANOVA], "cohort-permanova", request.permanova);
    if (asked[COHORT_PERMANOVA]) request.permanova->pairwise = parsed.has("cohort-permanova-pairwise");
    check(COHORT_PERMDISP);
    permutation_test_of(parsed, asked[COHORT_PERMDISP], "cohort-permdisp", request.permdisp);
    if (asked[COHORT_PERMDISP]) request.permdisp->pairwise = parsed.has("cohort-permdisp-pairwise");
    // (the Mantel test and ANOSIM came together: their checks interleave)
    needs_cohort(COHORT_MANTEL);
    needs_cohort(COHORT_ANOSIM);
    dependents_need(COHORT_MANTEL);
    dependents_need(COHORT_ANOSIM);
    if (asked[COHORT_MANTEL]) request.mantel.emplace();
    if (asked[COHORT_ANOSIM]) request.anosim.emplace();
    if (asked[COHORT_MANTEL]) permutations_of(parsed, "cohort-mantel-permutations", *request.mantel);
    if (asked[COHORT_ANOSIM]) permutations_of(parsed, "cohort-anosim-permutations", *request.anosim);
    if (asked[COHORT_MANTEL]) seed_of(parsed, "cohort-mantel-seed", *request.mantel);
    if (asked[COHORT_ANOSIM]) seed_of(parsed, "cohort-anosim-seed", *request.anosim);
    const uint32_t mantel_methods = mantel_methods_of_name(parsed.get("cohort-mantel-method", "pearson"));
    if (!mantel_methods)
        throw std::runtime_error("--cohort-mantel-method must be pearson, spearman or both, not '" + parsed.require("cohort-mantel-method") + "'");
    if (asked[COHORT_MANTEL]) request.mantel->methods = mantel_methods;
    for (const cohort_analysis a : {COHORT_MODEL, COHORT_EDGEMODEL}) {
        check(a);
        const std::string flag = kAnalyses[a].flag;
        if (asked[a] && !parsed.has(flag + "-terms"))
            throw std::runtime_error("--" + flag + " needs --" + flag + "-terms (the terms of the model, f:NAME or n:NAME, in test order)");
        if (a == COHORT_MODEL)
            permutation_test_of(parsed, asked[a], flag, request.model);
        else
            permutation_test_of(parsed, asked[a], flag, request.edgemodel);
    }
    // --cohort-unifrac / --cohort-distance / --cohort-strata.  The two guards read the table's columns and are what counts: their
    // messages, like the help text, name the analyses of the day they were written
    if (parsed.has("cohort-unifrac")) {
        if (!with_cohort)
            throw std::runtime_error("--cohort-unifrac needs --cohort (it takes the UniFrac distances between the samples of the list)");
        request.unifrac.emplace().metrics = parse_unifrac_list(parsed.require("cohort-unifrac"));
    }
    bool any_over_distance = false, any_permutes = false;
    for (size_t a = 0; a < NUM_COHORT_ANALYSES; ++a) {
        if (asked[a]) {
            any_over_distance |= kAnalyses[a].over_distance;
            any_permutes |= kAnalyses[a].permutes;
        }
    }
    if (parsed.has("cohort-distance")) {
        if (!any_over_distance)
            throw std::runtime_error("--cohort-distance needs --cohort-permanova, --cohort-pcoa or --cohort-permdisp (the analyses that "
                                     "run over a distance; --cohort-model is one too)");
        const std::string name = parsed.require("cohort-distance");
        request.distance = distance_of_name(name, true);
        if (request.distance == 0xffffffffu)
            throw std::runtime_error("--cohort-distance must be kr, unweighted, weighted or generalized, not '" + name + "'");
    }
    if (parsed.has("cohort-strata-column") && !parsed.has("cohort-strata"))
        throw std::runtime_error("--cohort-strata-column needs --cohort-strata (it names a column of that file)");
    if (parsed.has("cohort-strata") && !any_permutes)
        throw std::runtime_error("--cohort-strata needs --cohort-permanova, --cohort-permdisp, --cohort-edge-test or --cohort-model "
                                 "(the tests that permute samples)");
    check(COHORT_EDGETEST);
    permutation_test_of(parsed, asked[COHORT_EDGETEST], "cohort-edge-test", request.edgetest);
    if (with_cohort) {
        for (const char* other : {"mates", "profile-only", "profile", "assign"})
            if (parsed.has(other)) throw std::runtime_error(std::string("--cohort does not work with --") + other);
        if (std::stoul(parsed.get("db-shard", "1")) > 1)
            throw std::runtime_error("--cohort does not work with --db-shard > 1 (the rows of a sharded placement are finished "
                                     "on several devices)");
    }
    return plan;
}

std::string cohort_plan::file_of(cohort_analysis analysis, size_t which) const
{
    const auto& file = kAnalyses[analysis].files[which];
    return make_cohort_filename(file.stem, _query_file, _output_dir, file.extension);
}

std::string cohort_plan::unifrac_file_of(uint32_t metric) const
{
    return make_cohort_filename(std::string("unifrac_") + distance_name(metric), _query_file, _output_dir);
}

/// The list of samples and every side file, each error named by its line, before the database or a device is touched
void cohort_plan::read_inputs(const std::string& query_file)
{
    if (!with_cohort) return;
    _query_file = query_file;
    const auto columns = [](size_t n) { return std::to_string(n) + " columns"; };
    samples = read_cohort_list(query_file);
    if (asked[COHORT_CORRELATION]) {
        _metadata = read_cohort_metadata(_parsed.require("cohort-correlation"), samples);
        said_read("metadata", columns(_metadata.columns.size()), _metadata.skipped);
    }
    if (_parsed.has("cohort-strata")) {
        _strata = read_cohort_strata(_parsed.require("cohort-strata"), _parsed.get("cohort-strata-column", ""), samples, &_strata_name);
        std::cout << "Cohort strata: column " << _strata_name << ", " << std::set<uint32_t>(_strata.begin(), _strata.end()).size()
                  << " strata of " << _strata.size() << " samples" << std::endl;
    }
    // (the four factor files go through one reader, each with its own cap on the labels of a column and its flag in the messages)
    if (asked[COHORT_PERMANOVA]) {
        _permanova_factors = read_cohort_factors(_parsed.require("cohort-permanova"), samples, request.permanova->pairwise);
        said_read("factors", columns(_permanova_factors.columns.size()), _permanova_factors.skipped);
    }
    if (asked[COHORT_EDGETEST]) {
        _edgetest_factors =
            read_cohort_factors(_parsed.require("cohort-edge-test"), samples, false, EPIK_AMD_EDGETEST_MAX_GROUPS, "--cohort-edge-test");
        said_read("edge-test factors", columns(_edgetest_factors.columns.size()), _edgetest_factors.skipped);
    }
    if (asked[COHORT_PERMDISP]) {
        _permdisp_factors =
            read_cohort_factors(_parsed.require("cohort-permdisp"), samples, false, EPIK_AMD_PERMDISP_MAX_GROUPS, "--cohort-permdisp");
        said_read("PERMDISP factors", columns(_permdisp_factors.columns.size()), _permdisp_factors.skipped);
    }
    if (asked[COHORT_MANTEL]) {
        _mantel_sides = read_cohort_mantel_sides(_parsed.get("cohort-mantel", ""), _parsed.matrices, _parsed.get("cohort-mantel-partial", ""), samples);
        said_read("Mantel sides", columns(_mantel_sides.num_columns) + ", " + std::to_string(_mantel_sides.num_matrices) + " matrices",
                  _mantel_sides.skipped);
    }
    if (asked[COHORT_ANOSIM]) {
        _anosim_factors = read_cohort_factors(_parsed.require("cohort-anosim"), samples, false, 0, "--cohort-anosim");
        said_read("ANOSIM factors", columns(_anosim_factors.columns.size()), _anosim_factors.skipped);
    }
    if (asked[COHORT_MODEL]) {
        _model_design = read_cohort_design(_parsed.require("cohort-model"), _parsed.require("cohort-model-terms"), samples);
        said_read("model design", std::to_string(_model_design.terms.size()) + " terms", _model_design.skipped);
    }
    if (asked[COHORT_EDGEMODEL]) {  // (the same file may serve --cohort-model)
        _edgemodel_design = read_cohort_design(_parsed.require("cohort-edge-model"), _parsed.require("cohort-edge-model-terms"), samples);
        said_read("edge model design", std::to_string(_edgemodel_design.terms.size()) + " terms", _edgemodel_design.skipped);
    }
}

/// The handles' cohorts summed on the first device, read once, every analysis computed there, and the files written
void cohort_plan::run_and_write(placer& devices, const std::string& query_file, const std::string& output_dir)
{
    if (!with_cohort) return;
    _query_file = query_file, _output_dir = output_dir;
    auto& r = request;
    r.strata = _parsed.has("cohort-strata") ? _strata.data() : nullptr;
    const auto factors_into = [](auto& test, const cohort_factors& factors) {
        if (test) test->labels = factors.labels.data(), test->num_columns = (uint32_t)factors.columns.size();
    };
    const auto design_into = [](auto& test, const cohort_design& design) {
        if (!test) return;
        test->kind = design.kind.data(), test->labels = design.labels.data(), test->values = design.values.data();
        test->num_terms = (uint32_t)design.terms.size();
    };
    if (r.correlation) r.correlation->meta = _metadata.values.data(), r.correlation->num_columns = (uint32_t)_metadata.columns.size();
    factors_into(r.permanova, _permanova_factors), factors_into(r.edgetest, _edgetest_factors);
    factors_into(r.permdisp, _permdisp_factors), factors_into(r.anosim, _anosim_factors);
    design_into(r.model, _model_design), design_into(r.edgemodel, _edgemodel_design);
    if (r.mantel) {
        auto& m = *r.mantel;
        m.values = _mantel_sides.values.data(), m.matrices = _mantel_sides.matrices.data(), m.present = _mantel_sides.present.data();
        m.num_columns = _mantel_sides.num_columns, m.num_matrices = _mantel_sides.num_matrices, m.control = _mantel_sides.control;
    }
    devices.read_cohort(r);

    const sample_cohort& cohort = r.cells;
    const uint32_t N = cohort.num_branches;
    // (T_s and n_s, the sums wrapping as the rule's: what the files take; a sample is live with T_s > 0)
    std::vector<uint64_t> mass_of(samples.size(), 0), reads(samples.size(), 0);
    std::vector<char> live(samples.size());
    for (size_t s = 0; s < samples.size(); ++s) {
        for (size_t b = 0; b < N; ++b) mass_of[s] += cohort.mass[s * N + b], reads[s] += cohort.best[s * N + b];
        live[s] = mass_of[s] != 0;
    }
    const uint64_t* const totals = mass_of.data();
    // a test's file says on its first line which strata its permutations stayed within
    const auto write_test = [&](cohort_analysis a, const std::string& text) {
        write_through_part(file_of(a), with_strata_field(text, _strata_name));
    };
    // a factor that is constant inside every stratum of its used samples: no permutation changes anything, p = 1
    const auto warn_nested = [&](cohort_analysis a, const cohort_factors& factors, uint32_t missing) {
        for (size_t c = 0; r.strata && c < factors.columns.size(); ++c)
            if (constant_within_strata(factors.labels.data(), samples.size(), factors.columns.size(), c, missing, totals, r.strata))
                std::cout << "Warning: --" << kAnalyses[a].flag << ": the column " << factors.columns[c]
                          << " is constant inside every stratum of " << _strata_name << ": no permutation can change it, p = 1" << std::endl;
    };
    const auto not_converged = [&](cohort_analysis a, const char* what, uint32_t most, const char* unit) {
        _warnings[a] = std::string("Warning: the ") + what + " did not converge in " + std::to_string(most) + " " + unit +
                       " (converged=0 in " + file_of(a) + ")\n";
    };
    const auto aliased_columns = [&](cohort_analysis a, const std::vector<uint8_t>& aliased, const char* whose) {
        size_t dropped = 0;
        for (const uint8_t byte : aliased) dropped += byte;
        if (dropped)
            _warnings[a] = "Warning: " + std::to_string(dropped) + " columns of the " + whose + " are explained by the columns before them and " +
                           "were dropped (the # aliased lines of " + file_of(a) + ")\n";
    };

    if (r.unifrac)
        for (size_t i = 0; i < r.unifrac->metrics.size(); ++i)
            write_through_part(unifrac_file_of(r.unifrac->metrics[i]), format_cohort_unifrac_tsv(samples, r.unifrac->matrix[i]));
    write_through_part(make_cohort_filename("samples", query_file, output_dir), format_cohort_samples_tsv(samples, cohort));
    write_through_part(make_cohort_filename("profile", query_file, output_dir), format_cohort_profile_tsv(samples, cohort));
    write_through_part(make_cohort_filename("kr", query_file, output_dir), format_cohort_kr_tsv(samples, r.kr));
    if (r.epca) {
        const auto& t = *r.epca;
        write_through_part(file_of(COHORT_EPCA), format_epca_tsv(samples, live, t.num_components, t.mu.data(), t.proj.data(), t.info));
        write_through_part(file_of(COHORT_EPCA, 1), format_epca_edges_tsv(t.first, t.edge.data(), t.info));
        if (!t.info.converged) not_converged(COHORT_EPCA, "edge principal components", EPIK_AMD_EPCA_MAX_SWEEPS, "sweeps");
    }
    if (r.kmeans) {
        const auto& t = *r.kmeans;
        write_through_part(file_of(COHORT_KMEANS), format_kmeans_tsv(samples, t.samples.data(), t.clusters.data(), t.info));
        write_through_part(file_of(COHORT_KMEANS, 1), format_kmeans_centroids_tsv(t.centroids.data(), N, t.info));
        if (!t.info.converged) not_converged(COHORT_KMEANS, "phylogenetic k-means", t.max_iterations, "iterations");
    }
    if (r.alpha) write_through_part(file_of(COHORT_ALPHA), format_alpha_tsv(samples, r.alpha->alpha.data()));
    if (r.rarefy)
        write_through_part(file_of(COHORT_RAREFY),
                           format_rarefy_tsv(samples, reads.data(), r.rarefy->depth_step, r.rarefy->num_depths, r.rarefy->curve.data()));
    if (r.correlation)
        write_through_part(file_of(COHORT_CORRELATION), format_correlation_tsv(samples, totals, _metadata.columns, N, r.correlation->correlation.data(),
                                                                        r.correlation->used.data()));
    if (r.dispersion) write_through_part(file_of(COHORT_DISPERSION), format_dispersion_tsv(samples, totals, N, r.dispersion->dispersion.data()));
    if (r.permanova) {
        const auto& t = *r.permanova;
        const auto& f = _permanova_factors;
        write_test(COHORT_PERMANOVA, format_permanova_tsv(samples, totals, f.columns, f.names, f.labels.data(), t.num_permutations, t.seed, t.pairwise,
                                                   t.records.data(), t.group_ss.data(), r.distance));
        warn_nested(COHORT_PERMANOVA, f, EPIK_AMD_PERMANOVA_MISSING);
    }
    if (r.edgetest) {
        const auto& t = *r.edgetest;
        const auto& f = _edgetest_factors;
        write_test(COHORT_EDGETEST,
                   format_edgetest_tsv(samples, totals, f.columns, f.names, f.labels.data(), N, t.num_permutations, t.seed, t.records.data()));
        warn_nested(COHORT_EDGETEST, f, EPIK_AMD_EDGETEST_MISSING);
    }
    uint64_t permdisp_clipped = 0;
    if (r.permdisp) {
        const auto& t = *r.permdisp;
        const auto& f = _permdisp_factors;
        write_test(COHORT_PERMDISP, format_permdisp_tsv(samples, totals, f.columns, f.names, f.labels.data(), t.num_permutations, t.seed, t.pairwise,
                                                 t.records.data(), t.group_mean.data(), t.z.data(), r.distance));
        warn_nested(COHORT_PERMDISP, f, EPIK_AMD_PERMDISP_MISSING);
        const size_t slots = t.records.size() / f.columns.size();
        for (size_t c = 0; c < f.columns.size(); ++c) permdisp_clipped += t.records[c * slots].clipped;
    }
    if (r.mantel) {
        const auto& t = *r.mantel;
        write_test(COHORT_MANTEL, format_mantel_tsv(samples, totals, _mantel_sides.names, t.num_columns, t.methods, t.control, t.num_permutations,
                                             t.seed, t.records.data(), r.distance));
    }
    if (r.anosim) {
        const auto& t = *r.anosim;
        const auto& f = _anosim_factors;
        write_test(COHORT_ANOSIM, format_anosim_tsv(samples, totals, f.columns, f.names, f.labels.data(), t.num_permutations, t.seed, t.records.data(),
                                             r.distance));
        warn_nested(COHORT_ANOSIM, f, EPIK_AMD_PERMANOVA_MISSING);
    }
    if (r.model) {
        const auto& t = *r.model;
        const auto& design = _model_design;
        write_test(COHORT_MODEL, format_model_tsv(samples, totals, design, t.num_permutations, t.seed, t.records.data(), t.info, t.aliased.data(),
                                           r.distance));
        // (the model's used samples are the complete cases)
        const size_t T = design.terms.size();
        std::vector<uint64_t> complete(mass_of);
        for (size_t s = 0; s < complete.size(); ++s)
            for (size_t k = 0; k < T; ++k)
                if (design.kind[k] ? std::isnan(design.values[s * T + k]) : design.labels[s * T + k] == EPIK_AMD_MODEL_MISSING) complete[s] = 0;
        for (size_t k = 0; r.strata && k < T; ++k)
            if (!design.kind[k] &&
                constant_within_strata(design.labels.data(), complete.size(), T, k, EPIK_AMD_MODEL_MISSING, complete.data(), r.strata))
                std::cout << "Warning: --cohort-model: the term " << design.terms[k] << " is constant inside every stratum of " << _strata_name
                          << ": no permutation changes its sum of squares" << std::endl;
        aliased_columns(COHORT_MODEL, t.aliased, "design");
    }
    if (r.edgemodel) {
        const auto& t = *r.edgemodel;
        write_test(COHORT_EDGEMODEL, format_edgemodel_tsv(samples, totals, _edgemodel_design, N, t.num_permutations, t.seed, t.records.data(), t.info,
                                                   t.aliased.data()));
        aliased_columns(COHORT_EDGEMODEL, t.aliased, "edge model's design");
    }
    if (permdisp_clipped)
        _permdisp_clipped_warning = "Warning: " + std::to_string(permdisp_clipped) + " squared distances to a group centroid are negative (the " +
                                    (r.distance == EPIK_AMD_DISTANCE_KR ? "KR" : distance_name(r.distance)) +
                                    " distance is not Euclidean) and count as zero (the clipped column of " + file_of(COHORT_PERMDISP) + ")\n";
    if (r.pcoa) {
        const auto& t = *r.pcoa;
        write_through_part(file_of(COHORT_PCOA), format_pcoa_tsv(samples, totals, t.num_components, t.mu.data(), t.coord.data(), t.info, r.distance));
        if (!t.info.converged) not_converged(COHORT_PCOA, "principal coordinates", EPIK_AMD_PCOA_MAX_SWEEPS, "sweeps");
    }
    if (r.squash) {
        const auto& t = *r.squash;
        write_through_part(file_of(COHORT_SQUASH), format_squash_tsv(samples, live, t.merges.data(), t.num_merges));
        write_through_part(file_of(COHORT_SQUASH, 1), format_squash_newick(samples, live, t.merges.data(), t.num_merges));
    }
}

void cohort_plan::print_summary() const
{
    if (!with_cohort) return;
    std::cout << "Cohort samples: " << make_cohort_filename("samples", _query_file, _output_dir)
              << "\nCohort profile: " << make_cohort_filename("profile", _query_file, _output_dir)
              << "\nCohort distances: " << make_cohort_filename("kr", _query_file, _output_dir) << std::endl;
    if (request.unifrac)
        for (const uint32_t metric : request.unifrac->metrics)
            std::cout << "Cohort UniFrac distances (" << distance_name(metric) << "): " << unifrac_file_of(metric) << std::endl;
    for (size_t a = 0; a < NUM_COHORT_ANALYSES; ++a) {
        for (size_t which = 0; asked[a] && which < 2 && kAnalyses[a].files[which].stem; ++which)
            std::cout << kAnalyses[a].files[which].label << ": " << file_of((cohort_analysis)a, which) << std::endl;
        std::cout << _warnings[a];
        if (a == COHORT_EDGEMODEL) std::cout << _permdisp_clipped_warning;  // (its place of old, not beside PERMDISP's line)
        std::cout << std::flush;
    }
}

}  // namespace epik_amd
