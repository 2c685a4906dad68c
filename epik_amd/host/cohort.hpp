// cohort.hpp -- a cohort of samples on the host: the rule of include/epik_amd.h (epik_amd_cohort) over rows in host
// memory, the sum of cohorts, and the Kantorovich-Rubinstein distance between every two samples by the rule's
// sequential loop.  libepik_amd's cohort_add_kernel and cohort_kr_kernel are the same rule on the device; both give the
// same bits (this file is compiled with -ffp-contract=off, and epik_amd_cohort_kr_host is kr_matrix below).
// No reference counterpart: the reference leaves sums and distances over jplace files to a second tool.
// Needs nothing but the C header: libepik_amd compiles cohort.cpp too.
#ifndef EPIK_AMD_HOST_COHORT_HPP
#define EPIK_AMD_HOST_COHORT_HPP

#include <cstdint>
#include <string>
#include <vector>

#include "epik_amd.h"

namespace epik_amd {

struct sample_cohort {
    uint32_t num_samples = 0, num_branches = 0;
    std::vector<uint64_t> mass;  // [num_samples][num_branches]
    std::vector<uint64_t> best;  // [num_samples][num_branches]
    std::vector<epik_amd_profile_totals> totals;  // [num_samples]
    uint64_t bad_samples = 0;    // reads whose sample is >= num_samples: they add to no row

    sample_cohort() = default;
    sample_cohort(uint32_t samples, uint32_t branches)
        : num_samples(samples), num_branches(branches), mass((size_t)samples * branches, 0), best((size_t)samples * branches, 0),
          totals(samples, epik_amd_profile_totals{})
    {
    }

    /// n reads in the form of the C ABI, read i of sample samples[i]: rows[n][keep], n_rows[n], kmer_counts[n][keep],
    /// weights[n] (nullptr: 1)
    void add_rows(const epik_amd_placement* rows, const uint32_t* n_rows, const uint32_t* kmer_counts, const uint32_t* weights,
                  const uint32_t* samples, uint64_t n, uint32_t keep);
    /// what a device cohort holds (epik_amd_cohort_read), or another host cohort: integer sums
    void add_cells(const uint64_t* other_mass, const uint64_t* other_best, const epik_amd_profile_totals* other_totals);
    void merge(const sample_cohort& other);
};

/// KR(s, t) of the rule for all pairs into out[num_samples][num_samples].  0, or EPIK_AMD_ERR_INVALID with `err`
/// naming the branch whose first[] or length is not valid.
int kr_matrix(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
              const double* branch_length, double* out, std::string& err);

/// The UniFrac distance `metric` (EPIK_AMD_DISTANCE_UNWEIGHTED, _WEIGHTED or _GENERALIZED) of the rule for all pairs into
/// out[num_samples][num_samples].  The code behind epik_amd_cohort_unifrac_host; cohort_unifrac_kernel (unifrac_place.hip)
/// gives the same bits.  0, or EPIK_AMD_ERR_INVALID with `err` as kr_matrix, or naming a metric outside 1 .. 3.
int unifrac_matrix(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                   const double* branch_length, uint32_t metric, double* out, std::string& err);

/// kr_matrix for EPIK_AMD_DISTANCE_KR, unifrac_matrix for the three UniFrac distances; any other metric is refused by name
int distance_matrix(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                    const double* branch_length, uint32_t metric, double* out, std::string& err);

/// Squash clustering by the rule (include/epik_amd.h): merges[num_samples - 1], every record written, the unused ones as
/// the rule says, and *num_merges.  The code behind epik_amd_cohort_squash_host; libepik_amd's squash kernels
/// (squash_place.hip) give the same bits.  0, or EPIK_AMD_ERR_INVALID with `err` as kr_matrix.
int squash_merges(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                  const double* branch_length, epik_amd_squash_merge* merges, uint32_t* num_merges, std::string& err);

/// Edge principal components by the rule (include/epik_amd.h): mu[K], proj[S][K], edge[K][N] and *info, every cell
/// written.  The code behind epik_amd_cohort_epca_host; libepik_amd's kernels (epca_place.hip) give the same bits.  0, or
/// EPIK_AMD_ERR_INVALID with `err` naming K outside [1, 64] or the branch whose first[] is above it.
int epca_components(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                    uint32_t num_components, double* mu, double* proj, double* edge, epik_amd_epca_info* info, std::string& err);

/// Phylogenetic k-means by the rule (include/epik_amd.h): samples[S], clusters[K], centroids[K][N] and *info, every cell
/// written.  The code behind epik_amd_cohort_kmeans_host; libepik_amd's kernels (kmeans_place.hip) give the same bits.
/// 0, or EPIK_AMD_ERR_INVALID with `err` naming num_clusters outside [1, 64], max_iterations outside [1, 1000], the branch
/// whose first[] is above it or whose length is negative or not finite.
int kmeans_clusters(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                    const double* branch_length, uint32_t num_clusters, uint32_t max_iterations, epik_amd_kmeans_sample* samples,
                    epik_amd_kmeans_cluster* clusters, double* centroids, epik_amd_kmeans_info* info, std::string& err);

/// Alpha diversity by the rule (include/epik_amd.h): alpha[S], every record written.  The code behind
/// epik_amd_cohort_alpha_host; libepik_amd's kernels (diversity_place.hip) give the same bits.  0, or EPIK_AMD_ERR_INVALID
/// with `err` naming the branch whose first[] is above it or whose length is negative or not finite.
int alpha_indices(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                  const double* branch_length, epik_amd_alpha* alpha, std::string& err);

/// depth_step >= 1, num_depths in [1, 256] and num_depths * depth_step <= 2^20: 0, or EPIK_AMD_ERR_INVALID with `err`
int rarefy_depths_valid(uint32_t depth_step, uint32_t num_depths, std::string& err);

/// Rarefaction curves by the rule (include/epik_amd.h) from best[S][N]: curve[S][J][2], every cell written.  The code
/// behind epik_amd_cohort_rarefy_host; the kernels of diversity_place.hip give the same bits.  Errors as alpha_indices,
/// and the depths as rarefy_depths_valid.
int rarefy_curves(const uint64_t* best, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                  const double* branch_length, uint32_t depth_step, uint32_t num_depths, double* curve, std::string& err);

/// num_columns in [1, 64] and no infinity in meta[S][M]: 0, or EPIK_AMD_ERR_INVALID with `err` naming the cause
int correlation_columns_valid(const double* meta, uint32_t num_samples, uint32_t num_columns, std::string& err);

/// Edge correlation by the rule (include/epik_amd.h): out[M][N] and used[M], every cell written.  The code behind
/// epik_amd_cohort_correlation_host; libepik_amd's kernels (correlation_place.hip) give the same bits.  0, or
/// EPIK_AMD_ERR_INVALID with `err` naming the branch whose first[] is above it, or as correlation_columns_valid.
int correlation_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                        const double* meta, uint32_t num_columns, epik_amd_correlation* out, uint32_t* used, std::string& err);

/// Edge dispersion by the rule: out[N], every cell written.  The code behind epik_amd_cohort_dispersion_host.
int dispersion_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                       epik_amd_dispersion* out, std::string& err);

/// The four permutation tests below take `strata` (strata[S] by sample, any uint32 an id; null: one stratum): the strata rule
/// of include/epik_amd.h, sigma_p in place of rank_p.  Null gives the bits of the rule without strata.

/// num_columns in [1, 64], num_permutations in [1, 999 999], every label below 256 or 0xffffffff (missing) and, with
/// pairwise, at most 32 distinct labels a column: 0, or EPIK_AMD_ERR_INVALID with `err` naming the cause
int permanova_arguments_valid(const uint32_t* labels, uint32_t num_samples, uint32_t num_columns, uint32_t num_permutations,
                              bool pairwise, std::string& err);

/// PERMANOVA by the rule (include/epik_amd.h) from a KR matrix kr[S][S] and totals[S] (T_s): out[M][1 + Q], and where not
/// null ssw[M][1 + Q][P + 1] and group_ss[M][256], every cell written.  libepik_amd's kernels (permanova_place.hip) give the
/// same bits.  0, or as permanova_arguments_valid.
int permanova_records_of_kr(const double* kr, const uint64_t* totals, uint32_t num_samples, const uint32_t* labels,
                            uint32_t num_columns, uint32_t num_permutations, uint64_t seed, bool pairwise, epik_amd_permanova* out,
                            double* ssw, double* group_ss, std::string& err, const uint32_t* strata = nullptr);
/// The same from the cells: distance_matrix, then permanova_records_of_kr.  The code behind epik_amd_cohort_permanova_host
/// and _permanova_metric_host.
int permanova_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                      const double* branch_length, const uint32_t* labels, uint32_t num_columns, uint32_t num_permutations,
                      uint64_t seed, bool pairwise, epik_amd_permanova* out, double* ssw, double* group_ss, std::string& err,
                      uint32_t metric = EPIK_AMD_DISTANCE_KR, const uint32_t* strata = nullptr);

/// Principal coordinates by the rule (include/epik_amd.h) from a KR matrix kr[S][S] and totals[S] (T_s): mu[S], coord[S][K]
/// and *info, every cell written.  libepik_amd's kernels (pcoa_place.hip) give the same bits.  0, or EPIK_AMD_ERR_INVALID
/// with `err` naming K outside [1, 64].
int pcoa_components_of_kr(const double* kr, const uint64_t* totals, uint32_t num_samples, uint32_t num_components, double* mu,
                          double* coord, epik_amd_pcoa_info* info, std::string& err);
/// The same from the cells: distance_matrix, then pcoa_components_of_kr.  The code behind epik_amd_cohort_pcoa_host and
/// _pcoa_metric_host.
int pcoa_components(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                    const double* branch_length, uint32_t num_components, double* mu, double* coord, epik_amd_pcoa_info* info,
                    std::string& err, uint32_t metric = EPIK_AMD_DISTANCE_KR);

/// num_columns in [1, 64], num_permutations in [1, 999 999], every label below 32 or 0xffffffff (missing): 0, or
/// EPIK_AMD_ERR_INVALID with `err` naming the cause
int edgetest_arguments_valid(const uint32_t* labels, uint32_t num_samples, uint32_t num_columns, uint32_t num_permutations,
                             std::string& err);
/// The edge test by the rule (include/epik_amd.h), one thread: out[M][N], and where not null stat[M][4][N][P + 1] and
/// max[M][4][P + 1], every cell written.  libepik_amd's kernels (edgetest_place.hip) give the same bits.  The code behind
/// epik_amd_cohort_edgetest_host.  0, or as edgetest_arguments_valid; first[b] > b is refused.
int edgetest_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                     const uint32_t* labels, uint32_t num_columns, uint32_t num_permutations, uint64_t seed, epik_amd_edgetest* out,
                     double* stat, double* max, std::string& err, const uint32_t* strata = nullptr);

/// num_columns in [1, 64], num_permutations in [1, 999 999], every label below 32 or 0xffffffff (missing): 0, or
/// EPIK_AMD_ERR_INVALID with `err` naming the cause
int permdisp_arguments_valid(const uint32_t* labels, uint32_t num_samples, uint32_t num_columns, uint32_t num_permutations,
                             std::string& err);
/// PERMDISP by the rule (include/epik_amd.h) from the matrix kr[S][S] and totals[S], one thread: out[M][1 + Q], group_mean[M][32],
/// z[M][S] and, where not null, stat[M][1 + Q][P + 1], every cell written.  libepik_amd's kernels (permdisp_place.hip) give the
/// same bits.  The code behind epik_amd_cohort_permdisp_kr_host.  0, or as permdisp_arguments_valid.
int permdisp_records_of_kr(const double* kr, const uint64_t* totals, uint32_t num_samples, const uint32_t* labels,
                           uint32_t num_columns, uint32_t num_permutations, uint64_t seed, bool pairwise, epik_amd_permdisp* out,
                           double* stat, double* group_mean, double* z, std::string& err, const uint32_t* strata = nullptr);
/// The same from mass[S][N]: the matrix by distance_matrix first.  The code behind epik_amd_cohort_permdisp_host and
/// _permdisp_metric_host.
int permdisp_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                     const double* branch_length, const uint32_t* labels, uint32_t num_columns, uint32_t num_permutations,
                     uint64_t seed, bool pairwise, epik_amd_permdisp* out, double* stat, double* group_mean, double* z, std::string& err,
                     uint32_t metric = EPIK_AMD_DISTANCE_KR, const uint32_t* strata = nullptr);

/// num_terms in [1, 16], every kind 0 or 1, num_permutations in [1, 999 999], every label of a factor term below 32 or
/// 0xffffffff (missing), no infinite value of a numeric term, and at most 64 columns as the rule counts them: 0, or
/// EPIK_AMD_ERR_INVALID with `err` naming the cause
int model_arguments_valid(const uint32_t* kind, const uint32_t* labels, const double* values, uint32_t num_samples,
                          uint32_t num_terms, uint32_t num_permutations, std::string& err);
/// The sequential model by the rule (include/epik_amd.h) from the matrix kr[S][S] and totals[S], one thread: out[T + 1], *info,
/// aliased[64] and, where not null, stat[T + 1][P + 1], every cell written.  libepik_amd's kernels (model_place.hip) give the
/// same bits.  The code behind epik_amd_cohort_model_kr_host.  0, or as model_arguments_valid.
int model_records_of_kr(const double* kr, const uint64_t* totals, uint32_t num_samples, const uint32_t* kind, const uint32_t* labels,
                        const double* values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed, epik_amd_model_term* out,
                        epik_amd_model_info* info, double* stat, uint8_t* aliased, std::string& err,
                        const uint32_t* strata = nullptr);
/// The same from mass[S][N]: the matrix by distance_matrix first.  The code behind epik_amd_cohort_model_host and
/// _model_metric_host.
int model_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                  const double* branch_length, const uint32_t* kind, const uint32_t* labels, const double* values, uint32_t num_terms,
                  uint32_t num_permutations, uint64_t seed, epik_amd_model_term* out, epik_amd_model_info* info, double* stat,
                  uint8_t* aliased, std::string& err, uint32_t metric = EPIK_AMD_DISTANCE_KR, const uint32_t* strata = nullptr);

/// The edge model by the rule (include/epik_amd.h) from mass[S][N], one thread: out[T][N], *info, aliased[64] and, where not
/// null, stat[T][2][N][P + 1] and max[T][2][P + 1], every cell written.  libepik_amd's kernels (edgemodel_place.hip) give the
/// same bits.  The code behind epik_amd_cohort_edgemodel_host.  0, as model_arguments_valid, or first[b] > b.
int edgemodel_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first, const uint32_t* kind,
                      const uint32_t* labels, const double* values, uint32_t num_terms, uint32_t num_permutations, uint64_t seed,
                      epik_amd_edgemodel* out, epik_amd_edgemodel_info* info, double* stat, double* max, uint8_t* aliased,
                      std::string& err, const uint32_t* strata = nullptr);

/// The sides of a Mantel call as the C ABI takes them: values[Mv][S] (NaN: missing), matrices[Mm][S][S] with
/// matrix_present[Mm][S], the methods' bits and the control (a side, or EPIK_AMD_MANTEL_NO_CONTROL)
struct mantel_sides {
    const double* values;
    uint32_t num_columns;
    const double* matrices;
    const uint8_t* matrix_present;
    uint32_t num_matrices, methods, control;
    uint32_t sides() const { return num_columns + num_matrices; }
    uint32_t tests() const { return sides() * ((methods & 1u) + (methods >> 1 & 1u)); }
};
/// num_samples at most 8 192, Mv in [0, 64], Mm in [0, 8] and a side at least, their arrays present, methods in 1 .. 3, the
/// control a side or none, num_permutations in [1, 999 999], no infinite value, and no cell [s][t], s < t, of a matrix between
/// two present samples that is negative or not finite: 0, or EPIK_AMD_ERR_INVALID with `err` naming the cause.  Reads nothing of
/// the arrays when a count is refused.
int mantel_arguments_valid(const mantel_sides& sides, uint32_t num_samples, uint32_t num_permutations, std::string& err);
/// num_samples at most 8 192, then as permanova_arguments_valid without pairwise
int anosim_arguments_valid(const uint32_t* labels, uint32_t num_samples, uint32_t num_columns, uint32_t num_permutations,
                           std::string& err);
/// The Mantel and partial Mantel tests by the rule (include/epik_amd.h) from the matrix kr[S][S] and totals[S], one thread:
/// out[sides.tests()] and, where not null, stat[tests][P + 1], every cell written.  libepik_amd's kernels (mantel_place.hip) give
/// the same bits.  The code behind epik_amd_cohort_mantel_kr_host.  0, or as mantel_arguments_valid.
int mantel_records_of_kr(const double* kr, const uint64_t* totals, uint32_t num_samples, const mantel_sides& sides,
                         uint32_t num_permutations, uint64_t seed, epik_amd_mantel* out, double* stat, std::string& err,
                         const uint32_t* strata = nullptr);
/// The same from mass[S][N]: the matrix by distance_matrix first.  The code behind epik_amd_cohort_mantel_host.
int mantel_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                   const double* branch_length, const mantel_sides& sides, uint32_t num_permutations, uint64_t seed,
                   epik_amd_mantel* out, double* stat, std::string& err, uint32_t metric = EPIK_AMD_DISTANCE_KR,
                   const uint32_t* strata = nullptr);
/// ANOSIM by the rule from the matrix kr[S][S] and totals[S], one thread: out[M] and, where not null, stat[M][P + 1], every cell
/// written.  The code behind epik_amd_cohort_anosim_kr_host; the kernels of mantel_place.hip give the same bits.
int anosim_records_of_kr(const double* kr, const uint64_t* totals, uint32_t num_samples, const uint32_t* labels,
                         uint32_t num_columns, uint32_t num_permutations, uint64_t seed, epik_amd_anosim* out, double* stat,
                         std::string& err, const uint32_t* strata = nullptr);
/// The same from mass[S][N].  The code behind epik_amd_cohort_anosim_host.
int anosim_records(const uint64_t* mass, uint32_t num_samples, uint32_t num_branches, const uint32_t* first,
                   const double* branch_length, const uint32_t* labels, uint32_t num_columns, uint32_t num_permutations,
                   uint64_t seed, epik_amd_anosim* out, double* stat, std::string& err, uint32_t metric = EPIK_AMD_DISTANCE_KR,
                   const uint32_t* strata = nullptr);

/// The list of samples of --cohort: one name<TAB>path line each, paths relative to the list's directory; blank lines and
/// lines that begin with '#' are skipped.  Throws std::runtime_error naming the line for a line without a tab, an empty
/// name or path, a name given before, or a file that cannot be read; and for a list without any sample.
struct cohort_sample {
    std::string name, path;
};
std::vector<cohort_sample> read_cohort_list(const std::string& list_file);

/// The metadata of --cohort-correlation: a TSV whose header is sample<TAB>name1<TAB>... (1 to 64 unique, non-empty
/// names), then one line per sample; blank lines and lines that begin with '#' are skipped.  A value is empty or NA (both
/// missing: NaN in `values`) or a decimal number, [+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?, read by strtod.  Throws
/// std::runtime_error naming the line, and the column where there is one, for anything else, a value that overflows to
/// infinity, a wrong field count or a sample given twice; and naming the sample of the list that the file lacks.  A line
/// whose name is not in the list is skipped and counted.
struct cohort_metadata {
    std::vector<std::string> columns;
    std::vector<double> values;  // [S][M], in the order of the list
    size_t skipped = 0;
};
cohort_metadata read_cohort_metadata(const std::string& file, const std::vector<cohort_sample>& samples);

/// The factors of --cohort-permanova: a TSV as read_cohort_metadata's, but a value is a label: any non-empty text without a
/// tab; empty or NA is missing (0xffffffff in `labels`).  The labels of a column are numbered by first appearance in the
/// file among the list's samples: names[c][id].  Throws std::runtime_error naming the line, and the column where there is
/// one, for a wrong field count, a sample given twice, a column with more than 256 distinct labels (32 with `pairwise`);
/// and naming the sample of the list that the file lacks.  A line whose name is not in the list is skipped and counted.
struct cohort_factors {
    std::vector<std::string> columns;
    std::vector<std::vector<std::string>> names;  // [M]: the labels of a column by id
    std::vector<uint32_t> labels;                 // [S][M], in the order of the list
    size_t skipped = 0;
};
/// `most_labels`, where not 0, is the cap instead (32 for --cohort-edge-test); `flag` begins every message.
cohort_factors read_cohort_factors(const std::string& file, const std::vector<cohort_sample>& samples, bool pairwise,
                                   size_t most_labels = 0, const char* flag = "--cohort-permanova");

/// The design of --cohort-model: FILE is a TSV in the layout of the factor file, `terms` the LIST of --cohort-model-terms, a
/// comma-separated f:NAME (a factor) or n:NAME (numeric) per term in test order, NAME a column of FILE.  Cells are text by the
/// factor reader's rules (empty or NA is missing); a numeric term's cells are numbers by the metadata reader's rule.  The labels
/// of a factor term are numbered by first appearance in the file among the list's samples: names[t][id].  Throws
/// std::runtime_error for an empty list, more than 16 terms, a prefix other than f: or n:, a term given twice, a column the
/// header lacks, and, naming the line and the column, for a cell of a numeric term that is no number or overflows, a factor
/// term with more than 32 labels, a wrong field count or a sample given twice; and naming the sample of the list that the
/// file lacks.  A line whose name is not in the list is skipped and counted.
struct cohort_design {
    std::vector<std::string> terms;               // [T]: the column names
    std::vector<uint32_t> kind;                   // [T]: 0 a factor, 1 numeric
    std::vector<std::vector<std::string>> names;  // [T]: the labels of a factor term by id
    std::vector<uint32_t> labels;                 // [S][T], in the order of the list
    std::vector<double> values;                   // [S][T]
    size_t skipped = 0;
};
cohort_design read_cohort_design(const std::string& file, const std::string& terms, const std::vector<cohort_sample>& samples);

/// <output_dir>/cohort_<what>_<basename(list)><extension>, what = samples | profile | kr | squash | epca | epca_edges | pcoa | kmeans |
/// kmeans_centroids | alpha | rarefy | correlation | dispersion | permanova | edgetest | permdisp | model | unifrac_<metric>
std::string make_cohort_filename(const std::string& what, const std::string& list_file, const std::string& output_dir,
                                 const std::string& extension = ".tsv");

/// cohort_samples: a header line, then per sample in list order name, records, placed, no_hit, too_short, too_narrow,
/// total_mass_q.  cohort_profile: long format, name, edge_num, best, mass_q for every (sample, branch) cell with a
/// non-zero best or mass_q, samples in list order, branches by edge_num (the post-order id, the jplace's number).
/// cohort_kr: a first line of names, then per sample its name and the distances to every sample as %.17g.
std::string format_cohort_samples_tsv(const std::vector<cohort_sample>& samples, const sample_cohort& cohort);
std::string format_cohort_profile_tsv(const std::vector<cohort_sample>& samples, const sample_cohort& cohort);
std::string format_cohort_kr_tsv(const std::vector<cohort_sample>& samples, const std::vector<double>& kr);
/// kr | unweighted | weighted | generalized of EPIK_AMD_DISTANCE_*; throws for any other metric.  distance_of_name: the
/// metric of such a name (KR only `with_kr`), or 0xffffffff.  distance_field: what the first line of a cohort_pcoa,
/// cohort_permanova or cohort_permdisp file ends in: nothing over KR, else <TAB>distance=NAME.
const char* distance_name(uint32_t metric);
uint32_t distance_of_name(const std::string& name, bool with_kr);
std::string distance_field(uint32_t metric);
/// The LIST of --cohort-unifrac: a comma-separated subset of unweighted, weighted, generalized, or all; the metrics in the
/// order given.  Throws std::runtime_error naming an unknown or repeated name.
std::vector<uint32_t> parse_unifrac_list(const std::string& list);
/// cohort_unifrac_<metric> .tsv: the square layout of cohort_kr, doubles %.17g
inline std::string format_cohort_unifrac_tsv(const std::vector<cohort_sample>& samples, const std::vector<double>& matrix)
{
    return format_cohort_kr_tsv(samples, matrix);
}
/// cohort_squash .tsv: "# epik_amd squash v1  samples=S clustered=S' merges=M", a "# unclustered<TAB>name" line per
/// empty sample (live[s] == 0), the header step node a b size dist len_a len_b, a line per merge: a leaf is its index in
/// list order, an internal node S + step, size the samples under the node, doubles as %.17g.  .nwk: the cluster tree,
/// child a before child b, lengths %.17g, none at the root, leaves labelled with the names ('...' with inner quotes
/// doubled for a name with a character outside [A-Za-z0-9_.-]); "name;" for one clustered sample, ";" for none.
std::string format_squash_tsv(const std::vector<cohort_sample>& samples, const std::vector<char>& live,
                              const epik_amd_squash_merge* merges, uint32_t num_merges);
std::string format_squash_newick(const std::vector<cohort_sample>& samples, const std::vector<char>& live,
                                 const epik_amd_squash_merge* merges, uint32_t num_merges);
/// cohort_epca .tsv: "# epik_amd epca v1  samples=S used=L components=K' sweeps=n converged=0|1", a "# unused<TAB>name"
/// line per sample without mass (used[s] == 0), a "# component<TAB>k<TAB>mu<TAB>lambda<TAB>fraction<TAB>null|ok" line per
/// component (k from 1, lambda = mu / max(L - 1, 1), fraction = mu / trace or 0), the column names name pc1 .. pcK', then
/// per used sample in list order its name and proj[s][0 .. K'), the rows of proj K = num_components wide; doubles %.17g.
/// cohort_epca_edges .tsv: edge_num pc1 .. pcK', a line per inner branch (first[b] < b) in id order from edge[K][N].
std::string format_epca_tsv(const std::vector<cohort_sample>& samples, const std::vector<char>& used, uint32_t num_components,
                            const double* mu, const double* proj, const epik_amd_epca_info& info);
std::string format_epca_edges_tsv(const std::vector<uint32_t>& first, const double* edge, const epik_amd_epca_info& info);
/// cohort_pcoa .tsv: "# epik_amd pcoa v1  samples=S used=L components=K' sweeps=n converged=0|1 negative=x" (x = -neg / pos,
/// 0 when pos is 0), a "# unused<TAB>name" line per sample without mass (totals[s] == 0), a "# eigenvalue<TAB>k<TAB>mu<TAB>
/// fraction<TAB>real|null|negative" line for each of the L eigenvalues (k from 1, fraction = mu / pos or 0), the column names
/// name pc1 .. pcK', then per used sample in list order its name and coord[s][0 .. K'), the rows of coord K = num_components
/// wide; doubles %.17g.  Over a `distance` other than KR the first line ends in distance_field(distance).
std::string format_pcoa_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals, uint32_t num_components,
                            const double* mu, const double* coord, const epik_amd_pcoa_info& info,
                            uint32_t distance = EPIK_AMD_DISTANCE_KR);
/// cohort_kmeans .tsv: "# epik_amd kmeans v1  samples=S used=L clusters=K' iterations=i converged=0|1", a "# unused<TAB>name"
/// line per sample without mass, a "# cluster<TAB>k<TAB>size<TAB>seed name<TAB>sum_dist<TAB>sum_sq" line per cluster
/// k < K', the column names name cluster dist, then per used sample in list order its name, cluster and dist; doubles %.17g.
/// cohort_kmeans_centroids .tsv: cluster edge_num mass, a line per non-zero cell of centroids[K][N], k < K'.
std::string format_kmeans_tsv(const std::vector<cohort_sample>& samples, const epik_amd_kmeans_sample* records,
                              const epik_amd_kmeans_cluster* clusters, const epik_amd_kmeans_info& info);
std::string format_kmeans_centroids_tsv(const double* centroids, uint32_t num_branches, const epik_amd_kmeans_info& info);
/// cohort_alpha .tsv: "# epik_amd alpha v1  samples=S used=L", a "# unused<TAB>name" line per sample without mass
/// (pd == -1.0), the column names name pd rooted_pd bwpd_0.5 bwpd_1 quadratic_entropy, then a line per used sample in
/// list order; doubles %.17g.
std::string format_alpha_tsv(const std::vector<cohort_sample>& samples, const epik_amd_alpha* alpha);
/// cohort_rarefy .tsv: "# epik_amd rarefy v1  samples=S used=L step=STEP depths=J", a "# unused<TAB>name" line per sample
/// that is not rarefiable (reads[s] = n_s is 0 or >= 2^53), the column names name k reads pd rooted_pd, then, long format,
/// a line for every used sample and every k_j <= n_s from curve[S][J][2]; doubles %.17g.
std::string format_rarefy_tsv(const std::vector<cohort_sample>& samples, const uint64_t* reads, uint32_t depth_step,
                              uint32_t num_depths, const double* curve);
/// cohort_correlation .tsv: "# epik_amd correlation v1  samples=S used=L columns=M", a "# unused<TAB>name" line per sample
/// without mass (totals[s] = T_s is 0), a "# column<TAB>c<TAB>name<TAB>used_c" line per column, the column names edge_num
/// column mass_pearson mass_spearman imbalance_pearson imbalance_spearman, then, long format, a line for every branch and
/// every column from records[M][N]; doubles %.17g, NA as NA.
std::string format_correlation_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals,
                                   const std::vector<std::string>& columns, uint32_t num_branches,
                                   const epik_amd_correlation* records, const uint32_t* used_of);
/// cohort_dispersion .tsv: "# epik_amd dispersion v1  samples=S used=L", the "# unused" lines, the column names edge_num
/// and the eight fields, then a line per branch.
std::string format_dispersion_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals, uint32_t num_branches,
                                  const epik_amd_dispersion* records);
/// cohort_permanova .tsv: "# epik_amd permanova v1  samples=S used=L columns=M permutations=P seed=X pairwise=0|1", the
/// "# unused" lines, a "# column<TAB>c<TAB>name<TAB>used_c<TAB>groups_c" line per column, a "# group<TAB>c<TAB>g<TAB>label<TAB>n<TAB>
/// ss_within_g" line per group (the groups in the rule's order, from labels[S][M], totals[S] and names[c][id]; ss_within_g from
/// group_ss[M][256]), the column names column a b used groups ss_total ss_among ss_within f r2 at_most p, then per column
/// the whole test (a = b = *) and, with pairwise, its pairs in slot order from records[M][1 + Q]; ss_among is
/// ss_total - ss_within; doubles %.17g, NA as NA.  Over a `distance` other than KR the first line ends in distance_field(distance).
std::string format_permanova_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals,
                                 const std::vector<std::string>& columns, const std::vector<std::vector<std::string>>& names,
                                 const uint32_t* labels, uint32_t num_permutations, uint64_t seed, bool pairwise,
                                 const epik_amd_permanova* records, const double* group_ss,
                                 uint32_t distance = EPIK_AMD_DISTANCE_KR);
/// cohort_edgetest .tsv: "# epik_amd edgetest v1  samples=S used=L columns=M permutations=P seed=X", the "# unused" lines, a
/// "# column<TAB>c<TAB>name<TAB>used_c<TAB>groups_c" line per column, a "# group<TAB>c<TAB>g<TAB>label<TAB>n" line per group (the
/// groups in the rule's order), the column names edge_num column and, for mass and imbalance, _eta2 _f _p _p_adj _top _h _kw_p
/// _kw_p_adj, then per column a line per branch with at least one defined family, from records[M][N]; top is the group's
/// label; doubles %.17g, NA as NA.
std::string format_edgetest_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals,
                                const std::vector<std::string>& columns, const std::vector<std::vector<std::string>>& names,
                                const uint32_t* labels, uint32_t num_branches, uint32_t num_permutations, uint64_t seed,
                                const epik_amd_edgetest* records);
/// cohort_permdisp .tsv: "# epik_amd permdisp v1  samples=S used=L columns=M permutations=P seed=X pairwise=0|1", the "# unused"
/// lines, the "# column" lines as cohort_permanova's, a "# group<TAB>c<TAB>g<TAB>label<TAB>n<TAB>mean_distance" line per group (from
/// group_mean[M][32]), the column names column a b used groups clipped eta2 f at_least p, per column the whole test (a = b = *)
/// and, with pairwise, its pairs in slot order from records[M][1 + Q]; then "# distances", the column names column name label
/// distance and, per column, a line per sample of U_c in list order from z[M][S]; doubles %.17g, NA as NA.  Over a `distance`
/// other than KR the first line ends in distance_field(distance).
std::string format_permdisp_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals,
                                const std::vector<std::string>& columns, const std::vector<std::vector<std::string>>& names,
                                const uint32_t* labels, uint32_t num_permutations, uint64_t seed, bool pairwise,
                                const epik_amd_permdisp* records, const double* group_mean, const double* z,
                                uint32_t distance = EPIK_AMD_DISTANCE_KR);
/// cohort_model .tsv: "# epik_amd model v1  samples=S used=L terms=T columns=C rank=R permutations=P seed=X" (L the complete
/// cases with mass), a "# unused<TAB>name" line per sample without mass, a "# incomplete<TAB>name<TAB>term" line per sample with
/// mass that lacks a value (the first term it lacks), a "# term<TAB>k<TAB>f|n<TAB>name<TAB>columns<TAB>df" line per term, a
/// "# group<TAB>k<TAB>g<TAB>label<TAB>n" line per group of a factor term (the groups in the rule's order), a "# aliased<TAB>k<TAB>label
/// or -" line per dropped column, the column names term df ss r2 f at_least p, a line per term in order, then model, residual
/// (df_res, ss_res, and 1 less the r2 of every term with a column, one subtraction chain in term order) and total (L - 1,
/// ss_total, 1); doubles %.17g, NA where undefined.  Over a `distance` other than KR the first line ends in distance_field(distance).
std::string format_model_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals, const cohort_design& design,
                             uint32_t num_permutations, uint64_t seed, const epik_amd_model_term* records,
                             const epik_amd_model_info& info, const uint8_t* aliased, uint32_t distance = EPIK_AMD_DISTANCE_KR);
/// cohort_edgemodel .tsv: "# epik_amd edgemodel v1  samples=S used=L terms=T columns=C rank=R permutations=P seed=X", the
/// "# unused", "# incomplete", "# term", "# group" and "# aliased" lines of cohort_model .tsv, the column names term edge_num and,
/// for mass and imbalance, _ss _r2 _partial_r2 _f _sign _p _p_adj, then per term a line per branch with a defined family, from
/// records[T][N]; doubles %.17g, NA where undefined.
std::string format_edgemodel_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals, const cohort_design& design,
                                 uint32_t num_branches, uint32_t num_permutations, uint64_t seed, const epik_amd_edgemodel* records,
                                 const epik_amd_edgemodel_info& info, const uint8_t* aliased);
/// A matrix of --cohort-mantel-matrix NAME=FILE: FILE is a square TSV in the layout of cohort_kr_<list>.tsv, a first line
/// name<TAB>name1<TAB>..., then per line a name and one distance per name of the first line; blank lines and lines that begin with
/// '#' are skipped.  The names are matched to the list: matrix[S][S] in the order of the list, present[s] = 1 for a sample of the
/// list that the file has (a sample it lacks is missing on that side), names outside the list skipped and counted.  Throws
/// std::runtime_error naming the line, and the column where there is one, for a name given twice (in the first line or as a row), a
/// row whose name the first line lacks, a wrong field count, a cell that is no number, negative or not finite, a cell that differs
/// from its mirror cell, and for a name of the first line without a row.  `flag` begins every message.
struct cohort_matrix {
    std::vector<double> matrix;    // [S][S]
    std::vector<uint8_t> present;  // [S]
    size_t skipped = 0;
};
cohort_matrix read_cohort_matrix(const std::string& file, const std::vector<cohort_sample>& samples,
                                 const char* flag = "--cohort-mantel-matrix");
/// The sides of --cohort-mantel FILE and --cohort-mantel-matrix NAME=FILE ... with --cohort-mantel-partial NAME: the metadata
/// file (empty: none) read by read_cohort_metadata, every column a side, then the matrices in the order given (at most 8, each
/// NAME=FILE with a NAME that no other side has), read by read_cohort_matrix.  names[Q]; values[Mv][S] (by side, as the C ABI
/// takes them), matrices[Mm][S][S], present[Mm][S]; control: the side that `partial` names, or EPIK_AMD_MANTEL_NO_CONTROL for an
/// empty one.  Throws std::runtime_error as the two readers do, and naming an argument without '=', an empty or repeated NAME,
/// a ninth matrix, no side at all, or a `partial` that names no side.
struct cohort_mantel_sides {
    std::vector<std::string> names;
    std::vector<double> values, matrices;
    std::vector<uint8_t> present;
    uint32_t num_columns = 0, num_matrices = 0, control = EPIK_AMD_MANTEL_NO_CONTROL;
    size_t skipped = 0;
    mantel_sides sides(uint32_t methods) const
    {
        return mantel_sides{values.data(), num_columns, matrices.data(), present.data(), num_matrices, methods, control};
    }
};
cohort_mantel_sides read_cohort_mantel_sides(const std::string& metadata_file, const std::vector<std::string>& matrix_arguments,
                                             const std::string& partial, const std::vector<cohort_sample>& samples);
/// pearson | spearman | both of the methods' bits, and the bits of such a name (0 for any other)
const char* mantel_method_name(uint32_t methods);
uint32_t mantel_methods_of_name(const std::string& name);
/// cohort_mantel .tsv: "# epik_amd mantel v1  samples=S used=L sides=Q permutations=P seed=X method=pearson|spearman|both
/// partial=NAME|-", the "# unused" lines, a "# side<TAB>q<TAB>column|matrix<TAB>name<TAB>used_q" line per side (the first
/// num_columns of side_names are columns; used_q of the side's first test), the column names side method used r r_xz r_yz stat
/// at_least p, then a line per test of records[Q * popcount(methods)]; doubles %.17g, NA as NA.  Over a `distance` other than KR
/// the first line ends in distance_field(distance).
std::string format_mantel_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals,
                              const std::vector<std::string>& side_names, uint32_t num_columns, uint32_t methods, uint32_t control,
                              uint32_t num_permutations, uint64_t seed, const epik_amd_mantel* records,
                              uint32_t distance = EPIK_AMD_DISTANCE_KR);
/// cohort_anosim .tsv: "# epik_amd anosim v1  samples=S used=L columns=M permutations=P seed=X", the "# unused" lines, the
/// "# column" lines as cohort_permanova's, a "# group<TAB>c<TAB>g<TAB>label<TAB>n" line per group (the groups in the rule's order),
/// the column names column used groups mean_between mean_within r at_least p, then a line per column of records[M]; doubles
/// %.17g, NA as NA.  Over a `distance` other than KR the first line ends in distance_field(distance).
std::string format_anosim_tsv(const std::vector<cohort_sample>& samples, const uint64_t* totals,
                              const std::vector<std::string>& columns, const std::vector<std::vector<std::string>>& names,
                              const uint32_t* labels, uint32_t num_permutations, uint64_t seed, const epik_amd_anosim* records,
                              uint32_t distance = EPIK_AMD_DISTANCE_KR);
/// The strata of --cohort-strata FILE [--cohort-strata-column NAME]: FILE is a TSV read by the factor reader (the same errors,
/// naming line and column, under the flag's name) without a cap on the distinct labels; `column` picks the column and may be
/// empty only if FILE has one.  strata[S]: the label ids of that column by first appearance; *name: the column's name.  Throws
/// std::runtime_error too for a column that FILE lacks, and for a sample of the list without a value, naming its line.
std::vector<uint32_t> read_cohort_strata(const std::string& file, const std::string& column, const std::vector<cohort_sample>& samples,
                                         std::string* name);
/// `text`, a cohort_permanova, _permdisp, _edgetest or _model file, with <TAB>strata=NAME at the end of its first line (after
/// distance=.. where that is there): what --cohort-strata makes of the four files.  An empty name leaves the text as it is.
std::string with_strata_field(std::string text, const std::string& name);
/// whether the labels of column c of labels[S][M] (`missing`: none) are constant inside every stratum among the samples with
/// mass and a label: nothing can be permuted there
bool constant_within_strata(const uint32_t* labels, size_t S, size_t M, size_t c, uint32_t missing, const uint64_t* totals,
                            const uint32_t* strata);
/// `text` into `filename` through `filename`.part, renamed when all of it is written
void write_through_part(const std::string& filename, const std::string& text);

}  // namespace epik_amd
#endif
