// cohort_test.cpp -- the host cohort (cohort.cpp) driven from files, for tests/test_cohort_cpu.py; needs no GPU and no
// libepik_amd.
//   cohort_test add <out.bin> <in.bin>...   the cohort of every input, merged: uint64 mass[S][N], best[S][N],
//                                           totals[S][5], bad_samples
//   cohort_test kr <out.bin> <in.bin>       the KR matrix, float64 [S][S]
//   cohort_test unifrac <out.bin> <in.bin> <metric>
//                                           the UniFrac matrix of a `kr` input, metric 1 (unweighted), 2 (weighted) or 3
//                                           (generalized): float64 [S][S]
//   cohort_test squash <out.bin> <in.bin>   the squash clustering of a `kr` input: epik_amd_squash_merge [S - 1], then
//                                           uint32 num_merges
//   cohort_test epca <out.bin> <in.bin> <K> the edge principal components of a `kr` input (its lengths are not used):
//                                           float64 mu[K], proj[S][K], edge[K][N], then epik_amd_epca_info
//   cohort_test pcoa <out.bin> <in.bin> <K> the principal coordinates of a `kr` input: float64 mu[S], coord[S][K], then
//                                           epik_amd_pcoa_info
//   cohort_test pcoa-tsv <out.tsv> <in.bin> <names.txt> <K>
//                                           the file of --cohort-pcoa for a `kr` input whose samples are named by the lines
//                                           of names.txt, through the formatter
//   cohort_test kmeans <out.bin> <in.bin> <K> <max_iterations>
//                                           the phylogenetic k-means of a `kr` input: epik_amd_kmeans_sample [S],
//                                           epik_amd_kmeans_cluster [K], float64 centroids[K][N], then epik_amd_kmeans_info
//   cohort_test alpha <out.bin> <in.bin>    the alpha diversity of a `kr` input: epik_amd_alpha [S]
//   cohort_test rarefy <out.bin> <in.bin> <depth_step> <num_depths>
//                                           the rarefaction curves of a `kr` input whose cells are `best`: float64 [S][J][2]
//   cohort_test correlation <out.bin> <in.bin> <meta.bin>
//                                           the edge correlation of a `kr` input (its lengths are not used) with a raw
//                                           `meta` file, float64 [S][M]: epik_amd_correlation [M][N], then uint32 used[M]
//   cohort_test dispersion <out.bin> <in.bin>
//                                           the edge dispersion of a `kr` input: epik_amd_dispersion [N]
//   cohort_test permanova <out.bin> <in.bin> <labels.bin> <P> <seed> <pairwise>
//                                           PERMANOVA of a `kr` input with a raw `labels` file, uint32 [S][M]:
//                                           epik_amd_permanova [M][1 + Q], float64 ssw[M][1 + Q][P + 1], float64 group_ss[M][256]
//   cohort_test permdisp <out.bin> <in.bin> <labels.bin> <P> <seed> <pairwise>
//                                           PERMDISP of a `kr` input, arguments as permanova's (a label below 32):
//                                           epik_amd_permdisp [M][1 + Q], float64 stat[M][1 + Q][P + 1], group_mean[M][32], z[M][S]
//   cohort_test permdisp-tsv <out.tsv> <in.bin> <names.txt> <factors.tsv> <P> <seed> <pairwise>
//                                           the file of --cohort-permdisp, as permanova-tsv
//   cohort_test permanova-tsv <out.tsv> <in.bin> <names.txt> <factors.tsv> <P> <seed> <pairwise>
//                                           the file of --cohort-permanova for a `kr` input whose samples are named by the
//                                           lines of names.txt, through the factor file's reader and the formatter
//   cohort_test edgetest <out.bin> <in.bin> <labels.bin> <P> <seed>
//                                           the edge test of a `kr` input with a raw `labels` file, uint32 [S][M]:
//                                           epik_amd_edgetest [M][N], float64 stat[M][4][N][P + 1], float64 max[M][4][P + 1]
//   cohort_test edgetest-tsv <out.tsv> <in.bin> <names.txt> <factors.tsv> <P> <seed>
//                                           the file of --cohort-edge-test for a `kr` input whose samples are named by the
//                                           lines of names.txt, through the factor file's reader and the formatter
//   cohort_test model <out.bin> <in.bin> <design.bin> <P> <seed>
//                                           the sequential model of a `kr` input with a `design` file, uint64 T, uint32 kind[T],
//                                           uint32 labels[S][T], float64 values[S][T]: epik_amd_model_term [T + 1],
//                                           epik_amd_model_info, float64 stat[T + 1][P + 1], uint8 aliased[64]
//   cohort_test model-tsv <out.tsv> <in.bin> <names.txt> <design.tsv> <terms> <P> <seed>
//                                           the file of --cohort-model for a `kr` input whose samples are named by the lines of
//                                           names.txt, through the design file's reader and the formatter
//   cohort_test edgemodel <out.bin> <in.bin> <design.bin> <P> <seed>
//                                           the edge model of a `kr` input (its lengths are not read) with a `design` file as for
//                                           `model`: epik_amd_edgemodel [T][N], epik_amd_edgemodel_info, float64
//                                           stat[T][2][N][P + 1], float64 max[T][2][P + 1], uint8 aliased[64];
//                                           edgemodel-strata: with <strata.bin> after the design
//   cohort_test edgemodel-tsv <out.tsv> <in.bin> <names.txt> <design.tsv> <terms> <P> <seed>
//                                           the file of --cohort-edge-model, as model-tsv
//   cohort_test mantel <out.bin> <in.bin> <sides.bin> <strata.bin or -> <P> <seed>
//                                           the Mantel tests of a `kr` input with a `sides` file, uint64 Mv, Mm, methods, control
//                                           (0xffffffff: none), float64 values[Mv][S], float64 matrices[Mm][S][S], uint8
//                                           present[Mm][S]: epik_amd_mantel [tests], float64 stat[tests][P + 1]
//   cohort_test anosim <out.bin> <in.bin> <labels.bin> <strata.bin or -> <P> <seed>
//                                           ANOSIM of a `kr` input with a raw `labels` file, uint32 [S][M]: epik_amd_anosim [M],
//                                           float64 stat[M][P + 1]
// An `add` input holds, little endian: uint64 n, keep, num_branches, num_samples; epik_amd_placement rows[n][keep];
// uint32 n_rows[n]; uint32 kmer_counts[n][keep]; uint32 weights[n]; uint32 samples[n].
// A `kr` input: uint64 num_samples, num_branches; uint64 mass[S][N]; uint32 first[N]; float64 branch_length[N].
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "cohort.hpp"

namespace {

template <typename T>
std::vector<T> read_array(std::ifstream& in, size_t count)
{
    std::vector<T> v(count);
    in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T)));
    if (!in) throw std::runtime_error("input file too short");
    return v;
}

template <typename T>
void write_array(std::ofstream& out, const T* data, size_t count)
{
    out.write(reinterpret_cast<const char*>(data), (std::streamsize)(count * sizeof(T)));
}

// the strata of the `*-strata` modes: uint32 [S], any value an id
std::vector<uint32_t> read_strata(const char* path, uint64_t S)
{
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    if (!in) throw std::runtime_error(std::string("cannot open ") + path);
    if ((uint64_t)in.tellg() != S * sizeof(uint32_t)) throw std::runtime_error("the strata file is not uint32 [S]");
    in.seekg(0);
    return read_array<uint32_t>(in, S);
}

}  // namespace

int main(int argc, char** argv)
{
    try {
        if (argc >= 4 && std::strcmp(argv[1], "add") == 0) {
            epik_amd::sample_cohort total;
            for (int i = 3; i < argc; ++i) {
                std::ifstream in(argv[i], std::ios::binary);
                if (!in) throw std::runtime_error(std::string("cannot open ") + argv[i]);
                const auto head = read_array<uint64_t>(in, 4);
                const uint64_t n = head[0], keep = head[1];
                const auto rows = read_array<epik_amd_placement>(in, n * keep);
                const auto n_rows = read_array<uint32_t>(in, n);
                const auto counts = read_array<uint32_t>(in, n * keep);
                const auto weights = read_array<uint32_t>(in, n);
                const auto samples = read_array<uint32_t>(in, n);
                epik_amd::sample_cohort part((uint32_t)head[3], (uint32_t)head[2]);
                part.add_rows(rows.data(), n_rows.data(), counts.data(), weights.data(), samples.data(), n, (uint32_t)keep);
                if (i == 3)
                    total = part;
                else
                    total.merge(part);
            }
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, total.mass.data(), total.mass.size());
            write_array(out, total.best.data(), total.best.size());
            write_array(out, total.totals.data(), total.totals.size());
            write_array(out, &total.bad_samples, 1);
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if (argc == 4 && std::strcmp(argv[1], "kr") == 0) {
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            const auto mass = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const auto length = read_array<double>(in, N);
            std::vector<double> kr(S * S);
            std::string err;
            if (epik_amd::kr_matrix(mass.data(), (uint32_t)S, (uint32_t)N, first.data(), length.data(), kr.data(), err) != 0)
                throw std::runtime_error(err);
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, kr.data(), kr.size());
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if (argc == 5 && std::strcmp(argv[1], "unifrac") == 0) {
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            const auto mass = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const auto length = read_array<double>(in, N);
            std::vector<double> matrix(S * S);
            std::string err;
            if (epik_amd::unifrac_matrix(mass.data(), (uint32_t)S, (uint32_t)N, first.data(), length.data(),
                                         (uint32_t)std::strtoul(argv[4], nullptr, 10), matrix.data(), err) != 0)
                throw std::runtime_error(err);
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, matrix.data(), matrix.size());
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if (argc == 4 && std::strcmp(argv[1], "squash") == 0) {
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            if (S == 0) throw std::runtime_error("no sample");
            const auto mass = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const auto length = read_array<double>(in, N);
            std::vector<epik_amd_squash_merge> merges(S - 1);
            uint32_t num_merges = 0;
            std::string err;
            if (epik_amd::squash_merges(mass.data(), (uint32_t)S, (uint32_t)N, first.data(), length.data(), merges.data(),
                                        &num_merges, err) != 0)
                throw std::runtime_error(err);
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, merges.data(), merges.size());
            write_array(out, &num_merges, 1);
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if (argc == 5 && std::strcmp(argv[1], "epca") == 0) {
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            if (S == 0) throw std::runtime_error("no sample");
            const auto mass = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const unsigned long K = std::stoul(argv[4]);
            if (K < 1 || K > EPIK_AMD_EPCA_MAX_COMPONENTS) throw std::runtime_error("num_components = " + std::to_string(K) + " is outside [1, 64]");
            std::vector<double> mu(K), proj(S * K), edge(K * N);
            epik_amd_epca_info info{};
            std::string err;
            if (epik_amd::epca_components(mass.data(), (uint32_t)S, (uint32_t)N, first.data(), (uint32_t)K, mu.data(), proj.data(),
                                          edge.data(), &info, err) != 0)
                throw std::runtime_error(err);
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, mu.data(), mu.size());
            write_array(out, proj.data(), proj.size());
            write_array(out, edge.data(), edge.size());
            write_array(out, &info, 1);
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if ((argc == 5 && std::strcmp(argv[1], "pcoa") == 0) || (argc == 6 && std::strcmp(argv[1], "pcoa-tsv") == 0)) {
            const bool tsv = argc == 6;
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            if (S == 0) throw std::runtime_error("no sample");
            const auto mass = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const auto length = read_array<double>(in, N);
            const unsigned long K = std::stoul(argv[argc - 1]);
            if (K < 1 || K > EPIK_AMD_PCOA_MAX_COMPONENTS) throw std::runtime_error("num_components = " + std::to_string(K) + " is outside [1, 64]");
            std::vector<double> mu(S), coord(S * K);
            epik_amd_pcoa_info info{};
            std::string err;
            if (epik_amd::pcoa_components(mass.data(), (uint32_t)S, (uint32_t)N, first.data(), length.data(), (uint32_t)K, mu.data(),
                                          coord.data(), &info, err) != 0)
                throw std::runtime_error(err);
            if (tsv) {
                std::vector<epik_amd::cohort_sample> samples;
                std::ifstream names(argv[4]);
                if (!names) throw std::runtime_error(std::string("cannot open ") + argv[4]);
                for (std::string line; std::getline(names, line);) samples.push_back({line, ""});
                if (samples.size() != S) throw std::runtime_error("the names file does not name every sample");
                std::vector<uint64_t> totals(S, 0);
                for (uint64_t s = 0; s < S; ++s)
                    for (uint64_t b = 0; b < N; ++b) totals[s] += mass[s * N + b];
                epik_amd::write_through_part(argv[2], epik_amd::format_pcoa_tsv(samples, totals.data(), (uint32_t)K, mu.data(),
                                                                                coord.data(), info));
                return 0;
            }
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, mu.data(), mu.size());
            write_array(out, coord.data(), coord.size());
            write_array(out, &info, 1);
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if (argc == 6 && std::strcmp(argv[1], "kmeans") == 0) {
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            if (S == 0) throw std::runtime_error("no sample");
            const auto mass = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const auto length = read_array<double>(in, N);
            const unsigned long K = std::stoul(argv[4]), max_iterations = std::stoul(argv[5]);
            if (K < 1 || K > EPIK_AMD_KMEANS_MAX_CLUSTERS) throw std::runtime_error("num_clusters = " + std::to_string(K) + " is outside [1, 64]");
            if (max_iterations < 1 || max_iterations > EPIK_AMD_KMEANS_MAX_ITERATIONS)
                throw std::runtime_error("max_iterations = " + std::to_string(max_iterations) + " is outside [1, 1000]");
            std::vector<epik_amd_kmeans_sample> samples(S);
            std::vector<epik_amd_kmeans_cluster> clusters(K);
            std::vector<double> centroids(K * N);
            epik_amd_kmeans_info info{};
            std::string err;
            if (epik_amd::kmeans_clusters(mass.data(), (uint32_t)S, (uint32_t)N, first.data(), length.data(), (uint32_t)K,
                                          (uint32_t)max_iterations, samples.data(), clusters.data(), centroids.data(), &info, err) != 0)
                throw std::runtime_error(err);
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, samples.data(), samples.size());
            write_array(out, clusters.data(), clusters.size());
            write_array(out, centroids.data(), centroids.size());
            write_array(out, &info, 1);
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if ((argc == 4 && std::strcmp(argv[1], "alpha") == 0) || (argc == 6 && std::strcmp(argv[1], "rarefy") == 0)) {
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            if (S == 0) throw std::runtime_error("no sample");
            const auto cells = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const auto length = read_array<double>(in, N);
            std::string err;
            std::ofstream out;
            if (argc == 4) {
                std::vector<epik_amd_alpha> alpha(S);
                if (epik_amd::alpha_indices(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), length.data(), alpha.data(), err) != 0)
                    throw std::runtime_error(err);
                out.open(argv[2], std::ios::binary);
                write_array(out, alpha.data(), alpha.size());
            } else {
                const unsigned long step = std::stoul(argv[4]), depths = std::stoul(argv[5]);
                if (step > 0xfffffffful || depths > 0xfffffffful) throw std::runtime_error("depth_step and num_depths must fit 32 bits");
                if (epik_amd::rarefy_depths_valid((uint32_t)step, (uint32_t)depths, err) != 0) throw std::runtime_error(err);
                std::vector<double> curve(S * depths * 2);
                if (epik_amd::rarefy_curves(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), length.data(), (uint32_t)step,
                                            (uint32_t)depths, curve.data(), err) != 0)
                    throw std::runtime_error(err);
                out.open(argv[2], std::ios::binary);
                write_array(out, curve.data(), curve.size());
            }
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if ((argc == 5 && std::strcmp(argv[1], "correlation") == 0) || (argc == 4 && std::strcmp(argv[1], "dispersion") == 0)) {
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            if (S == 0) throw std::runtime_error("no sample");
            const auto cells = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            std::string err;
            std::ofstream out;
            if (argc == 5) {
                std::ifstream meta_in(argv[4], std::ios::binary | std::ios::ate);
                if (!meta_in) throw std::runtime_error(std::string("cannot open ") + argv[4]);
                const uint64_t bytes = (uint64_t)meta_in.tellg();
                meta_in.seekg(0);
                if (bytes == 0 || bytes % (S * sizeof(double)) != 0) throw std::runtime_error("the meta file is not float64 [S][M]");
                const uint64_t M = bytes / (S * sizeof(double));
                if (M > EPIK_AMD_CORRELATION_MAX_COLUMNS) throw std::runtime_error("the meta file has more than 64 columns");
                const auto meta = read_array<double>(meta_in, S * M);
                std::vector<epik_amd_correlation> records(M * N);
                std::vector<uint32_t> used(M);
                if (epik_amd::correlation_records(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), meta.data(), (uint32_t)M,
                                                  records.data(), used.data(), err) != 0)
                    throw std::runtime_error(err);
                out.open(argv[2], std::ios::binary);
                write_array(out, records.data(), records.size());
                write_array(out, used.data(), used.size());
            } else {
                std::vector<epik_amd_dispersion> records(N);
                if (epik_amd::dispersion_records(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), records.data(), err) != 0)
                    throw std::runtime_error(err);
                out.open(argv[2], std::ios::binary);
                write_array(out, records.data(), records.size());
            }
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if ((argc == 8 && (std::strcmp(argv[1], "permanova") == 0 || std::strcmp(argv[1], "permdisp") == 0)) ||
            (argc == 9 && (std::strcmp(argv[1], "permanova-tsv") == 0 || std::strcmp(argv[1], "permdisp-tsv") == 0)) ||
            (argc == 9 && (std::strcmp(argv[1], "permanova-strata") == 0 || std::strcmp(argv[1], "permdisp-strata") == 0))) {
            const bool stratified = std::strstr(argv[1], "-strata") != nullptr;
            const bool tsv = argc == 9 && !stratified, disp = std::strncmp(argv[1], "permdisp", 8) == 0;
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            if (S == 0) throw std::runtime_error("no sample");
            const auto cells = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const auto lengths = read_array<double>(in, N);
            const uint32_t P = (uint32_t)std::strtoul(argv[argc - 3], nullptr, 10);
            const uint64_t seed = std::strtoull(argv[argc - 2], nullptr, 10);
            const bool pairwise = std::strcmp(argv[argc - 1], "0") != 0;
            std::vector<uint32_t> labels, strata;
            if (stratified) strata = read_strata(argv[5], S);
            const uint32_t* within = stratified ? strata.data() : nullptr;
            epik_amd::cohort_factors factors;
            std::vector<epik_amd::cohort_sample> samples;
            if (tsv) {
                std::ifstream names(argv[4]);
                if (!names) throw std::runtime_error(std::string("cannot open ") + argv[4]);
                for (std::string line; std::getline(names, line);) samples.push_back({line, ""});
                if (samples.size() != S) throw std::runtime_error("the names file does not name every sample");
                factors = disp ? epik_amd::read_cohort_factors(argv[5], samples, false, EPIK_AMD_PERMDISP_MAX_GROUPS, "--cohort-permdisp")
                               : epik_amd::read_cohort_factors(argv[5], samples, pairwise);
                std::cout << "Cohort factors: " << factors.columns.size() << " columns, " << factors.skipped
                          << " lines of samples that are not in the list skipped" << std::endl;
                labels = factors.labels;
            } else {
                std::ifstream labels_in(argv[4], std::ios::binary | std::ios::ate);
                if (!labels_in) throw std::runtime_error(std::string("cannot open ") + argv[4]);
                const uint64_t bytes = (uint64_t)labels_in.tellg();
                labels_in.seekg(0);
                if (bytes == 0 || bytes % (S * sizeof(uint32_t)) != 0) throw std::runtime_error("the labels file is not uint32 [S][M]");
                labels = read_array<uint32_t>(labels_in, bytes / sizeof(uint32_t));
            }
            const uint64_t M = labels.size() / S;
            if (M > EPIK_AMD_PERMANOVA_MAX_COLUMNS) throw std::runtime_error("the labels file has more than 64 columns");
            if (P < 1 || P > EPIK_AMD_PERMANOVA_MAX_PERMUTATIONS) throw std::runtime_error("P is outside [1, 999999]");
            const uint64_t tests = M * (1 + (pairwise ? EPIK_AMD_PERMANOVA_PAIR_SLOTS : 0));
            if (disp) {
                std::vector<epik_amd_permdisp> records(tests);
                std::vector<double> stat(tsv ? 0 : tests * ((uint64_t)P + 1)), group_mean(M * EPIK_AMD_PERMDISP_MAX_GROUPS), z(M * S);
                std::string err;
                if (epik_amd::permdisp_records(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), lengths.data(), labels.data(),
                                               (uint32_t)M, P, seed, pairwise, records.data(), tsv ? nullptr : stat.data(),
                                               group_mean.data(), z.data(), err, EPIK_AMD_DISTANCE_KR, within) != 0)
                    throw std::runtime_error(err);
                if (tsv) {
                    std::vector<uint64_t> totals(S, 0);
                    for (uint64_t s = 0; s < S; ++s)
                        for (uint64_t b = 0; b < N; ++b) totals[s] += cells[s * N + b];
                    epik_amd::write_through_part(argv[2], epik_amd::format_permdisp_tsv(samples, totals.data(), factors.columns, factors.names,
                                                                                        labels.data(), P, seed, pairwise, records.data(),
                                                                                        group_mean.data(), z.data()));
                    return 0;
                }
                std::ofstream out(argv[2], std::ios::binary);
                write_array(out, records.data(), records.size());
                write_array(out, stat.data(), stat.size());
                write_array(out, group_mean.data(), group_mean.size());
                write_array(out, z.data(), z.size());
                if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
                return 0;
            }
            std::vector<epik_amd_permanova> records(tests);
            std::vector<double> ssw(tsv ? 0 : tests * ((uint64_t)P + 1)), group_ss(M * EPIK_AMD_PERMANOVA_MAX_GROUPS);
            std::string err;
            if (epik_amd::permanova_records(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), lengths.data(), labels.data(),
                                            (uint32_t)M, P, seed, pairwise, records.data(), tsv ? nullptr : ssw.data(), group_ss.data(),
                                            err, EPIK_AMD_DISTANCE_KR, within) != 0)
                throw std::runtime_error(err);
            if (tsv) {
                std::vector<uint64_t> totals(S, 0);
                for (uint64_t s = 0; s < S; ++s)
                    for (uint64_t b = 0; b < N; ++b) totals[s] += cells[s * N + b];
                epik_amd::write_through_part(argv[2], epik_amd::format_permanova_tsv(samples, totals.data(), factors.columns, factors.names,
                                                                                     labels.data(), P, seed, pairwise, records.data(),
                                                                                     group_ss.data()));
                return 0;
            }
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, records.data(), records.size());
            write_array(out, ssw.data(), ssw.size());
            write_array(out, group_ss.data(), group_ss.size());
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if ((argc == 7 && std::strcmp(argv[1], "edgetest") == 0) || (argc == 8 && std::strcmp(argv[1], "edgetest-tsv") == 0) ||
            (argc == 8 && std::strcmp(argv[1], "edgetest-strata") == 0)) {
            const bool stratified = std::strcmp(argv[1], "edgetest-strata") == 0, tsv = argc == 8 && !stratified;
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            if (S == 0) throw std::runtime_error("no sample");
            const auto cells = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const uint32_t P = (uint32_t)std::strtoul(argv[argc - 2], nullptr, 10);
            const uint64_t seed = std::strtoull(argv[argc - 1], nullptr, 10);
            std::vector<uint32_t> labels, strata;
            if (stratified) strata = read_strata(argv[5], S);
            epik_amd::cohort_factors factors;
            std::vector<epik_amd::cohort_sample> samples;
            if (tsv) {
                std::ifstream names(argv[4]);
                if (!names) throw std::runtime_error(std::string("cannot open ") + argv[4]);
                for (std::string line; std::getline(names, line);) samples.push_back({line, ""});
                if (samples.size() != S) throw std::runtime_error("the names file does not name every sample");
                factors = epik_amd::read_cohort_factors(argv[5], samples, false, EPIK_AMD_EDGETEST_MAX_GROUPS, "--cohort-edge-test");
                std::cout << "Cohort edge-test factors: " << factors.columns.size() << " columns, " << factors.skipped
                          << " lines of samples that are not in the list skipped" << std::endl;
                labels = factors.labels;
            } else {
                std::ifstream labels_in(argv[4], std::ios::binary | std::ios::ate);
                if (!labels_in) throw std::runtime_error(std::string("cannot open ") + argv[4]);
                const uint64_t bytes = (uint64_t)labels_in.tellg();
                labels_in.seekg(0);
                if (bytes == 0 || bytes % (S * sizeof(uint32_t)) != 0) throw std::runtime_error("the labels file is not uint32 [S][M]");
                labels = read_array<uint32_t>(labels_in, bytes / sizeof(uint32_t));
            }
            const uint64_t M = labels.size() / S, row = (uint64_t)P + 1;
            if (M > EPIK_AMD_EDGETEST_MAX_COLUMNS) throw std::runtime_error("the labels file has more than 64 columns");
            if (P < 1 || P > EPIK_AMD_EDGETEST_MAX_PERMUTATIONS) throw std::runtime_error("P is outside [1, 999999]");
            std::vector<epik_amd_edgetest> records(M * N);
            std::vector<double> stat(tsv ? 0 : M * EPIK_AMD_EDGETEST_FAMILIES * N * row), max(tsv ? 0 : M * EPIK_AMD_EDGETEST_FAMILIES * row);
            std::string err;
            if (epik_amd::edgetest_records(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), labels.data(), (uint32_t)M, P, seed,
                                           records.data(), tsv ? nullptr : stat.data(), tsv ? nullptr : max.data(), err,
                                           stratified ? strata.data() : nullptr) != 0)
                throw std::runtime_error(err);
            if (tsv) {
                std::vector<uint64_t> totals(S, 0);
                for (uint64_t s = 0; s < S; ++s)
                    for (uint64_t b = 0; b < N; ++b) totals[s] += cells[s * N + b];
                epik_amd::write_through_part(argv[2], epik_amd::format_edgetest_tsv(samples, totals.data(), factors.columns, factors.names,
                                                                                    labels.data(), (uint32_t)N, P, seed, records.data()));
                return 0;
            }
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, records.data(), records.size());
            write_array(out, stat.data(), stat.size());
            write_array(out, max.data(), max.size());
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if (argc == 9 && std::strcmp(argv[1], "model-tsv") == 0) {
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            if (S == 0) throw std::runtime_error("no sample");
            const auto cells = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const auto lengths = read_array<double>(in, N);
            const uint32_t P = (uint32_t)std::strtoul(argv[7], nullptr, 10);
            const uint64_t seed = std::strtoull(argv[8], nullptr, 10);
            std::vector<epik_amd::cohort_sample> samples;
            std::ifstream names(argv[4]);
            if (!names) throw std::runtime_error(std::string("cannot open ") + argv[4]);
            for (std::string line; std::getline(names, line);) samples.push_back({line, ""});
            if (samples.size() != S) throw std::runtime_error("the names file does not name every sample");
            const epik_amd::cohort_design design = epik_amd::read_cohort_design(argv[5], argv[6], samples);
            std::cout << "Cohort model design: " << design.terms.size() << " terms, " << design.skipped
                      << " lines of samples that are not in the list skipped" << std::endl;
            const size_t T = design.terms.size();
            std::vector<epik_amd_model_term> records(T + 1);
            epik_amd_model_info info{};
            std::vector<uint8_t> aliased(EPIK_AMD_MODEL_MAX_COLUMNS);
            std::string err;
            if (epik_amd::model_records(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), lengths.data(), design.kind.data(),
                                        design.labels.data(), design.values.data(), (uint32_t)T, P, seed, records.data(), &info, nullptr,
                                        aliased.data(), err) != 0)
                throw std::runtime_error(err);
            std::vector<uint64_t> totals(S, 0);
            for (uint64_t s = 0; s < S; ++s)
                for (uint64_t b = 0; b < N; ++b) totals[s] += cells[s * N + b];
            epik_amd::write_through_part(argv[2], epik_amd::format_model_tsv(samples, totals.data(), design, P, seed, records.data(), info,
                                                                             aliased.data()));
            return 0;
        }
        if (argc == 9 && std::strcmp(argv[1], "edgemodel-tsv") == 0) {
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            if (S == 0) throw std::runtime_error("no sample");
            const auto cells = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const uint32_t P = (uint32_t)std::strtoul(argv[7], nullptr, 10);
            const uint64_t seed = std::strtoull(argv[8], nullptr, 10);
            std::vector<epik_amd::cohort_sample> samples;
            std::ifstream names(argv[4]);
            if (!names) throw std::runtime_error(std::string("cannot open ") + argv[4]);
            for (std::string line; std::getline(names, line);) samples.push_back({line, ""});
            if (samples.size() != S) throw std::runtime_error("the names file does not name every sample");
            const epik_amd::cohort_design design = epik_amd::read_cohort_design(argv[5], argv[6], samples);
            std::cout << "Cohort edge model design: " << design.terms.size() << " terms, " << design.skipped
                      << " lines of samples that are not in the list skipped" << std::endl;
            const size_t T = design.terms.size();
            std::vector<epik_amd_edgemodel> records(T * N);
            epik_amd_edgemodel_info info{};
            std::vector<uint8_t> aliased(EPIK_AMD_MODEL_MAX_COLUMNS);
            std::string err;
            if (epik_amd::edgemodel_records(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), design.kind.data(), design.labels.data(),
                                            design.values.data(), (uint32_t)T, P, seed, records.data(), &info, nullptr, nullptr,
                                            aliased.data(), err) != 0)
                throw std::runtime_error(err);
            std::vector<uint64_t> totals(S, 0);
            for (uint64_t s = 0; s < S; ++s)
                for (uint64_t b = 0; b < N; ++b) totals[s] += cells[s * N + b];
            epik_amd::write_through_part(argv[2], epik_amd::format_edgemodel_tsv(samples, totals.data(), design, (uint32_t)N, P, seed,
                                                                                 records.data(), info, aliased.data()));
            return 0;
        }
        if ((argc == 7 && std::strcmp(argv[1], "model") == 0) || (argc == 8 && std::strcmp(argv[1], "model-strata") == 0)) {
            const bool stratified = argc == 8;
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            if (S == 0) throw std::runtime_error("no sample");
            const auto cells = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const auto lengths = read_array<double>(in, N);
            const uint32_t P = (uint32_t)std::strtoul(argv[argc - 2], nullptr, 10);
            const uint64_t seed = std::strtoull(argv[argc - 1], nullptr, 10);
            std::vector<uint32_t> strata;
            if (stratified) strata = read_strata(argv[5], S);
            std::ifstream design(argv[4], std::ios::binary);
            if (!design) throw std::runtime_error(std::string("cannot open ") + argv[4]);
            const uint64_t T = read_array<uint64_t>(design, 1)[0];
            if (T < 1 || T > EPIK_AMD_MODEL_MAX_TERMS) throw std::runtime_error("the design file has a number of terms outside [1, 16]");
            if (P < 1 || P > EPIK_AMD_MODEL_MAX_PERMUTATIONS) throw std::runtime_error("P is outside [1, 999999]");
            const auto kind = read_array<uint32_t>(design, T);
            const auto labels = read_array<uint32_t>(design, S * T);
            const auto values = read_array<double>(design, S * T);
            std::vector<epik_amd_model_term> records(T + 1);
            epik_amd_model_info info{};
            std::vector<double> stat((T + 1) * ((uint64_t)P + 1));
            std::vector<uint8_t> aliased(EPIK_AMD_MODEL_MAX_COLUMNS);
            std::string err;
            if (epik_amd::model_records(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), lengths.data(), kind.data(), labels.data(),
                                        values.data(), (uint32_t)T, P, seed, records.data(), &info, stat.data(), aliased.data(), err,
                                        EPIK_AMD_DISTANCE_KR, stratified ? strata.data() : nullptr) != 0)
                throw std::runtime_error(err);
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, records.data(), records.size());
            write_array(out, &info, 1);
            write_array(out, stat.data(), stat.size());
            write_array(out, aliased.data(), aliased.size());
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if ((argc == 7 && std::strcmp(argv[1], "edgemodel") == 0) || (argc == 8 && std::strcmp(argv[1], "edgemodel-strata") == 0)) {
            const bool stratified = argc == 8;
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            if (S == 0) throw std::runtime_error("no sample");
            const auto cells = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const uint32_t P = (uint32_t)std::strtoul(argv[argc - 2], nullptr, 10);
            const uint64_t seed = std::strtoull(argv[argc - 1], nullptr, 10);
            std::vector<uint32_t> strata;
            if (stratified) strata = read_strata(argv[5], S);
            std::ifstream design(argv[4], std::ios::binary);
            if (!design) throw std::runtime_error(std::string("cannot open ") + argv[4]);
            const uint64_t T = read_array<uint64_t>(design, 1)[0];
            if (T < 1 || T > EPIK_AMD_MODEL_MAX_TERMS) throw std::runtime_error("the design file has a number of terms outside [1, 16]");
            if (P < 1 || P > EPIK_AMD_MODEL_MAX_PERMUTATIONS) throw std::runtime_error("P is outside [1, 999999]");
            const auto kind = read_array<uint32_t>(design, T);
            const auto labels = read_array<uint32_t>(design, S * T);
            const auto values = read_array<double>(design, S * T);
            const uint64_t row = (uint64_t)P + 1;
            std::vector<epik_amd_edgemodel> records(T * N);
            epik_amd_edgemodel_info info{};
            std::vector<double> stat(T * EPIK_AMD_EDGEMODEL_FAMILIES * N * row), most(T * EPIK_AMD_EDGEMODEL_FAMILIES * row);
            std::vector<uint8_t> aliased(EPIK_AMD_MODEL_MAX_COLUMNS);
            std::string err;
            if (epik_amd::edgemodel_records(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), kind.data(), labels.data(), values.data(),
                                            (uint32_t)T, P, seed, records.data(), &info, stat.data(), most.data(), aliased.data(), err,
                                            stratified ? strata.data() : nullptr) != 0)
                throw std::runtime_error(err);
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, records.data(), records.size());
            write_array(out, &info, 1);
            write_array(out, stat.data(), stat.size());
            write_array(out, most.data(), most.size());
            write_array(out, aliased.data(), aliased.size());
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if (argc == 8 && (std::strcmp(argv[1], "mantel") == 0 || std::strcmp(argv[1], "anosim") == 0)) {
            const bool ranked = std::strcmp(argv[1], "anosim") == 0;
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            if (S == 0) throw std::runtime_error("no sample");
            const auto cells = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const auto lengths = read_array<double>(in, N);
            const uint32_t P = (uint32_t)std::strtoul(argv[6], nullptr, 10);
            const uint64_t seed = std::strtoull(argv[7], nullptr, 10);
            if (P < 1 || P > EPIK_AMD_PERMANOVA_MAX_PERMUTATIONS) throw std::runtime_error("P is outside [1, 999999]");
            std::vector<uint32_t> strata;
            const bool stratified = std::strcmp(argv[5], "-") != 0;
            if (stratified) strata = read_strata(argv[5], S);
            std::ifstream side(argv[4], std::ios::binary | std::ios::ate);
            if (!side) throw std::runtime_error(std::string("cannot open ") + argv[4]);
            const uint64_t bytes = (uint64_t)side.tellg();
            side.seekg(0);
            std::string err;
            std::ofstream out(argv[2], std::ios::binary);
            if (ranked) {
                if (bytes == 0 || bytes % (S * sizeof(uint32_t)) != 0) throw std::runtime_error("the labels file is not uint32 [S][M]");
                const uint64_t M = bytes / (S * sizeof(uint32_t));
                if (M > EPIK_AMD_PERMANOVA_MAX_COLUMNS) throw std::runtime_error("the labels file has more than 64 columns");
                const auto labels = read_array<uint32_t>(side, S * M);
                std::vector<epik_amd_anosim> records(M);
                std::vector<double> stat(M * ((uint64_t)P + 1));
                if (epik_amd::anosim_records(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), lengths.data(), labels.data(), (uint32_t)M,
                                             P, seed, records.data(), stat.data(), err, EPIK_AMD_DISTANCE_KR,
                                             stratified ? strata.data() : nullptr) != 0)
                    throw std::runtime_error(err);
                write_array(out, records.data(), records.size());
                write_array(out, stat.data(), stat.size());
            } else {
                const auto shape = read_array<uint64_t>(side, 4);  // Mv, Mm, methods, control
                if (shape[0] > EPIK_AMD_MANTEL_MAX_COLUMNS || shape[1] > EPIK_AMD_MANTEL_MAX_MATRICES)
                    throw std::runtime_error("the sides file has more than 64 columns or 8 matrices");
                const auto values = read_array<double>(side, shape[0] * S);
                const auto matrices = read_array<double>(side, shape[1] * S * S);
                const auto present = read_array<uint8_t>(side, shape[1] * S);
                const epik_amd::mantel_sides sides{values.data(), (uint32_t)shape[0], matrices.data(), present.data(), (uint32_t)shape[1],
                                                   (uint32_t)shape[2], (uint32_t)shape[3]};
                if (const int rc = epik_amd::mantel_arguments_valid(sides, (uint32_t)S, P, err); rc != 0) throw std::runtime_error(err);
                std::vector<epik_amd_mantel> records(sides.tests());
                std::vector<double> stat(records.size() * ((uint64_t)P + 1));
                if (epik_amd::mantel_records(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), lengths.data(), sides, P, seed,
                                             records.data(), stat.data(), err, EPIK_AMD_DISTANCE_KR,
                                             stratified ? strata.data() : nullptr) != 0)
                    throw std::runtime_error(err);
                write_array(out, records.data(), records.size());
                write_array(out, stat.data(), stat.size());
            }
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        // the files of --cohort-mantel and --cohort-anosim for a `kr` input whose samples are named by the lines of names.txt, through
        // the drivers' readers and formatters: mantel-tsv <out.tsv> <in.bin> <names.txt> <meta.tsv or -> <NAME=FILE,... or ->
        // <pearson|spearman|both> <partial NAME or -> <P> <seed>; anosim-tsv <out.tsv> <in.bin> <names.txt> <factors.tsv> <P> <seed>
        if ((argc == 11 && std::strcmp(argv[1], "mantel-tsv") == 0) || (argc == 8 && std::strcmp(argv[1], "anosim-tsv") == 0)) {
            const bool ranked = argc == 8;
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const auto head = read_array<uint64_t>(in, 2);
            const uint64_t S = head[0], N = head[1];
            const auto cells = read_array<uint64_t>(in, S * N);
            const auto first = read_array<uint32_t>(in, N);
            const auto lengths = read_array<double>(in, N);
            std::vector<epik_amd::cohort_sample> samples;
            std::ifstream names(argv[4]);
            if (!names) throw std::runtime_error(std::string("cannot open ") + argv[4]);
            for (std::string line; std::getline(names, line);) samples.push_back({line, ""});
            if (samples.size() != S) throw std::runtime_error("names.txt does not name the samples of the input");
            const uint32_t P = (uint32_t)std::strtoul(argv[argc - 2], nullptr, 10);
            const uint64_t seed = std::strtoull(argv[argc - 1], nullptr, 10);
            std::vector<uint64_t> totals(S, 0);
            for (size_t s = 0; s < S; ++s)
                for (size_t b = 0; b < N; ++b) totals[s] += cells[s * N + b];
            std::string err;
            if (ranked) {
                const auto factors = epik_amd::read_cohort_factors(argv[5], samples, false, 0, "--cohort-anosim");
                std::vector<epik_amd_anosim> records(factors.columns.size());
                if (epik_amd::anosim_records(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), lengths.data(), factors.labels.data(),
                                             (uint32_t)factors.columns.size(), P, seed, records.data(), nullptr, err) != 0)
                    throw std::runtime_error(err);
                epik_amd::write_through_part(argv[2], epik_amd::format_anosim_tsv(samples, totals.data(), factors.columns, factors.names,
                                                                                  factors.labels.data(), P, seed, records.data()));
                return 0;
            }
            std::vector<std::string> matrices;
            if (std::strcmp(argv[6], "-") != 0) {
                std::string list = argv[6];
                for (size_t at = 0; at <= list.size();) {
                    const size_t comma = std::min(list.find(',', at), list.size());
                    matrices.push_back(list.substr(at, comma - at));
                    at = comma + 1;
                }
            }
            const uint32_t methods = epik_amd::mantel_methods_of_name(argv[7]);
            if (!methods) throw std::runtime_error("the method must be pearson, spearman or both");
            const auto read = epik_amd::read_cohort_mantel_sides(std::strcmp(argv[5], "-") == 0 ? "" : argv[5], matrices,
                                                                 std::strcmp(argv[8], "-") == 0 ? "" : argv[8], samples);
            const epik_amd::mantel_sides sides = read.sides(methods);
            std::vector<epik_amd_mantel> records(sides.tests());
            if (epik_amd::mantel_records(cells.data(), (uint32_t)S, (uint32_t)N, first.data(), lengths.data(), sides, P, seed,
                                         records.data(), nullptr, err) != 0)
                throw std::runtime_error(err);
            epik_amd::write_through_part(argv[2], epik_amd::format_mantel_tsv(samples, totals.data(), read.names, read.num_columns, methods,
                                                                              read.control, P, seed, records.data()));
            return 0;
        }
        // the drivers' strata reader and header field: strata-read <out.bin> <names.txt> <strata.tsv> <column or -> writes
        // strata[S] and, after them, the column's name; strata-field <out.tsv> <in.tsv> <NAME> the file with the field
        if (argc == 6 && std::strcmp(argv[1], "strata-read") == 0) {
            std::vector<epik_amd::cohort_sample> samples;
            std::ifstream names(argv[3]);
            if (!names) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            for (std::string line; std::getline(names, line);) samples.push_back({line, ""});
            std::string name;
            const auto strata = epik_amd::read_cohort_strata(argv[4], std::strcmp(argv[5], "-") == 0 ? "" : argv[5], samples, &name);
            std::ofstream out(argv[2], std::ios::binary);
            write_array(out, strata.data(), strata.size());
            out << name;
            if (!out) throw std::runtime_error(std::string("cannot write ") + argv[2]);
            return 0;
        }
        if (argc == 5 && std::strcmp(argv[1], "strata-field") == 0) {
            std::ifstream in(argv[3], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("cannot open ") + argv[3]);
            const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            epik_amd::write_through_part(argv[2], epik_amd::with_strata_field(text, argv[4]));
            return 0;
        }
        std::cerr << "usage: cohort_test add <out.bin> <in.bin>... | kr <out.bin> <in.bin> | squash <out.bin> <in.bin> | "
                     "epca <out.bin> <in.bin> <K> | pcoa <out.bin> <in.bin> <K> | pcoa-tsv <out.tsv> <in.bin> <names.txt> <K> | kmeans <out.bin> <in.bin> <K> <max_iterations> | alpha <out.bin> <in.bin> | "
                     "rarefy <out.bin> <in.bin> <depth_step> <num_depths> | correlation <out.bin> <in.bin> <meta.bin> | "
                     "dispersion <out.bin> <in.bin> | permanova <out.bin> <in.bin> <labels.bin> <P> <seed> <pairwise> | "
                     "permanova-tsv <out.tsv> <in.bin> <names.txt> <factors.tsv> <P> <seed> <pairwise> | "
                     "permdisp <out.bin> <in.bin> <labels.bin> <P> <seed> <pairwise> | "
                     "permdisp-tsv <out.tsv> <in.bin> <names.txt> <factors.tsv> <P> <seed> <pairwise> | "
                     "edgetest <out.bin> <in.bin> <labels.bin> <P> <seed> | "
                     "edgetest-tsv <out.tsv> <in.bin> <names.txt> <factors.tsv> <P> <seed> | "
                     "model <out.bin> <in.bin> <design.bin> <P> <seed> | "
                     "model-tsv <out.tsv> <in.bin> <names.txt> <design.tsv> <terms> <P> <seed> | "
                     "permanova-strata | permdisp-strata <out.bin> <in.bin> <labels.bin> <strata.bin> <P> <seed> <pairwise> | "
                     "edgetest-strata <out.bin> <in.bin> <labels.bin> <strata.bin> <P> <seed> | "
                     "model-strata <out.bin> <in.bin> <design.bin> <strata.bin> <P> <seed> | "
                     "edgemodel <out.bin> <in.bin> <design.bin> <P> <seed> | "
                     "edgemodel-strata <out.bin> <in.bin> <design.bin> <strata.bin> <P> <seed> | "
                     "edgemodel-tsv <out.tsv> <in.bin> <names.txt> <design.tsv> <terms> <P> <seed> | "
                     "mantel <out.bin> <in.bin> <sides.bin> <strata.bin or -> <P> <seed> | "
                     "anosim <out.bin> <in.bin> <labels.bin> <strata.bin or -> <P> <seed> | "
                     "mantel-tsv <out.tsv> <in.bin> <names.txt> <meta.tsv or -> <NAME=FILE,... or -> <method> <partial or -> <P> <seed> | "
                     "anosim-tsv <out.tsv> <in.bin> <names.txt> <factors.tsv> <P> <seed> | "
                     "strata-read <out.bin> <names.txt> <strata.tsv> <column or -> | strata-field <out.tsv> <in.tsv> <NAME>\n";
        return 2;
    } catch (const std::exception& error) {
        std::cerr << "Error: " << error.what() << std::endl;
        return 1;
    }
}
