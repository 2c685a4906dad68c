// main.cpp -- the `epik-dna` / `epik-aa` drivers over the MI355X placer.
//
// Keeps the command line of the reference driver (epik/src/epik/main.cpp:209-222):
//   -d/--database  -q/--query  -j/--jobs  --batch-size  --omega  --mu  --max-ram
//   -o/--output-dir  --keep-at-most  --keep-factor  -h/--help
// with the same defaults (1, 2000, 1.5, 1.0, -, -, 7, 0.01), the same exit codes
// (0 / -1 on error, main.cpp:272,282,387,390), the same output file name
// (main.cpp:34-37) and the same final report lines (main.cpp:368-382).  Not reproduced:
// the progress bar and colours (indicators/termcolor).  Added: --gpus N | --devices a,b,c (the database on
// every device, batches shared out) and --db-shard G (the database cut in G by k-mer code, shard g on device g:
// every batch is placed by all of them together -- a database larger than one device's memory); --profile /
// --profile-only (the sample's abundance profile, profile.hpp: beside the jplace, or instead of it and summed on the
// devices); --mates FILE (paired-end reads: the second mates, one placement per pair); --assign [--assign-mass T] (per
// record the LCA clade that holds T of its placement mass and the EDPL, confidence.hpp, computed on the devices);
// --cohort (the query is a list of samples: their profiles and the KR distance between every two of them, cohort.hpp,
// summed and computed on the devices, no jplace); --windows W (long sequences painted by windows, windows.hpp: every
// window placed by itself and called for a group of --window-groups, segments and breakpoints, no jplace).
// The two binaries differ as the reference's do (epik/CMakeLists.txt:72,124): epik-dna
// accepts DNA databases, epik-aa protein ones.
#include <algorithm>
#include <cctype>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <exception>
#include <fstream>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "cohort.hpp"
#include "cohort_run.hpp"
#include "confidence.hpp"
#include "taxonomy.hpp"
#include "jplace.hpp"
#include "phylo_kmer_db.hpp"
#include "phylo_tree.hpp"
#include "placer.hpp"
#include "profile.hpp"
#include "report.hpp"
#include "seq_record.hpp"
#include "windows.hpp"

#ifndef EPIK_AMD_NO_MAIN
namespace {

/// Hand-over between two stages of the driver: at most `capacity` items wait; after close() push()
/// returns false and the pops return what is left, then false.
template <typename T>
class bounded_queue {
public:
    explicit bounded_queue(size_t capacity) : _capacity(capacity) {}
    bool push(T item)
    {
        std::unique_lock<std::mutex> lock(_mutex);
        _not_full.wait(lock, [&] { return _closed || _items.size() < _capacity; });
        if (_closed) return false;
        _items.push_back(std::move(item));
        _not_empty.notify_one();
        return true;
    }
    bool pop(T& item)
    {
        std::unique_lock<std::mutex> lock(_mutex);
        _not_empty.wait(lock, [&] { return _closed || !_items.empty(); });
        if (_items.empty()) return false;  // closed and drained
        item = std::move(_items.front());
        _items.pop_front();
        _not_full.notify_one();
        return true;
    }
    /// Waits for at least one item, then takes what is there, `max_items` at most, in order.
    /// False once the queue is closed and drained.
    bool pop_up_to(std::vector<T>& items, size_t max_items)
    {
        items.clear();
        std::unique_lock<std::mutex> lock(_mutex);
        _not_empty.wait(lock, [&] { return _closed || !_items.empty(); });
        while (!_items.empty() && items.size() < max_items) {
            items.push_back(std::move(_items.front()));
            _items.pop_front();
        }
        _not_full.notify_all();
        return !items.empty();
    }
    bool pop_all(std::vector<T>& items) { return pop_up_to(items, std::numeric_limits<size_t>::max()); }
    void close()
    {
        std::lock_guard<std::mutex> lock(_mutex);
        _closed = true;
        _not_full.notify_all();
        _not_empty.notify_all();
    }

private:
    std::mutex _mutex;
    std::condition_variable _not_full, _not_empty;
    std::deque<T> _items;
    size_t _capacity;
    bool _closed = false;
};

/// Busy time of one stage.
class stage_clock {
public:
    void start() { _begin = std::chrono::steady_clock::now(); }
    void stop() { _total += std::chrono::steady_clock::now() - _begin; }
    double ms() const { return std::chrono::duration<double, std::milli>(_total).count(); }

private:
    std::chrono::steady_clock::time_point _begin;
    std::chrono::steady_clock::duration _total{};
};

#ifdef EPIK_AMD_AA
constexpr const char* kSequenceType = "Proteins";
#else
constexpr const char* kSequenceType = "DNA";
#endif

/// main.cpp:22-32
std::string make_invocation(int argc, char** argv)
{
    std::string invocation;
    for (int i = 0; i < argc; ++i) invocation += std::string(argv[i]) + " ";
    return invocation;
}

/// main.cpp:34-37: <output_dir>/placements_<basename(query)>.jplace
std::string make_output_filename(const std::string& input_file, const std::string& output_dir)
{
    const auto slash = input_file.find_last_of('/');
    const std::string base = slash == std::string::npos ? input_file : input_file.substr(slash + 1);
    std::string dir = output_dir;
    if (!dir.empty() && dir.back() != '/') dir.push_back('/');
    return dir + "placements_" + base + ".jplace";
}

/// --strand reverse|both: <output_dir>/strands_<basename(query)>.tsv beside the jplace
std::string make_strands_filename(const std::string& input_file, const std::string& output_dir)
{
    const auto slash = input_file.find_last_of('/');
    const std::string base = slash == std::string::npos ? input_file : input_file.substr(slash + 1);
    std::string dir = output_dir;
    if (!dir.empty() && dir.back() != '/') dir.push_back('/');
    return dir + "strands_" + base + ".tsv";
}

/// --translate: <output_dir>/frames_<basename(query)>.tsv beside the jplace
std::string make_frames_filename(const std::string& input_file, const std::string& output_dir)
{
    const auto slash = input_file.find_last_of('/');
    const std::string base = slash == std::string::npos ? input_file : input_file.substr(slash + 1);
    std::string dir = output_dir;
    if (!dir.empty() && dir.back() != '/') dir.push_back('/');
    return dir + "frames_" + base + ".tsv";
}

/// What two mates are both called: the header up to the first white space, without a trailing /1 or /2
std::string_view mate_name(std::string_view header)
{
    size_t end = 0;
    while (end < header.size() && !std::isspace((unsigned char)header[end])) ++end;
    std::string_view name = header.substr(0, end);
    if (name.size() >= 2 && name[name.size() - 2] == '/' && (name.back() == '1' || name.back() == '2')) name.remove_suffix(2);
    return name;
}

}  // namespace
#endif  // EPIK_AMD_NO_MAIN

#ifndef EPIK_AMD_NO_MAIN

namespace {

const char* kHelp =
    "Evolutionary Placement with Informative K-mers (MI355X placer)\n"
    "Usage:\n"
    "  epik-dna|epik-aa [OPTION...]\n\n"
    "  -d, --database arg      IPK database\n"
    "  -q, --query arg         Input query file (.fasta)\n"
    "  -j, --jobs arg          Num threads (default: 1)\n"
    "      --batch-size arg    Batch size (default: 2000)\n"
    "      --omega arg         Determines the threshold value (default: 1.5)\n"
    "      --mu arg            Proportion of the database to load (default: 1.0)\n"
    "      --max-ram arg       Approximate database size to load, MB\n"
    "  -o, --output-dir arg    Output directory\n"
    "      --keep-at-most arg  Number of branches to report (default: 7)\n"
    "      --keep-factor arg   Minimum LWR to report (default: 0.01)\n"
    "      --gpus arg          Number of MI355X devices to use (default: 1)\n"
    "      --devices arg       Comma-separated HIP device ordinals (overrides --gpus)\n"
    "      --db-shard arg      Cut the database in so many shards by k-mer code, one per device\n"
    "                          (a database larger than one device; default: 1 = replicate it)\n"
    "      --strand arg        forward | reverse (reverse complement) | both (the better per read) (default: forward)\n"
    "      --translate arg     Nucleotide reads on this amino-acid database: forward (frames +1 +2 +3) | reverse\n"
    "                          (-1 -2 -3) | both (all six); the best frame per read (epik-aa; default: off)\n"
    "      --mates arg         Paired-end reads: the FASTA file of the second mates, records in the order of the query;\n"
    "                          every pair gets ONE placement, named by the query's records (epik-dna)\n"
    "      --mate-orientation arg  fr (mate 2 is the reverse complement of the fragment's far end) | ff (default: fr)\n"
    "      --profile           Also write profile_<query>.tsv: per branch the summed like-weight ratios and the reads\n"
    "                          placed best on it, with clade sums; reads without any hit are counted, not spread\n"
    "      --profile-only      Write that profile and no jplace: the rows are summed on the device(s) and never\n"
    "                          leave them (not with --db-shard > 1)\n"
    "      --assign            Also write assign_<query>.tsv -- per record the LCA clade that holds --assign-mass of its\n"
    "                          placement mass, that clade's size and mass, and the EDPL -- and assign_clades_<query>.tsv,\n"
    "                          the records assigned to each branch and clade; computed on the device(s) (not with\n"
    "                          --db-shard > 1; with --profile-only the rows still never leave the device)\n"
    "      --assign-mass arg   Share of a record's placement mass its clade must hold, in [0, 1] (default: 0.95)\n"
    "      --taxonomy arg      A taxonomy file, one leaf_label<TAB>A;B;C line per reference leaf.  Also write taxa_<query>.tsv --\n"
    "                          per taxon the records assigned to it and the mass placed in it, and the same over its clade --\n"
    "                          or, with --cohort, cohort_taxa_<list>.tsv, the sample x taxon table; summed on the device(s)\n"
    "                          (not with --assign or --db-shard > 1)\n"
    "      --taxonomy-mass arg Share of a record's placement mass its taxon must hold, in (0.5, 1] (default: 0.95)\n"
    "      --taxonomy-per-read Also write taxa_reads_<query>.tsv: per record its taxon, that taxon's share and its best row's taxon\n"
    "      --cohort            The query is a list of samples, one name<TAB>path line each (paths relative to the list; blank\n"
    "                          and # lines skipped).  Writes no jplace but cohort_samples_<list>.tsv (records per sample),\n"
    "                          cohort_profile_<list>.tsv (name, edge_num, best, mass_q of every non-zero cell) and\n"
    "                          cohort_kr_<list>.tsv (the Kantorovich-Rubinstein distance between every two samples), summed\n"
    "                          and computed on the device(s); with --strand / --translate, not with --mates, --profile,\n"
    "                          --profile-only, --assign or --db-shard > 1\n"
    "      --cohort-squash     With --cohort: also cluster the samples by squash clustering (Matsen & Evans 2013) on the\n"
    "                          device, every merged cluster the weighted average of its parts' masses, and write\n"
    "                          cohort_squash_<list>.tsv (a line per merge) and cohort_squash_<list>.nwk (the cluster tree)\n"
    "      --cohort-epca       With --cohort: also compute the edge principal components of the samples (Matsen & Evans 2013)\n"
    "                          on the device and write cohort_epca_<list>.tsv (the components and every sample's\n"
    "                          projections) and cohort_epca_edges_<list>.tsv (the components' coefficients per inner branch)\n"
    "      --cohort-epca-components arg  With --cohort-epca: the number of components, in [1, 64] (default: 5)\n"
    "      --cohort-pcoa       With --cohort: also compute the principal coordinates (Gower 1966) of the samples over their KR\n"
    "                          distances on the device and write cohort_pcoa_<list>.tsv (all eigenvalues, the negative ones of a\n"
    "                          distance that is not Euclidean included, and every sample's coordinates)\n"
    "      --cohort-pcoa-components arg  With --cohort-pcoa: the number of axes, in [1, 64] (default: 5)\n"
    "      --cohort-unifrac arg  With --cohort: also compute the UniFrac distances between every two samples on the device: arg is\n"
    "                          a comma-separated subset of unweighted (Lozupone & Knight 2005), weighted (normalised; Lozupone et al.\n"
    "                          2007) and generalized (alpha = 0.5; Chen et al. 2012), or all; writes cohort_unifrac_<metric>_<list>.tsv\n"
    "                          each.  The tree is rooted where the database's tree is: UniFrac depends on the rooting, KR does not\n"
    "      --cohort-distance arg  With --cohort-permanova, --cohort-pcoa or --cohort-permdisp: the distance they run over: kr\n"
    "                          (default), unweighted, weighted or generalized; with another than kr the first line of their files\n"
    "                          ends in <TAB>distance=arg\n"
    "      --cohort-kmeans arg With --cohort: also cluster the samples into at most arg clusters, in [1, 64], by phylogenetic\n"
    "                          k-means (Czech et al. 2019) on the device and write cohort_kmeans_<list>.tsv (the clusters and\n"
    "                          every sample's cluster and distance) and cohort_kmeans_centroids_<list>.tsv (the centroids' masses)\n"
    "      --cohort-kmeans-iterations arg  With --cohort-kmeans: the most iterations, in [1, 1000] (default: 100)\n"
    "      --cohort-alpha      With --cohort: also compute the alpha diversity of every sample (McCoy & Matsen 2013: PD, rooted PD,\n"
    "                          balance-weighted PD at 0.5 and 1, quadratic entropy) on the device and write cohort_alpha_<list>.tsv\n"
    "      --cohort-rarefy arg With --cohort: also compute every sample's rarefaction curve (Nipperess & Matsen 2013: the expected\n"
    "                          PD and rooted PD of k reads drawn without replacement) up to depth arg, in [1, 1048576], on the\n"
    "                          device and write cohort_rarefy_<list>.tsv\n"
    "      --cohort-rarefy-step arg  With --cohort-rarefy: the distance between two depths (default: max(1, ceil(depth / 64)));\n"
    "                          floor(depth / step) must lie in [1, 256]\n"
    "      --cohort-correlation arg  With --cohort: also correlate every branch's mass and imbalance with the per-sample metadata\n"
    "                          of the TSV file arg (Czech et al. 2019: Pearson and Spearman; header sample<TAB>name1<TAB>..., 1 to 64\n"
    "                          columns, empty or NA for a missing value) on the device and write cohort_correlation_<list>.tsv\n"
    "      --cohort-dispersion With --cohort: also compute how every branch's mass and imbalance vary across the samples (mean,\n"
    "                          variance, standard deviation, coefficient of variation, variance to mean) on the device and write\n"
    "                          cohort_dispersion_<list>.tsv\n"
    "      --cohort-permanova arg  With --cohort: also test, for every factor column of the TSV file arg (header\n"
    "                          sample<TAB>factor1<TAB>..., 1 to 64 columns of labels, empty or NA for a missing one), whether its\n"
    "                          groups of samples differ (PERMANOVA over the KR distances, Anderson 2001) on the device and write\n"
    "                          cohort_permanova_<list>.tsv\n"
    "      --cohort-permanova-permutations arg  With --cohort-permanova: the number of permutations in [1, 999999] (default: 999)\n"
    "      --cohort-permanova-seed arg  With --cohort-permanova: the seed of the permutations, a uint64 (default: 1)\n"
    "      --cohort-permanova-pairwise  With --cohort-permanova: also test every two groups of every column (at most 32 groups\n"
    "                          a column)\n"
    "      --cohort-permdisp arg  With --cohort: also test, for every factor column of the TSV file arg (as --cohort-permanova's,\n"
    "                          at most 32 labels a column), whether its groups differ in spread: PERMDISP (Anderson 2006), the\n"
    "                          distances to the group centroids over the KR distances, by permutation of residuals on the\n"
    "                          device; cohort_permdisp_<list>.tsv\n"
    "      --cohort-permdisp-permutations arg  With --cohort-permdisp: the number of permutations in [1, 999999] (default: 999)\n"
    "      --cohort-permdisp-seed arg  With --cohort-permdisp: the seed of the permutations, a uint64 (default: 1)\n"
    "      --cohort-permdisp-pairwise  With --cohort-permdisp: also test every two groups of every column\n"
    "      --cohort-mantel arg  With --cohort: also test, for every column of the metadata TSV file arg (as --cohort-correlation's),\n"
    "                          whether the distance between samples grows with the difference in the column: the Mantel test\n"
    "                          (Mantel 1967, one-sided) by permutation on the device; cohort_mantel_<list>.tsv\n"
    "      --cohort-mantel-matrix arg  With --cohort: NAME=FILE, a square TSV in the layout of cohort_kr_<list>.tsv as one more side\n"
    "                          of the Mantel test (a sample of the list that it lacks is missing on that side); up to 8 times\n"
    "      --cohort-mantel-method arg  With the Mantel test: pearson (default), spearman or both\n"
    "      --cohort-mantel-partial arg  With the Mantel test: the column or matrix NAME held fixed: the partial Mantel test (Smouse,\n"
    "                          Long & Sokal 1986) of every other side\n"
    "      --cohort-mantel-permutations arg  With the Mantel test: the number of permutations in [1, 999999] (default: 999)\n"
    "      --cohort-mantel-seed arg  With the Mantel test: the seed of the permutations, a uint64 (default: 1)\n"
    "      --cohort-anosim arg  With --cohort: also test, for every factor column of the TSV file arg (as --cohort-permanova's),\n"
    "                          whether the ranked distances between its groups exceed those within: ANOSIM (Clarke 1993) on the\n"
    "                          device; cohort_anosim_<list>.tsv\n"
    "      --cohort-anosim-permutations arg  With --cohort-anosim: the number of permutations in [1, 999999] (default: 999)\n"
    "      --cohort-anosim-seed arg  With --cohort-anosim: the seed of the permutations, a uint64 (default: 1)\n"
    "      --cohort-model arg     With --cohort: also fit, on the device, the sequential model adonis2(D ~ term1 + term2 + ...,\n"
    "                          by = \"terms\") over the columns of the TSV file arg (as --cohort-permanova's) that\n"
    "                          --cohort-model-terms names; cohort_model_<list>.tsv\n"
    "      --cohort-model-terms arg  With --cohort-model (required): the terms in test order, comma-separated f:NAME (a factor)\n"
    "                          or n:NAME (a numeric covariate); at most 16 terms and 64 design columns\n"
    "      --cohort-model-permutations arg  With --cohort-model: the number of permutations in [1, 999999] (default: 999)\n"
    "      --cohort-model-seed arg  With --cohort-model: the seed of the permutations, a uint64 (default: 1)\n"
    "      --cohort-edge-model arg  With --cohort: also fit, on the device, the sequential linear model of --cohort-edge-model-terms to\n"
    "                          every branch's mass share and imbalance, by permutation, with the max-statistic adjustment over the\n"
    "                          branches; arg is a TSV file as --cohort-model's; cohort_edgemodel_<list>.tsv\n"
    "      --cohort-edge-model-terms arg  With --cohort-edge-model (required): the terms in test order, as --cohort-model-terms\n"
    "      --cohort-edge-model-permutations arg  With --cohort-edge-model: the number of permutations in [1, 999999] (default: 999)\n"
    "      --cohort-edge-model-seed arg  With --cohort-edge-model: the seed of the permutations, a uint64 (default: 1)\n"
    "      --cohort-edge-test arg  With --cohort: also test, for every factor column of the TSV file arg (as --cohort-permanova's,\n"
    "                          at most 32 labels a column), on which branches its groups of samples differ: the one-way ANOVA and\n"
    "                          Kruskal-Wallis of every branch's mass and imbalance by permutation, with the max-statistic\n"
    "                          adjustment (Westfall & Young 1993), on the device; writes cohort_edgetest_<list>.tsv\n"
    "      --cohort-edge-test-permutations arg  With --cohort-edge-test: the number of permutations in [1, 999999] (default: 999)\n"
    "      --cohort-edge-test-seed arg  With --cohort-edge-test: the seed of the permutations, a uint64 (default: 1)\n"
    "      --cohort-strata arg  With --cohort-permanova, --cohort-permdisp, --cohort-edge-test or --cohort-model: permute within\n"
    "                          strata only (a subject sampled several times, a batch): a column of the TSV file arg (as\n"
    "                          --cohort-permanova's; any number of labels) gives every sample of the list its stratum; all of\n"
    "                          those tests of the run use it, and their files' first line ends in <TAB>strata=NAME\n"
    "      --cohort-strata-column arg  With --cohort-strata: the column of its file; required when the file has several\n"
    "      --windows arg       Paint long sequences by windows of arg characters: every window is placed by itself and called\n"
    "                          for the group of --window-groups that holds --window-mass of its placement mass.  Writes no\n"
    "                          jplace but windows_<query>.tsv (per record its segments: runs of windows with one call) and\n"
    "                          windows_breakpoints_<query>.tsv (where the call changes from one group to another); with\n"
    "                          --strand both every window picks its own strand; not with --mates, --translate, --profile,\n"
    "                          --profile-only, --assign, --taxonomy, --cohort or --db-shard > 1\n"
    "      --window-step arg   With --windows: the distance between two windows, in [1, window] (default: max(1, window / 4))\n"
    "      --window-mass arg   With --windows: the share of a window's placement mass its group must hold, in (0.5, 1]\n"
    "                          (default: 0.8)\n"
    "      --window-groups arg With --windows (required): a taxonomy file, one leaf_label<TAB>A;B;C line per reference leaf\n"
    "      --window-rank arg   With --windows: the groups are the taxa of so many elements of the taxopath (default: 1)\n"
    "      --windows-per-window  With --windows: also write windows_all_<query>.tsv, a line per window\n"
    "  -h, --help              Print usage\n";

using epik_amd::options;

options parse_args(int argc, char** argv)
{
    const std::map<std::string, std::string> short_names{
        {"-d", "database"}, {"-q", "query"}, {"-j", "jobs"}, {"-o", "output-dir"}, {"-h", "help"}};
    options opt;
    for (int i = 1; i < argc; ++i) {
        std::string arg = argv[i];
        std::string name, value;
        bool have_value = false;
        if (arg.rfind("--", 0) == 0) {
            name = arg.substr(2);
            const auto eq = name.find('=');
            if (eq != std::string::npos) {
                value = name.substr(eq + 1);
                name = name.substr(0, eq);
                have_value = true;
            }
        } else if (short_names.count(arg)) {
            name = short_names.at(arg);
        } else {
            continue;  // positional arguments are ignored (epik.py passes the query twice, epik.py:88,96)
        }
        if (name == "help" || ((name == "profile" || name == "profile-only" || name == "assign" || name == "cohort" || name == "cohort-squash" || name == "cohort-epca" || name == "cohort-pcoa" || name == "cohort-alpha" || name == "cohort-dispersion" || name == "cohort-permanova-pairwise" || name == "cohort-permdisp-pairwise" || name == "taxonomy-per-read" || name == "windows-per-window") && !have_value)) {  // flags
            opt.values[name] = "1";
            continue;
        }
        if (!have_value) {
            if (i + 1 >= argc) throw std::runtime_error("Option '" + name + "' is missing an argument");
            value = argv[++i];
        }
        if (name == "cohort-mantel-matrix") opt.matrices.push_back(value);  // (may be repeated: every argument, in order)
        opt.values[name] = value;
    }
    return opt;
}

/// The lines of a per-record file went into `filename`.part, because the header counts the records and only the end of the
/// input tells how many: the file proper is the header and then the part, which goes
void finish_part_file(std::ofstream& part_out, const std::string& filename, const std::string& header, uint64_t records)
{
    part_out.close();
    if (!part_out) throw std::runtime_error("Could not write " + filename + ".part");
    {
        std::ifstream part(filename + ".part", std::ios::binary);
        std::ofstream whole(filename, std::ios::binary);
        whole << header;
        if (records) whole << part.rdbuf();
        whole.close();
        if (!part || !whole) throw std::runtime_error("Could not write " + filename);
    }
    std::remove((filename + ".part").c_str());
}

}  // namespace

int main(int argc, char** argv)
{
    std::ios::sync_with_stdio(false);
    if (argc == 1) {
        std::cout << kHelp << std::endl;
        return 0;
    }
    try {
        const options parsed = parse_args(argc, argv);
        if (parsed.has("help")) {
            std::cout << kHelp << std::endl;
            return 0;
        }
        // --strand: checked before anything is opened or any device touched
        const auto strand_name = parsed.get("strand", "forward");
        epik_amd::strand_mode strand = epik_amd::strand_mode::forward;
        if (strand_name == "reverse")
            strand = epik_amd::strand_mode::reverse;
        else if (strand_name == "both")
            strand = epik_amd::strand_mode::both;
        else if (strand_name != "forward")
            throw std::runtime_error("--strand must be forward, reverse or both, not '" + strand_name + "'");
        if (strand != epik_amd::strand_mode::forward) {
#ifdef EPIK_AMD_AA
            throw std::runtime_error("--strand " + strand_name + " places nucleotide reads only (epik-dna)");
#endif
            if (std::stoul(parsed.get("db-shard", "1")) > 1)
                throw std::runtime_error("--strand " + strand_name + " does not work with --db-shard > 1");
        }
        // --mates: checked before anything is opened or any device touched
        const bool with_mates = parsed.has("mates");
        const auto orientation_name = parsed.get("mate-orientation", "fr");
        if (orientation_name != "fr" && orientation_name != "ff")
            throw std::runtime_error("--mate-orientation must be fr or ff, not '" + orientation_name + "'");
        if (parsed.has("mate-orientation") && !with_mates) throw std::runtime_error("--mate-orientation needs --mates");
        if (with_mates) {
#ifdef EPIK_AMD_AA
            throw std::runtime_error("--mates places pairs of nucleotide reads only (epik-dna)");
#endif
            if (parsed.has("translate")) throw std::runtime_error("--mates does not work with --translate");
            if (std::stoul(parsed.get("db-shard", "1")) > 1) throw std::runtime_error("--mates does not work with --db-shard > 1");
        }
        // --translate: checked before anything is opened or any device touched
        const bool translate = parsed.has("translate");
        epik_amd::translate_mode frames = epik_amd::translate_mode::both;
        if (translate) {
            const auto name = parsed.get("translate", "");
            if (name == "forward")
                frames = epik_amd::translate_mode::forward;
            else if (name == "reverse")
                frames = epik_amd::translate_mode::reverse;
            else if (name != "both")
                throw std::runtime_error("--translate must be forward, reverse or both, not '" + name + "'");
#ifndef EPIK_AMD_AA
            throw std::runtime_error("--translate " + name + " places nucleotide reads on amino-acid databases only (epik-aa)");
#endif
            if (std::stoul(parsed.get("db-shard", "1")) > 1)
                throw std::runtime_error("--translate " + name + " does not work with --db-shard > 1");
        }
        // --profile / --profile-only: checked before anything is opened or any device touched
        const bool profile_only = parsed.has("profile-only"), with_profile = parsed.has("profile") || profile_only;
        if (profile_only && std::stoul(parsed.get("db-shard", "1")) > 1)
            throw std::runtime_error("--profile-only does not work with --db-shard > 1 (use --profile: the rows of a sharded "
                                     "placement are finished on several devices)");
        // --assign / --assign-mass: checked before anything is opened or any device touched
        const bool with_assign = parsed.has("assign");
        if (parsed.has("assign-mass") && !with_assign) throw std::runtime_error("--assign-mass needs --assign");
        if (with_assign && std::stoul(parsed.get("db-shard", "1")) > 1)
            throw std::runtime_error("--assign does not work with --db-shard > 1 (the rows of a sharded placement are finished "
                                     "on several devices)");
        uint32_t assign_tau_q = 0;
        if (with_assign) {
            size_t used = 0;
            const auto text = parsed.get("assign-mass", "0.95");
            double tau = -1.0;
            try {
                tau = std::stod(text, &used);
            } catch (const std::exception&) {
                used = 0;
            }
            if (used != text.size() || used == 0) throw std::runtime_error("--assign-mass must be a number in [0, 1], not '" + text + "'");
            assign_tau_q = epik_amd::assign_tau_q(tau);
        }
        // --cohort and its analyses: checked before anything is opened or any device touched
        epik_amd::cohort_plan cohort_plan = epik_amd::parse_cohort_options(parsed);
        const bool with_cohort = cohort_plan.with_cohort;
        // --taxonomy / --taxonomy-mass / --taxonomy-per-read: checked before anything is opened or any device touched
        const bool with_taxonomy = parsed.has("taxonomy"), taxonomy_per_read = parsed.has("taxonomy-per-read");
        if (parsed.has("taxonomy-mass") && !with_taxonomy) throw std::runtime_error("--taxonomy-mass needs --taxonomy");
        if (taxonomy_per_read && !with_taxonomy) throw std::runtime_error("--taxonomy-per-read needs --taxonomy");
        uint32_t taxonomy_tau_q = 0;
        if (with_taxonomy) {
            if (with_assign) throw std::runtime_error("--taxonomy does not work with --assign (both in one pass is not built)");
            if (std::stoul(parsed.get("db-shard", "1")) > 1)
                throw std::runtime_error("--taxonomy does not work with --db-shard > 1 (the rows of a sharded placement are finished "
                                         "on several devices)");
            size_t used = 0;
            const auto text = parsed.get("taxonomy-mass", "0.95");
            double share = -1.0;
            try {
                share = std::stod(text, &used);
            } catch (const std::exception&) {
                used = 0;
            }
            if (used != text.size() || used == 0 || !(share > 0.5) || !(share <= 1.0))
                throw std::runtime_error("--taxonomy-mass must be a number in (0.5, 1], not '" + text + "'");
            taxonomy_tau_q = epik_amd::assign_tau_q(share);
            if (taxonomy_tau_q <= (1u << 29) || taxonomy_tau_q > (1u << 30))
                throw std::runtime_error("--taxonomy-mass must be a number in (0.5, 1], not '" + text + "'");
        }
        // --windows and the flags that depend on it: checked before anything is opened or any device touched
        epik_amd::windows_plan windows_plan = epik_amd::parse_windows_options(parsed);
        const auto db_file = parsed.require("database");
        const auto query_file = parsed.require("query");
        const auto num_threads = (size_t)std::stoul(parsed.get("jobs", "1"));
        const auto batch_size = (size_t)std::stoul(parsed.get("batch-size", "2000"));
        const auto user_omega = std::stof(parsed.get("omega", "1.5"));
        const auto user_mu = std::stof(parsed.get("mu", "1.0"));
        const auto keep_at_most = (size_t)std::stoul(parsed.get("keep-at-most", "7"));
        const auto keep_factor = std::stod(parsed.get("keep-factor", "0.01"));
        const auto output_dir = parsed.require("output-dir");
        epik_amd::check_mu(user_mu);
        // --cohort: the list of samples and the analyses' side files, every file looked at before the database or a device is
        cohort_plan.read_inputs(query_file);
        const std::vector<epik_amd::cohort_sample>& cohort_samples = cohort_plan.samples;

        windows_plan.read_inputs();  // (--window-groups: the same reader, the same errors)
        // --taxonomy: the file read, and every error of it named by its line, before the database or a device is
        epik_amd::taxonomy taxa;
        if (with_taxonomy) {
            std::ifstream in(parsed.require("taxonomy"), std::ios::binary);
            if (!in) throw std::runtime_error("Could not open the taxonomy file " + parsed.require("taxonomy"));
            std::string err;
            if (epik_amd::parse_taxonomy(in, taxa, err) != 0) throw std::runtime_error(parsed.require("taxonomy") + ": " + err);
        }

        size_t max_entries = std::numeric_limits<size_t>::max();
        if (parsed.has("max-ram")) {
            const auto max_ram = epik_amd::parse_memory_size(parsed.require("max-ram"));
            max_entries = static_cast<size_t>(max_ram / sizeof(epik_amd::pkdb_value));
            if (max_entries == 0) throw std::runtime_error("Memory limit is too low");
            std::cout << "Max-RAM provided: will be loaded not more than " << epik_amd::human_count(max_entries)
                      << " phylo-k-mers." << std::endl;
        }

        const auto db_shards = (uint32_t)std::stoul(parsed.get("db-shard", "1"));
        if (db_shards == 0 || db_shards > EPIK_AMD_MAX_SHARDS)
            throw std::runtime_error("--db-shard must be between 1 and " + std::to_string(EPIK_AMD_MAX_SHARDS));
        std::vector<int> devices;
        if (parsed.has("devices")) {
            std::stringstream ss(parsed.require("devices"));
            for (std::string item; std::getline(ss, item, ',');) devices.push_back(std::stoi(item));
        } else {
            // (sharded: a device per shard while there are devices; --gpus / --devices say otherwise)
            const int n = parsed.has("gpus") || db_shards == 1 ? std::stoi(parsed.get("gpus", "1"))
                                                                : std::min<int>((int)db_shards, std::max(1, epik_amd_device_count()));
            for (int i = 0; i < n; ++i) devices.push_back(i);
        }
        for (int device : devices)
            if (device < 0 || device >= epik_amd_device_count())
                throw std::runtime_error("HIP device " + std::to_string(device) + " is not available: " +
                                         std::to_string(epik_amd_device_count()) +
                                         " visible (this placer has no CPU fallback)");

        std::cout << "Loading database with mu=" << user_mu << " and omega=" << user_omega << "..." << std::endl;
        // --db-shard G: this is shard 0 of G; the placer's constructor loads the others one after the other and
        // drops each as soon as its lists are on its device (--max-ram then bounds what ONE shard keeps)
        auto db = epik_amd::load(db_file, user_mu, user_omega, max_entries, 0, db_shards);
        if (db.version() < epik_amd::protocol::EARLIEST_INDEX) {
            std::cerr << "The serialization protocol version is too old (v" << db.version() << ").\n";
            return -1;
        }
        if (db.sequence_type() != kSequenceType)
            throw std::runtime_error(std::string("This binary places ") + kSequenceType + " databases, the file holds " +
                                     db.sequence_type());

        std::cout << "Database parameters:" << std::endl
                  << "\tSequence type: " << db.sequence_type() << std::endl
                  << "\tk: " << db.kmer_size() << std::endl
                  << "\tomega: " << db.omega() << std::endl
                  << "\tPositions loaded: " << (db.positions_loaded() ? "true" : "false") << std::endl
                  << std::endl;
        std::cout << "Loaded " << epik_amd::human_count(db.get_num_entries_loaded()) << " of "
                  << epik_amd::human_count(db.get_num_entries_total()) << " phylo-k-mers"
                  << (db_shards > 1 ? " (shard 0 of " + std::to_string(db_shards) + ")" : std::string()) << ". " << std::endl
                  << std::endl;

        const auto tree = epik_amd::io::parse_newick(db.tree());
        const epik_amd::placer::shard_loader load_shard = [&](uint32_t g) {
            auto part = epik_amd::load(db_file, user_mu, user_omega, max_entries, g, db_shards);
            std::cout << "Loaded " << epik_amd::human_count(part.get_num_entries_loaded()) << " phylo-k-mers (shard " << g
                      << " of " << db_shards << ")." << std::endl;
            return part;
        };
        epik_amd::placer placer(db, tree, keep_at_most, keep_factor, num_threads, devices, db_shards, load_shard);
        placer.set_strand(strand);
        if (translate) placer.set_translate(frames);
        if (with_mates) placer.set_mates(orientation_name == "ff" ? epik_amd::mate_orientation::ff : epik_amd::mate_orientation::fr);
        if (profile_only) placer.set_profile_only();
        if (with_cohort) placer.set_cohort((uint32_t)cohort_samples.size());
        // --assign: the rule's tree on every device; the host's copy names clade sizes and sums the clades
        std::unique_ptr<epik_amd::confidence_tree> assign_tree;
        if (with_assign) {
            assign_tree.reset(new epik_amd::confidence_tree(tree));
            placer.set_assign(assign_tau_q);
        }
        // --taxonomy: the branches labelled from the tree's leaves, one object per device (a row of cells per sample)
        if (with_taxonomy) {
            std::vector<uint32_t> parent, label;
            std::vector<std::string> names;
            for (const auto& node : tree.nodes()) {
                parent.push_back(node.parent < 0 ? EPIK_AMD_TREE_NO_PARENT : (uint32_t)node.parent);
                names.push_back(node.get_label());
            }
            std::string err;
            if (epik_amd::label_branches(taxa, parent.data(), names, (uint32_t)parent.size(), label, err) != 0)
                throw std::runtime_error(parsed.require("taxonomy") + ": " + err);
            placer.set_taxonomy(taxa.parent, label, taxonomy_tau_q, taxonomy_per_read);
        }
        db.drop_lists();  // the lists are on the devices now; tree, k and omega stay for the output
        // --windows: a run of its own, no jplace
        if (windows_plan.with_windows) {
            std::vector<uint32_t> parent;
            std::vector<std::string> names;
            for (const auto& node : tree.nodes()) {
                parent.push_back(node.parent < 0 ? EPIK_AMD_TREE_NO_PARENT : (uint32_t)node.parent);
                names.push_back(node.get_label());
            }
            windows_plan.label(parent.data(), names, (uint32_t)parent.size());
            std::cout << "Instruction set: gfx950 (" << placer.handle_count() << " device(s))" << std::endl;
            std::cout << "Painting " << query_file << " by windows of " << windows_plan.window << " every " << windows_plan.step << " ("
                      << windows_plan.group_paths.size() << " groups)..." << std::endl;
            const auto begin = std::chrono::steady_clock::now();
            const auto report = epik_amd::run_windows(placer, windows_plan, (uint32_t)strand, query_file, output_dir, batch_size, num_threads);
            const auto ms = (size_t)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - begin).count();
            std::cout << std::endl
                      << "Painted " << report.records << " sequences: " << report.windows << " windows, " << report.segments
                      << " segments, " << report.breakpoints << " breakpoints.\nWindows: " << report.windows_file
                      << "\nBreakpoints: " << report.breakpoints_file << std::endl;
            if (windows_plan.per_window) std::cout << "Windows, one by one: " << report.all_file << std::endl;
            std::cout << "Placement time: " << epik_amd::human_duration(ms) << " (" << ms << " ms)" << std::endl;
            std::cout << "Done." << '\n' << std::flush;
            return 0;
        }
        const auto tree_as_newick = epik_amd::io::to_newick(tree, true);
        const auto jplace_filename = make_output_filename(query_file, output_dir);
        const auto invocation = make_invocation(argc, argv);

        // --profile-only: no jplace at all
        std::unique_ptr<epik_amd::io::jplace_writer> jplace;
        if (!profile_only && !with_cohort) {
            jplace.reset(new epik_amd::io::jplace_writer(jplace_filename, invocation, tree_as_newick));
            jplace->set_branch_lengths(placer.distal_lengths(), placer.pendant_lengths());
            jplace->start();
        }
        // --profile: summed by the writer thread from the rows it writes; --profile-only: read from the devices at the end
        epik_amd::sample_profile profile(with_profile ? tree.get_node_count() : 0);
        const auto profile_filename = epik_amd::make_profile_filename(query_file, output_dir);
        // --strand reverse|both: one "name<TAB>+|-" line per input record, input order
        std::ofstream strands_out;
        if (strand != epik_amd::strand_mode::forward && !with_cohort) {
            strands_out.open(make_strands_filename(query_file, output_dir));
            if (!strands_out) throw std::runtime_error("Could not open " + make_strands_filename(query_file, output_dir));
        }
        // --assign: one line per input record, input order, into a part file: the header line counts the records, which
        // only the end of the input tells; the file proper is the header and then the part
        std::ofstream assign_out;
        const auto assign_filename = epik_amd::make_assign_filename(query_file, output_dir);
        const auto assign_clades_filename = epik_amd::make_assign_clades_filename(query_file, output_dir);
        epik_amd::assign_summary assign_sums(with_assign ? tree.get_node_count() : 0);
        uint64_t assign_records = 0;
        if (with_assign) {
            assign_out.open(assign_filename + ".part", std::ios::binary);
            if (!assign_out) throw std::runtime_error("Could not open " + assign_filename + ".part");
        }
        // --taxonomy-per-read: as the assign file, through a part file
        std::ofstream taxa_reads_out;
        const auto in_dir = [&](const std::string& prefix) {
            const auto slash = query_file.find_last_of('/');
            std::string dir = output_dir;
            if (!dir.empty() && dir.back() != '/') dir.push_back('/');
            return dir + prefix + (slash == std::string::npos ? query_file : query_file.substr(slash + 1)) + ".tsv";
        };
        const auto taxa_filename = with_cohort ? epik_amd::make_cohort_filename("taxa", query_file, output_dir) : in_dir("taxa_");
        const auto taxa_reads_filename = in_dir("taxa_reads_");
        uint64_t taxa_reads_records = 0;
        if (taxonomy_per_read) {
            taxa_reads_out.open(taxa_reads_filename + ".part", std::ios::binary);
            if (!taxa_reads_out) throw std::runtime_error("Could not open " + taxa_reads_filename + ".part");
        }
        // --translate: one "name<TAB>+1..-3" line per input record, input order
        std::ofstream frames_out;
        if (translate && !with_cohort) {
            frames_out.open(make_frames_filename(query_file, output_dir));
            if (!frames_out) throw std::runtime_error("Could not open " + make_frames_filename(query_file, output_dir));
        }

        std::cout << "Instruction set: gfx950 (" << placer.handle_count()
                  << (db_shards > 1 ? " shard(s) of the database, one handle each)" : " device(s))") << std::endl;
        std::cout << "Placing " << query_file << (with_cohort ? " (" + std::to_string(cohort_samples.size()) + " samples)" : std::string())
                  << "..." << std::endl;
        const auto begin = std::chrono::steady_clock::now();
        size_t num_seq_placed = 0;
        double average_speed = 0.0;
        size_t num_iterations = 0;

        // Stages on their own threads, batches handed on through queues: the FASTA reader; one placer
        // thread per device; the jplace writer (formatting on `--jobs` threads).  The reference runs
        // read, place and write one after the other per batch (main.cpp:336-361); batch boundaries,
        // dedup per batch (place.cpp:207) and output order are the same here.  A placer thread takes
        // every batch that is waiting (up to kGroupBatches) as ONE launch -- a 2000-read batch is far too
        // small to fill a device -- so with several devices whole groups of batches go to them in turn,
        // and the writer puts the batches back in input order.
        constexpr size_t kGroupBatches = 64;
        struct work_item {
            size_t sequence = 0;                          // position of the batch in the input
            uint32_t sample = 0;                          // --cohort: the sample the batch belongs to
            std::shared_ptr<epik_amd::io::batch_fasta> file;  // ... and its file, mapped while a batch of it is on its way
            std::vector<epik_amd::seq_record> batch;     // owns the bytes the views below point into
            std::vector<epik_amd::seq_record> mates;     // --mates: the second mate of every record of the batch
            epik_amd::impl::placed_batch placed;
        };
        const size_t n_devices = placer.device_count();
        bounded_queue<work_item> to_place(2 * kGroupBatches * n_devices);
        bounded_queue<work_item> to_write(2 * kGroupBatches * n_devices);
        std::exception_ptr reader_error, writer_error;
        std::vector<std::exception_ptr> placer_errors(n_devices);
        stage_clock read_clock, write_clock;
        std::vector<stage_clock> place_clocks(n_devices);
        std::mutex stats_mutex;
        // (the records of a batch are views into the reader's mapping of the file: it stays until all is written)
        // (--cohort: the query is the list; every sample's file is opened when its turn comes)
        std::unique_ptr<epik_amd::io::batch_fasta> reader;
        if (!with_cohort) reader.reset(new epik_amd::io::batch_fasta(query_file, batch_size));
        // --mates: read in step with the query, record for record
        std::unique_ptr<epik_amd::io::batch_fasta> mates_reader;
        if (with_mates) mates_reader.reset(new epik_amd::io::batch_fasta(parsed.require("mates"), batch_size));
        std::thread reader_thread([&] {
            try {
                if (with_cohort) {
                    // the samples in list order, every file in batches of its own: a batch never holds two samples, so
                    // de-duplication stays per sample and a launch still takes the batches of many small samples
                    size_t sequence = 0;
                    bool open = true;
                    for (uint32_t s = 0; s < cohort_samples.size() && open; ++s) {
                        read_clock.start();
                        auto file = std::make_shared<epik_amd::io::batch_fasta>(cohort_samples[s].path, batch_size);
                        read_clock.stop();
                        for (;;) {
                            read_clock.start();
                            auto batch = file->next_batch();
                            read_clock.stop();
                            if (batch.empty()) break;
                            work_item item;
                            item.sequence = sequence++, item.sample = s, item.file = file, item.batch = std::move(batch);
                            if (!(open = to_place.push(std::move(item)))) break;
                        }
                    }
                    to_place.close();
                    return;
                }
                size_t records = 0;
                for (size_t sequence = 0;; ++sequence) {
                    read_clock.start();
                    auto batch = reader->next_batch();
                    std::vector<epik_amd::seq_record> mates;
                    if (mates_reader) {
                        mates = mates_reader->next_batch();
                        const size_t both = std::min(batch.size(), mates.size());
                        for (size_t i = 0; i < both; ++i)
                            if (mate_name(batch[i].header()) != mate_name(mates[i].header()))
                                throw std::runtime_error("--mates: record " + std::to_string(records + i + 1) + " of the mates is '" +
                                                         std::string(mate_name(mates[i].header())) + "', of the query '" +
                                                         std::string(mate_name(batch[i].header())) +
                                                         "': the mates must come in the order of the query");
                        if (batch.size() != mates.size()) {
                            const auto& longer = batch.size() > both ? batch : mates;
                            throw std::runtime_error(std::string("--mates: the ") + (batch.size() > both ? "mates" : "query") +
                                                     " end after " + std::to_string(records + both) + " records: no mate for record " +
                                                     std::to_string(records + both + 1) + " ('" +
                                                     std::string(mate_name(longer[both].header())) + "')");
                        }
                        records += both;
                    }
                    read_clock.stop();
                    if (batch.empty()) break;
                    work_item item;
                    item.sequence = sequence, item.batch = std::move(batch), item.mates = std::move(mates);
                    if (!to_place.push(std::move(item))) break;
                }
            } catch (...) {
                reader_error = std::current_exception();
            }
            to_place.close();  // the placer threads drain what is queued, then stop
        });
        std::thread writer_thread([&] {
            try {
                std::map<size_t, work_item> waiting;  // batches that arrived ahead of their turn
                size_t next = 0;
                std::vector<work_item> arrived;
                while (to_write.pop_all(arrived)) {
                    for (auto& item : arrived) waiting.emplace(item.sequence, std::move(item));
                    std::vector<const epik_amd::impl::placed_batch*> group;
                    std::vector<work_item> ready;  // keeps the batches alive while they are written
                    for (auto it = waiting.find(next); it != waiting.end(); it = waiting.find(next)) {
                        ready.push_back(std::move(it->second));
                        waiting.erase(it);
                        ++next;
                    }
                    for (const auto& item : ready) group.push_back(&item.placed);
                    if (group.empty()) continue;
                    write_clock.start();
                    if (jplace) jplace->write(group, num_threads);
                    if (with_profile && !profile_only)
                        for (const auto* placed : group) profile.add(*placed);
                    if (strands_out.is_open()) {
                        for (const auto& item : ready)
                            for (size_t i = 0; i < item.batch.size(); ++i)
                                strands_out << item.batch[i].header() << '\t'
                                            << (item.placed.strands[item.placed.unique_of[i]] ? '-' : '+') << '\n';
                        if (!strands_out) throw std::runtime_error("Could not write the strands file");
                    }
                    if (assign_out.is_open()) {
                        for (const auto& item : ready) {
                            std::string lines;
                            for (size_t i = 0; i < item.batch.size(); ++i) {
                                const auto& record = item.placed.confidence[item.placed.unique_of[i]];
                                lines += epik_amd::format_assign_line(item.batch[i].header(), record, *assign_tree);
                                assign_sums.add(record, 1);
                            }
                            assign_out << lines;
                            assign_records += item.batch.size();
                        }
                        if (!assign_out) throw std::runtime_error("Could not write the assign file");
                    }
                    if (taxa_reads_out.is_open()) {
                        for (const auto& item : ready) {
                            std::string lines;
                            for (size_t i = 0; i < item.batch.size(); ++i)
                                lines += epik_amd::format_taxa_reads_line(std::string(item.batch[i].header()),
                                                                          item.placed.taxa_records[item.placed.unique_of[i]], taxa);
                            taxa_reads_out << lines;
                            taxa_reads_records += item.batch.size();
                        }
                        if (!taxa_reads_out) throw std::runtime_error("Could not write the taxa reads file");
                    }
                    if (frames_out.is_open()) {
                        static const char* const names[6] = {"+1", "+2", "+3", "-1", "-2", "-3"};
                        for (const auto& item : ready)
                            for (size_t i = 0; i < item.batch.size(); ++i)
                                frames_out << item.batch[i].header() << '\t'
                                           << names[item.placed.frames[item.placed.unique_of[i]] % 6] << '\n';
                        if (!frames_out) throw std::runtime_error("Could not write the frames file");
                    }
                    write_clock.stop();
                }
            } catch (...) {
                writer_error = std::current_exception();
                to_write.close();
                to_place.close();
            }
        });
        std::vector<std::thread> placer_threads;
        for (size_t device = 0; device < n_devices; ++device) {
            placer_threads.emplace_back([&, device] {
                try {
                    std::vector<work_item> group;
                    while (to_place.pop_up_to(group, kGroupBatches)) {
                        const auto begin_group = std::chrono::steady_clock::now();
                        place_clocks[device].start();
                        std::vector<const std::vector<epik_amd::seq_record>*> batches;
                        std::vector<const std::vector<epik_amd::seq_record>*> mate_batches;
                        std::vector<uint32_t> batch_samples;
                        for (const auto& item : group)
                            batches.push_back(&item.batch), mate_batches.push_back(&item.mates), batch_samples.push_back(item.sample);
                        auto placed = placer.place_flat(batches, device, num_threads, with_mates ? &mate_batches : nullptr,
                                                        with_cohort ? &batch_samples : nullptr);
                        place_clocks[device].stop();
                        auto ms_diff = (float)std::chrono::duration_cast<std::chrono::microseconds>(
                                           std::chrono::steady_clock::now() - begin_group).count() / 1000.0f;
                        if (ms_diff <= 0) ms_diff = 0.001f;
                        {
                            std::lock_guard<std::mutex> lock(stats_mutex);
                            for (const auto& item : group) num_seq_placed += item.batch.size();
                            // main.cpp:351-352: nominal batch size over the batch's time; a batch of a group
                            // takes its share of the group's time
                            average_speed += (double)group.size() * 1000.0 * (double)batch_size /
                                             ((double)ms_diff / (double)group.size());
                            num_iterations += group.size();
                        }
                        bool open = true;
                        for (size_t i = 0; i < group.size() && open; ++i) {
                            group[i].placed = std::move(placed[i]);
                            open = to_write.push(std::move(group[i]));
                        }
                        if (!open) break;
                    }
                } catch (...) {
                    placer_errors[device] = std::current_exception();
                    to_place.close();
                }
            });
        }
        for (auto& t : placer_threads) t.join();
        to_place.close();
        to_write.close();
        reader_thread.join();
        writer_thread.join();
        for (const auto& error : placer_errors)
            if (error) std::rethrow_exception(error);
        for (const auto& error : {reader_error, writer_error})
            if (error) std::rethrow_exception(error);
        double place_ms = 0;
        for (const auto& clock : place_clocks) place_ms += clock.ms();
        if (std::getenv("EPIK_AMD_STAGE_TIMES"))
            std::cout << "stage read " << read_clock.ms() << " ms\nstage place " << place_ms
                      << " ms\nstage write " << write_clock.ms() << " ms" << std::endl;
        if (jplace) jplace->end();
        if (profile_only) placer.read_profiles(profile.mass.data(), profile.best.data(), profile.totals);
        if (with_profile) {
            std::vector<size_t> subtree_num_nodes;
            for (const auto& entry : db.tree_index()) subtree_num_nodes.push_back(entry.subtree_num_nodes);
            epik_amd::write_profile_tsv(profile_filename, profile, subtree_num_nodes);
        }
        cohort_plan.run_and_write(placer, query_file, output_dir);
        if (with_assign) {
            finish_part_file(assign_out, assign_filename, epik_amd::format_assign_header(assign_tau_q, assign_records), assign_records);
            epik_amd::write_text_file(assign_clades_filename, epik_amd::format_assign_clades_tsv(assign_sums, *assign_tree, assign_tau_q));
        }
        if (with_taxonomy) {
            // the devices' objects summed on the first, read once; the clade columns are prefix sums taken here
            const uint32_t rows_of_cells = with_cohort ? (uint32_t)cohort_samples.size() : 1;
            epik_amd::taxa_cells cells(rows_of_cells, taxa.num_taxa());
            placer.read_taxonomy(cells.direct.data(), cells.assigned.data(), cells.totals.data());
            if (with_cohort) {
                std::vector<std::string> names;
                for (const auto& sample : cohort_samples) names.push_back(sample.name);
                epik_amd::write_through_part(taxa_filename, epik_amd::format_cohort_taxa_tsv(names, cells, taxa, taxonomy_tau_q));
            } else {
                epik_amd::write_through_part(taxa_filename, epik_amd::format_taxa_tsv(cells, 0, taxa, taxonomy_tau_q));
            }
            if (taxonomy_per_read)
                finish_part_file(taxa_reads_out, taxa_reads_filename, epik_amd::format_taxa_reads_header(taxonomy_tau_q, taxa_reads_records),
                                 taxa_reads_records);
        }
        if (num_iterations) average_speed /= (double)num_iterations;
        std::cout << std::endl
                  << "Placed " << num_seq_placed << " sequences.\nAverage speed: " << epik_amd::human_count(average_speed, false)
                  << " seq/s.\n";
        if (jplace) std::cout << "Output: " << jplace_filename << std::endl;
        if (with_profile) std::cout << "Profile: " << profile_filename << std::endl;
        cohort_plan.print_summary();
        if (with_taxonomy) std::cout << "Taxa: " << taxa_filename << std::endl;
        if (taxonomy_per_read) std::cout << "Taxa of the reads: " << taxa_reads_filename << std::endl;
        if (with_assign) std::cout << "Assignments: " << assign_filename << "\nAssigned clades: " << assign_clades_filename << std::endl;
        if (strands_out.is_open()) {
            strands_out.close();
            if (!strands_out) throw std::runtime_error("Could not write " + make_strands_filename(query_file, output_dir));
            std::cout << "Strands: " << make_strands_filename(query_file, output_dir) << std::endl;
        }
        if (frames_out.is_open()) {
            frames_out.close();
            if (!frames_out) throw std::runtime_error("Could not write " + make_frames_filename(query_file, output_dir));
            std::cout << "Frames: " << make_frames_filename(query_file, output_dir) << std::endl;
        }
        const auto placement_end = std::chrono::steady_clock::now();
        const auto placement_time = (size_t)std::chrono::duration_cast<std::chrono::milliseconds>(placement_end - begin).count();
        if (std::getenv("EPIK_AMD_STAGE_TIMES"))  // (the reference's line below is in whole milliseconds)
            std::cout << "placement_time_us " << std::chrono::duration_cast<std::chrono::microseconds>(placement_end - begin).count()
                      << std::endl;
        std::cout << "Placement time: " << epik_amd::human_duration(placement_time) << " (" << placement_time << " ms)"
                  << std::endl;
        std::cout << "Done." << '\n' << std::flush;
    } catch (const std::runtime_error& error) {
        std::cerr << "Error: " << error.what() << std::endl;
        return -1;
    } catch (const std::exception& error) {  // std::stoul etc.
        std::cerr << "Error: " << error.what() << std::endl;
        return -1;
    }
    return 0;
}

#endif  // EPIK_AMD_NO_MAIN
