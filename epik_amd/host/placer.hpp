// placer.hpp -- host-side mirror of `epik::placer` over the C ABI of libepik_amd.so.
//
// Same names, arguments and error behaviour as the reference class
// (epik/include/epik/place.h:39-140): construct with (db, tree, keep_at_most, keep_factor,
// max_threads), call place(seq_records, num_threads) per FASTA batch, get a
// placed_collection whose string_views point into the caller's batch.
// Extra, MI355X-specific: a list of HIP devices (database replicated on each, no collective) and
// place_batches(): several FASTA batches in one launch on one of them -- the driver hands whole
// groups of batches to the devices in turn.
#ifndef EPIK_AMD_HOST_PLACER_HPP
#define EPIK_AMD_HOST_PLACER_HPP

#include <functional>
#include <optional>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "cohort.hpp"
#include "epik_amd.h"
#include "phylo_kmer_db.hpp"
#include "phylo_tree.hpp"
#include "seq_record.hpp"

namespace epik_amd::impl {

/// "sequence content -> list of headers" (place.h:42)
using sequence_map_t = std::unordered_map<std::string_view, std::vector<std::string_view>>;

/// A placement of one sequence (place.h:45-56)
struct placement {
    using weight_ratio_type = double;
    uint32_t branch_id;
    float score;
    weight_ratio_type weight_ratio;
    size_t count;
    phylo_node::branch_length_type distal_length;
    phylo_node::branch_length_type pendant_length;
};

/// place.h:59-68
struct placed_sequence {
    std::string_view sequence;
    std::vector<placement> placements;
};

/// place.h:72-75.  placed_seqs follow the first occurrence of each sequence in the batch
/// (the reference: std::unordered_map iteration order, place.cpp:57-61).
struct placed_collection {
    sequence_map_t sequence_map;
    std::vector<placed_sequence> placed_seqs;
};

/// The driver's own form of a placed batch: what a placed_collection holds, in five flat arrays (a
/// placed_collection is a hash-map node, a vector of headers and a vector of placements PER READ -- three
/// allocations each, made by the placing thread and freed by the writing one; at a million reads per second and
/// device that is what the driver would spend its time on).  Unique sequences in first-occurrence order.
struct placed_batch {
    std::vector<std::string_view> sequences;  // [n_unique]
    std::vector<uint32_t> row_begin;          // [n_unique + 1]: the placements of sequence u are rows[row_begin[u] .. row_begin[u + 1])
    std::vector<placement> rows;
    std::vector<uint32_t> name_begin;         // [n_unique + 1]: ... its headers names[name_begin[u] .. name_begin[u + 1]), input order
    std::vector<std::string_view> names;
    // strand modes other than forward (placer::set_strand) only, else empty:
    std::vector<uint8_t> strands;             // [n_unique]: 0 = the sequence was placed as given (+), 1 = its reverse complement (-)
    std::vector<uint32_t> unique_of;          // [batch size]: the unique sequence of each record, input order
    // translated placement (placer::set_translate) only, else empty:
    std::vector<uint8_t> frames;              // [n_unique]: the frame placed, 0..5 = +1 +2 +3 -1 -2 -3
    // pairs (placer::set_mates) only, else empty: `sequences` are the first mates, `strands` the fragments'
    std::vector<std::string_view> mates;      // [n_unique]: the second mate, as given
    // placement confidence (placer::set_assign) only, else empty; `unique_of` is then filled as well:
    std::vector<epik_amd_confidence> confidence;  // [n_unique]: LCA clade, its mass and the EDPL, from the device
    // taxonomic assignment with records (placer::set_taxonomy, per_read) only, else empty; `unique_of` is then filled as well:
    std::vector<epik_amd_taxon_record> taxa_records;  // [n_unique]: the taxon, its mass, the first row's taxon, the total
    size_t size() const noexcept { return sequences.size(); }
};

}  // namespace epik_amd::impl

namespace epik_amd {

/// Which strand of a nucleotide read is placed (epik_amd_placer_place_strands): the read as given (the reference's
/// contract, place.cpp:294), its reverse complement, or per read the better of the two.
enum class strand_mode : uint32_t { forward = EPIK_AMD_STRAND_FORWARD, reverse = EPIK_AMD_STRAND_REVERSE, both = EPIK_AMD_STRAND_BOTH };

/// Which frames of a nucleotide read are placed on an amino-acid database (epik_amd_placer_place_frames): +1 +2 +3,
/// -1 -2 -3, or all six; per read the best one.
enum class translate_mode : uint32_t { forward = EPIK_AMD_FRAMES_FORWARD, reverse = EPIK_AMD_FRAMES_REVERSE, both = EPIK_AMD_FRAMES_BOTH };

/// How the mates of a pair lie (epik_amd_placer_place_mates): FR, mate 2 the reverse complement of the fragment's far
/// end (Illumina paired-end), or FF.
enum class mate_orientation : uint32_t { fr = 0, ff = EPIK_AMD_MATES_FF };

class placer {
public:
    using placed_collection = impl::placed_collection;

    /// Shard g of a k-mer-space-sharded database (--db-shard), loaded when its turn comes and dropped as soon as
    /// its lists are on the device: the process never holds more than one shard on the host.
    using shard_loader = std::function<phylo_kmer_db(uint32_t shard_index)>;

    /// WARNING (as place.h:91-93): db and tree are kept by reference.
    /// db_shards == 1: the database replicated on every device of `devices`, whole groups of batches go to them in
    /// turn (no collective).  db_shards == G > 1: `db` holds shard 0 of G (phylo_kmer_db::shard_count() says so),
    /// load_shard(g) the others; handle g is created on devices[g % devices.size()] and every batch is placed by
    /// all of them together (epik_amd_placer_place_sharded) -- a database larger than one device's memory.
    placer(const phylo_kmer_db& db, const phylo_tree& original_tree, size_t keep_at_most, double keep_factor,
           size_t max_threads, std::vector<int> devices = {0}, uint32_t db_shards = 1,
           const shard_loader& load_shard = {});
    placer(const placer&) = delete;
    placer& operator=(const placer&) = delete;
    ~placer() noexcept;

    /// The reference's call: one batch, on the first device.
    placed_collection place(const std::vector<seq_record>& seq_records, size_t num_threads);

    /// Several batches in ONE launch on device `device_index` (of the list given to the constructor).
    /// Every batch is de-duplicated on its own, exactly as `place` does it (place.cpp:207-212: dedup is
    /// per batch), the unique reads of all of them cross the boundary together, and every batch gets
    /// its own placed_collection back.  Thread-safe across different devices.
    /// The host work on either side of the launch -- dedup, joining the reads, the placements with their branch
    /// lengths -- is per batch: `num_threads` threads share the batches.
    std::vector<placed_collection> place_batches(const std::vector<const std::vector<seq_record>*>& batches,
                                                 size_t device_index, size_t num_threads = 1);
    /// The same placement in the driver's flat form (impl::placed_batch): what epik-dna / epik-aa call.
    /// A placer of pairs (set_mates) is also given `mate_batches`: for every batch the second mates of its records, in
    /// their order.  A batch is then de-duplicated by the PAIR of sequences and every unique pair placed once.
    std::vector<impl::placed_batch> place_flat(const std::vector<const std::vector<seq_record>*>& batches,
                                               size_t device_index, size_t num_threads = 1,
                                               const std::vector<const std::vector<seq_record>*>* mate_batches = nullptr,
                                               const std::vector<uint32_t>* batch_samples = nullptr);

    /// How many callers may place at the same time (place_batches' device_index): the devices of a replicated
    /// database, ONE for a sharded one (all its handles work on every batch).
    size_t device_count() const noexcept { return _sharded ? 1 : _handles.size(); }
    size_t handle_count() const noexcept { return _handles.size(); }
    /// forward (the default) places through epik_amd_placer_place as ever; reverse / both through
    /// epik_amd_placer_place_strands, and the placed batches say per sequence which strand won.  Nucleotide
    /// databases, replicated (not --db-shard) only.
    void set_strand(strand_mode mode);
    strand_mode strand() const noexcept { return _strand; }
    /// The reads are nucleotide reads, translated on the device and placed through epik_amd_placer_place_frames;
    /// the placed batches say per sequence which frame won.  Amino-acid databases, replicated (not --db-shard) only.
    void set_translate(translate_mode mode);
    bool translating() const noexcept { return _translate; }
    /// The records come in pairs, two mates of one fragment: place_flat takes the second mates beside every batch and
    /// places each pair ONCE through epik_amd_placer_place_mates, on the strand(s) set_strand says (the fragment's).
    /// Nucleotide databases, replicated (not --db-shard), not translated.
    void set_mates(mate_orientation orientation);
    bool pairing() const noexcept { return _mates; }
    /// --profile-only: one device profile per handle (epik_amd_profile); from then on place_flat leaves the rows on the
    /// device, adds them to the profile of its device there -- every unique sequence with the number of its records as
    /// weight -- and returns batches without rows (sequences, names and the strand / frame bytes as ever).
    /// Replicated databases only (not --db-shard).
    void set_profile_only();
    bool profile_only() const noexcept { return !_profiles.empty(); }
    /// --assign: one device tree per handle (epik_amd_tree, from the tree given to the constructor); from then on
    /// place_flat goes through the epik_amd_placer_confidence_* entries and every placed batch carries the confidence
    /// record of each unique sequence, computed on the device from its rows -- with set_profile_only() the rows still
    /// never leave the device, only the 16 bytes per sequence do.  Replicated databases only (not --db-shard).
    void set_assign(uint32_t tau_q);
    bool assigning() const noexcept { return !_trees.empty(); }
    /// --cohort: one device cohort of `num_samples` samples per handle (epik_amd_cohort); from then on place_flat takes
    /// the sample of every batch (`batch_samples`, one value a batch: a batch never holds two samples), leaves the rows
    /// on the device and adds them to that sample's row there, every unique sequence with the number of its records as
    /// weight; it returns batches without rows and without strand / frame bytes.  Replicated databases only.
    void set_cohort(uint32_t num_samples);
    bool cohort_mode() const noexcept { return !_cohorts.empty(); }
    /// What read_cohort computes: `cells` (mass, best and totals, sized here) and `kr` of num_samples * num_samples values
    /// in every run, and each analysis whose member is engaged: its fields above the blank line are set on entry, those
    /// below are sized and filled here.  `strata` (--cohort-strata: strata[num_samples], or null) is what every test that
    /// permutes samples stays within; `distance` (EPIK_AMD_DISTANCE_*) is what permanova, pcoa, permdisp, model, mantel
    /// and anosim run over.
    struct cohort_squash {  ///< --cohort-squash: merges of num_samples - 1 records, num_merges of them used
        std::vector<epik_amd_squash_merge> merges;
        uint32_t num_merges = 0;
    };
    struct cohort_epca {  ///< --cohort-epca: mu of K, proj of num_samples * K, edge of K * num_branches, the tree's first[]
        uint32_t num_components = 5;

        std::vector<double> mu, proj, edge;
        epik_amd_epca_info info{};
        std::vector<uint32_t> first;
    };
    struct cohort_kmeans {  ///< --cohort-kmeans: samples of num_samples, clusters of K, centroids of K * num_branches
        uint32_t num_clusters = 0, max_iterations = 100;

        std::vector<epik_amd_kmeans_sample> samples;
        std::vector<epik_amd_kmeans_cluster> clusters;
        std::vector<double> centroids;
        epik_amd_kmeans_info info{};
    };
    struct cohort_alpha {  ///< --cohort-alpha: alpha of num_samples records
        std::vector<epik_amd_alpha> alpha;
    };
    struct cohort_rarefy {  ///< --cohort-rarefy: the curves at the depths j * depth_step, curve of num_samples * num_depths * 2
        uint32_t depth_step = 0, num_depths = 0;

        std::vector<double> curve;
    };
    struct cohort_correlation {  ///< --cohort-correlation with meta[S][M]: correlation of M * num_branches, used of M counts
        const double* meta = nullptr;
        uint32_t num_columns = 0;

        std::vector<epik_amd_correlation> correlation;
        std::vector<uint32_t> used;
    };
    struct cohort_dispersion {  ///< --cohort-dispersion: dispersion of num_branches records
        std::vector<epik_amd_dispersion> dispersion;
    };
    struct cohort_pcoa {  ///< --cohort-pcoa: mu of num_samples eigenvalues, coord of num_samples * K
        uint32_t num_components = 5;

        std::vector<double> mu, coord;
        epik_amd_pcoa_info info{};
    };
    struct cohort_unifrac {  ///< --cohort-unifrac: metrics (each at most once), matrix[i] of num_samples^2 for metrics[i]
        std::vector<uint32_t> metrics;

        std::vector<std::vector<double>> matrix;
    };
    /// What the tests that permute samples share; those over the factor columns labels[S][M] share these too
    struct cohort_permutation_test {
        uint32_t num_permutations = 999;
        uint64_t seed = 1;
    };
    struct cohort_factor_test : cohort_permutation_test {
        const uint32_t* labels = nullptr;
        uint32_t num_columns = 0;
    };
    struct cohort_permanova : cohort_factor_test {  ///< records of M * (1 + Q) tests (Q = 496 with pairwise), group_ss of M * 256
        bool pairwise = false;

        std::vector<epik_amd_permanova> records;
        std::vector<double> group_ss;
    };
    struct cohort_edgetest : cohort_factor_test {  ///< records of M * num_branches (column, branch) pairs
        std::vector<epik_amd_edgetest> records;
    };
    struct cohort_permdisp : cohort_factor_test {  ///< records of M * (1 + Q) tests, group_mean of M * 32, z of M * S
        bool pairwise = false;

        std::vector<epik_amd_permdisp> records;
        std::vector<double> group_mean, z;
    };
    struct cohort_anosim : cohort_factor_test {  ///< records of M columns
        std::vector<epik_amd_anosim> records;
    };
    /// The design kind[T], labels[S][T], values[S][T] of --cohort-model and --cohort-edge-model
    struct cohort_design_test : cohort_permutation_test {
        const uint32_t* kind = nullptr;
        const uint32_t* labels = nullptr;
        const double* values = nullptr;
        uint32_t num_terms = 0;
    };
    struct cohort_model : cohort_design_test {  ///< records of T + 1 terms, info and 64 aliased bytes
        std::vector<epik_amd_model_term> records;
        epik_amd_model_info info{};
        std::vector<uint8_t> aliased;
    };
    struct cohort_edgemodel : cohort_design_test {  ///< records of T * num_branches (term, branch) pairs, info, 64 aliased bytes
        std::vector<epik_amd_edgemodel> records;
        epik_amd_edgemodel_info info{};
        std::vector<uint8_t> aliased;
    };
    /// The sides values[Mv][S], matrices[Mm][S][S] and present[Mm][S] with the methods' bits and the control; records of
    /// Q * popcount(methods) tests
    struct cohort_mantel : cohort_permutation_test {
        const double* values = nullptr;
        const double* matrices = nullptr;
        const uint8_t* present = nullptr;
        uint32_t num_columns = 0, num_matrices = 0, methods = EPIK_AMD_MANTEL_PEARSON, control = EPIK_AMD_MANTEL_NO_CONTROL;

        std::vector<epik_amd_mantel> records;
    };
    struct cohort_request {
        sample_cohort cells;
        std::vector<double> kr;
        const uint32_t* strata = nullptr;
        uint32_t distance = EPIK_AMD_DISTANCE_KR;
        std::optional<cohort_unifrac> unifrac;
        std::optional<cohort_squash> squash;
        std::optional<cohort_epca> epca;
        std::optional<cohort_kmeans> kmeans;
        std::optional<cohort_alpha> alpha;
        std::optional<cohort_rarefy> rarefy;
        std::optional<cohort_correlation> correlation;
        std::optional<cohort_dispersion> dispersion;
        std::optional<cohort_permanova> permanova;
        std::optional<cohort_edgetest> edgetest;
        std::optional<cohort_pcoa> pcoa;
        std::optional<cohort_permdisp> permdisp;
        std::optional<cohort_model> model;
        std::optional<cohort_edgemodel> edgemodel;
        std::optional<cohort_mantel> mantel;
        std::optional<cohort_anosim> anosim;
    };
    /// The cohorts of all handles summed into the first one's (epik_amd_cohort_add_cells) and read back, and the KR
    /// distances and every engaged analysis of `request` computed on that device.  Once, at the end.
    void read_cohort(cohort_request& request);
    /// --taxonomy: one device taxonomy object per handle (epik_amd_taxonomy) from taxon_parent[T] and label[N], with one
    /// row of cells per sample of the cohort (call set_cohort first) or one row; from then on place_flat goes through
    /// the epik_amd_placer_taxa_* entries: every unique sequence is added with the number of its records as weight, a
    /// profile (set_profile_only) or the cohort is chained onto the same rows, and whatever the run does not write
    /// stays on the device.  per_read: every placed batch carries the record of each unique sequence.  Replicated
    /// databases only (not --db-shard), not with set_assign.
    void set_taxonomy(const std::vector<uint32_t>& taxon_parent, const std::vector<uint32_t>& label, uint32_t tau_q, bool per_read);
    bool taxonomy_mode() const noexcept { return !_taxa.empty(); }
    /// The objects of all handles summed into the first one's (epik_amd_taxonomy_add_cells) and read back: direct and
    /// assigned of num_samples * num_taxa cells each, totals of num_samples.  Once, at the end.
    void read_taxonomy(uint64_t* direct, uint64_t* assigned, epik_amd_taxa_totals* totals);
    /// --windows: what one batch of records gives (epik_amd_placer_paint_windows): record i owns the windows
    /// win_offsets[i] .. win_offsets[i + 1] - 1 and the segments at win_offsets[i] + s, s < n_segments[i]
    struct window_batch {
        std::vector<uint64_t> win_offsets;
        std::vector<epik_amd_window_record> records;
        std::vector<epik_amd_window_segment> segments;
        std::vector<uint32_t> n_segments;
        std::vector<uint8_t> strand;
        std::vector<uint32_t> n_rows;           ///< per_window only: the rows of every window ...
        std::vector<epik_amd_placement> best;   ///< ... and the first of them
    };
    /// Every record of `records` cut into windows, placed and painted on device `device_index`: no de-duplication, the
    /// records are independent.  Replicated databases only (not --db-shard).  One call a device at a time.
    window_batch paint_windows(const std::vector<seq_record>& records, size_t device_index, uint32_t window, uint32_t step,
                               uint32_t strand_mode, const std::vector<uint32_t>& group, uint32_t tau_q, bool per_window);
    /// The profiles of all devices read back and summed; `mass` and `best` of num_branches cells each.
    void read_profiles(uint64_t* mass, uint64_t* best, epik_amd_profile_totals& totals) const;
    /// distal_length / pendant_length of a placement on branch b (place.cpp:110-123, 435-437)
    std::vector<double> distal_lengths() const;
    const std::vector<double>& pendant_lengths() const noexcept { return _pendant_lengths; }

private:
    const phylo_kmer_db& _db;
    const phylo_tree& _original_tree;
    const float _threshold;
    const float _log_threshold;
    const size_t _keep_at_most;
    const double _keep_factor;
    std::vector<double> _pendant_lengths;
    std::vector<epik_amd_placer*> _handles;  // one per device (replicated) or per shard (sharded)
    std::vector<int> _devices;               // ... and the device of each
    std::vector<epik_amd_profile*> _profiles;  // set_profile_only(): one per handle
    std::vector<epik_amd_tree*> _trees;        // set_assign(): one per handle
    std::vector<epik_amd_cohort*> _cohorts;    // set_cohort(): one per handle
    std::vector<epik_amd_taxonomy*> _taxa;     // set_taxonomy(): one per handle
    uint32_t _taxa_tau_q = 0, _num_taxa = 0;
    bool _taxa_per_read = false;
    uint32_t _cohort_samples = 0;
    uint32_t _tau_q = 0;
    bool _sharded = false;
    strand_mode _strand = strand_mode::forward;
    bool _translate = false;
    translate_mode _frames = translate_mode::both;
    bool _mates = false;
    uint32_t _mates_mode = 0;  // EPIK_AMD_MATES_FF or 0
};

}  // namespace epik_amd
#endif
