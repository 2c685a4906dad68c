#include "placer.hpp"

#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "parallel.hpp"

// The driver is also linked against the test-only stub of the C ABI (Makefile: sanitize, stub), which places one
// strand only: its strand and frame entries are weak references here, and a library without it is an error when asked for.
#pragma weak epik_amd_placer_place_strands
#pragma weak epik_amd_placer_place_frames
#pragma weak epik_amd_profile_create
#pragma weak epik_amd_profile_destroy
#pragma weak epik_amd_profile_read
#pragma weak epik_amd_placer_profile_reads
#pragma weak epik_amd_placer_profile_strands
#pragma weak epik_amd_placer_profile_frames
#pragma weak epik_amd_placer_place_mates
#pragma weak epik_amd_placer_profile_mates
#pragma weak epik_amd_tree_create
#pragma weak epik_amd_tree_destroy
#pragma weak epik_amd_placer_confidence_reads
#pragma weak epik_amd_placer_confidence_strands
#pragma weak epik_amd_placer_confidence_frames
#pragma weak epik_amd_placer_confidence_mates
#pragma weak epik_amd_cohort_create
#pragma weak epik_amd_cohort_destroy
#pragma weak epik_amd_cohort_read
#pragma weak epik_amd_cohort_add_cells
#pragma weak epik_amd_cohort_kr
#pragma weak epik_amd_cohort_squash
#pragma weak epik_amd_cohort_epca
#pragma weak epik_amd_cohort_kmeans
#pragma weak epik_amd_cohort_alpha
#pragma weak epik_amd_cohort_rarefy
#pragma weak epik_amd_cohort_correlation
#pragma weak epik_amd_cohort_dispersion
#pragma weak epik_amd_cohort_permanova
#pragma weak epik_amd_cohort_edgetest
#pragma weak epik_amd_cohort_pcoa
#pragma weak epik_amd_cohort_permdisp
#pragma weak epik_amd_cohort_unifrac
#pragma weak epik_amd_cohort_permanova_metric
#pragma weak epik_amd_cohort_pcoa_metric
#pragma weak epik_amd_cohort_permdisp_metric
#pragma weak epik_amd_cohort_model_metric
#pragma weak epik_amd_cohort_permanova_strata
#pragma weak epik_amd_cohort_permdisp_strata
#pragma weak epik_amd_cohort_edgetest_strata
#pragma weak epik_amd_cohort_model_strata
#pragma weak epik_amd_cohort_edgemodel_strata
#pragma weak epik_amd_cohort_mantel
#pragma weak epik_amd_cohort_anosim
#pragma weak epik_amd_placer_cohort_reads
#pragma weak epik_amd_placer_cohort_strands
#pragma weak epik_amd_placer_cohort_frames
#pragma weak epik_amd_taxonomy_create
#pragma weak epik_amd_taxonomy_destroy
#pragma weak epik_amd_taxonomy_read
#pragma weak epik_amd_taxonomy_add_cells
#pragma weak epik_amd_placer_taxa_reads
#pragma weak epik_amd_placer_taxa_strands
#pragma weak epik_amd_placer_taxa_frames
#pragma weak epik_amd_placer_taxa_mates

namespace epik_amd {

using impl::placed_collection;
using impl::placed_sequence;
using impl::placement;
using impl::sequence_map_t;

placer::placer(const phylo_kmer_db& db, const phylo_tree& original_tree, size_t keep_at_most, double keep_factor,
               size_t /*max_threads*/, std::vector<int> devices, uint32_t db_shards, const shard_loader& load_shard)
    : _db{db}
    , _original_tree{original_tree}
    , _threshold{score_threshold(db.omega(), db.kmer_size(), alphabet_size(db.sequence_type()))}  // place.cpp:87
    , _log_threshold{std::log10(_threshold)}                                                      // place.cpp:88
    , _keep_at_most{keep_at_most}
    , _keep_factor{keep_factor}
{
    // pendant lengths (place.cpp:99-125)
    const auto& index = _db.tree_index();
    for (uint32_t i = 0; i < original_tree.get_node_count(); ++i) {
        const auto node = _original_tree.get_by_postorder_id(i);
        if (!node || i >= index.size())
            throw std::runtime_error("Could not find node by post-order id: " + std::to_string(i));
        const auto distal_length = (*node)->get_branch_length() / 2;
        auto mean_subtree_branch_length = 0.0;
        if (index[i].subtree_num_nodes > 1)
            mean_subtree_branch_length = index[i].subtree_total_length / (double)index[i].subtree_num_nodes;
        _pendant_lengths.push_back(mean_subtree_branch_length + distal_length);
    }

    const auto char_class = char_class_table(db.sequence_type());
    if (devices.empty()) devices.push_back(0);
    _sharded = db_shards > 1;
    if (_sharded && (db.shard_count() != db_shards || db.shard_index() != 0 || !load_shard))
        throw std::runtime_error("GPU placer: a sharded placer takes shard 0 of the database and a loader for the others");
    // one handle per device (the database replicated) or per shard (shard g on devices[g % devices.size()])
    const size_t n_handles = _sharded ? db_shards : devices.size();
    for (size_t g = 0; g < n_handles; ++g) {
        phylo_kmer_db loaded;  // shard g > 0: here until its lists are on the device
        if (_sharded && g > 0) {
            loaded = load_shard((uint32_t)g);
            if (loaded.shard_index() != g || loaded.shard_count() != db_shards || loaded.kmer_size() != db.kmer_size() ||
                loaded.num_keys() != db.num_keys() || loaded.omega() != db.omega())
                throw std::runtime_error("GPU placer: shard " + std::to_string(g) + " does not belong to this database");
        }
        const phylo_kmer_db& part = (_sharded && g > 0) ? loaded : db;
        epik_amd_placer_desc desc{};
        desc.abi_version = EPIK_AMD_ABI_VERSION;
        desc.kmer_size = (uint32_t)db.kmer_size();
        desc.alphabet_size = alphabet_size(db.sequence_type());
        desc.num_branches = (uint32_t)original_tree.get_node_count();
        desc.keep_at_most = (uint32_t)keep_at_most;
        desc.offset_bits = 64;
        desc.keep_factor = keep_factor;
        desc.threshold = _threshold;
        desc.log_threshold = _log_threshold;
        desc.num_keys = db.num_keys();
        desc.num_entries = part.values().size();
        desc.offsets = part.offsets().data();  // the sparse form: memory per present k-mer (ABI 3)
        desc.keys = part.keys().data();
        desc.num_present = part.keys().size();
        desc.values = part.values().data();
        desc.char_class = char_class.data();
        desc.device = devices[g % devices.size()];
        static const uint32_t no_key = 0;  // (an empty shard: keys must still be non-null to say "sparse form")
        if (desc.num_present == 0) desc.keys = &no_key;
        epik_amd_placer* handle = nullptr;
        const int rc = _sharded ? epik_amd_placer_create_sharded(&desc, (uint32_t)g, db_shards, &handle)
                                : epik_amd_placer_create(&desc, &handle);
        if (rc != EPIK_AMD_OK) {
            const std::string message = epik_amd_last_error();
            for (auto* h : _handles) epik_amd_placer_destroy(h);
            throw std::runtime_error("GPU placer: " + message);
        }
        _handles.push_back(handle);
        _devices.push_back(desc.device);
        if (_sharded && g == 0) {
            // A tree of the one-wavefront kernels leaves dense partial vectors, which place_sharded does not take:
            // said now, before the other shards are loaded and uploaded, not at the first batch.
            epik_amd_partial_info info{};
            if (epik_amd_placer_partial_info(handle, &info) == EPIK_AMD_OK && !info.lists) {
                for (auto* h : _handles) epik_amd_placer_destroy(h);
                _handles.clear();
                throw std::runtime_error("GPU placer: --db-shard needs the kernels of a large tree (this one has " +
                                         std::to_string(desc.num_branches) +
                                         " branches and fits one wavefront per read): replicate the database with --devices / --gpus instead");
            }
        }
    }
}

std::vector<double> placer::distal_lengths() const
{
    std::vector<double> out(_pendant_lengths.size(), 0.0);
    for (uint32_t i = 0; i < out.size(); ++i)
        if (const auto node = _original_tree.get_by_postorder_id(i)) out[i] = (*node)->get_branch_length() / 2;  // place.cpp:435
    return out;
}

void placer::set_strand(strand_mode mode)
{
    if (mode != strand_mode::forward) {
        if (_sharded) throw std::runtime_error("GPU placer: --strand reverse|both does not work with --db-shard > 1");
        if (alphabet_size(_db.sequence_type()) != 4)
            throw std::runtime_error("GPU placer: --strand reverse|both needs a nucleotide database");
        if (!&epik_amd_placer_place_strands)
            throw std::runtime_error("GPU placer: this libepik_amd has no strand placement");
    }
    _strand = mode;
}

void placer::set_translate(translate_mode mode)
{
    if (_sharded) throw std::runtime_error("GPU placer: --translate does not work with --db-shard > 1");
    if (alphabet_size(_db.sequence_type()) != 20)
        throw std::runtime_error("GPU placer: --translate needs an amino-acid database");
    if (!&epik_amd_placer_place_frames) throw std::runtime_error("GPU placer: this libepik_amd has no translated placement");
    _translate = true;
    _frames = mode;
}

void placer::set_mates(mate_orientation orientation)
{
    if (_sharded) throw std::runtime_error("GPU placer: --mates does not work with --db-shard > 1");
    if (alphabet_size(_db.sequence_type()) != 4) throw std::runtime_error("GPU placer: --mates needs a nucleotide database");
    if (_translate) throw std::runtime_error("GPU placer: --mates does not work with --translate");
    if (!&epik_amd_placer_place_mates || !&epik_amd_placer_profile_mates)
        throw std::runtime_error("GPU placer: this libepik_amd has no mates placement");
    _mates = true;
    _mates_mode = (uint32_t)orientation;
}

void placer::set_profile_only()
{
    if (_sharded) throw std::runtime_error("GPU placer: --profile-only does not work with --db-shard > 1");
    if (!&epik_amd_profile_create || !&epik_amd_profile_destroy || !&epik_amd_profile_read || !&epik_amd_placer_profile_reads ||
        !&epik_amd_placer_profile_strands || !&epik_amd_placer_profile_frames)
        throw std::runtime_error("GPU placer: this libepik_amd has no device profile");
    if (!_profiles.empty()) return;
    for (auto* h : _handles) {
        epik_amd_profile* profile = nullptr;
        if (epik_amd_profile_create(h, &profile) != EPIK_AMD_OK) {
            const std::string message = epik_amd_last_error();
            for (auto* made : _profiles) epik_amd_profile_destroy(made);
            _profiles.clear();
            throw std::runtime_error("GPU placer: " + message);
        }
        _profiles.push_back(profile);
    }
}

void placer::set_assign(uint32_t tau_q)
{
    if (_sharded) throw std::runtime_error("GPU placer: --assign does not work with --db-shard > 1");
    if (!&epik_amd_tree_create || !&epik_amd_tree_destroy || !&epik_amd_placer_confidence_reads || !&epik_amd_placer_confidence_strands ||
        !&epik_amd_placer_confidence_frames || !&epik_amd_placer_confidence_mates)
        throw std::runtime_error("GPU placer: this libepik_amd has no placement confidence");
    _tau_q = tau_q;
    if (!_trees.empty()) return;
    std::vector<uint32_t> parent;
    std::vector<double> length;
    for (const auto& node : _original_tree.nodes()) {
        parent.push_back(node.parent < 0 ? EPIK_AMD_TREE_NO_PARENT : (uint32_t)node.parent);
        length.push_back(node.branch_length);
    }
    for (size_t g = 0; g < _handles.size(); ++g) {
        epik_amd_tree* tree = nullptr;
        if (epik_amd_tree_create(_devices[g], parent.data(), length.data(), (uint32_t)parent.size(), &tree) != EPIK_AMD_OK) {
            const std::string message = epik_amd_last_error();
            for (auto* made : _trees) epik_amd_tree_destroy(made);
            _trees.clear();
            throw std::runtime_error("GPU placer: " + message);
        }
        _trees.push_back(tree);
    }
}

void placer::set_cohort(uint32_t num_samples)
{
    if (_sharded) throw std::runtime_error("GPU placer: --cohort does not work with --db-shard > 1");
    if (_mates || profile_only() || assigning())
        throw std::runtime_error("GPU placer: --cohort does not work with --mates, --profile-only or --assign");
    if (!&epik_amd_cohort_create || !&epik_amd_cohort_destroy || !&epik_amd_cohort_read || !&epik_amd_cohort_add_cells ||
        !&epik_amd_cohort_kr || !&epik_amd_placer_cohort_reads || !&epik_amd_placer_cohort_strands ||
        !&epik_amd_placer_cohort_frames || !&epik_amd_tree_create || !&epik_amd_tree_destroy)
        throw std::runtime_error("GPU placer: this libepik_amd has no device cohort");
    if (!_cohorts.empty()) return;
    _cohort_samples = num_samples;
    for (auto* h : _handles) {
        epik_amd_cohort* cohort = nullptr;
        if (epik_amd_cohort_create(h, num_samples, &cohort) != EPIK_AMD_OK) {
            const std::string message = epik_amd_last_error();
            for (auto* made : _cohorts) epik_amd_cohort_destroy(made);
            _cohorts.clear();
            throw std::runtime_error("GPU placer: " + message);
        }
        _cohorts.push_back(cohort);
    }
}

void placer::set_taxonomy(const std::vector<uint32_t>& taxon_parent, const std::vector<uint32_t>& label, uint32_t tau_q, bool per_read)
{
    if (_sharded) throw std::runtime_error("GPU placer: --taxonomy does not work with --db-shard > 1");
    if (assigning()) throw std::runtime_error("GPU placer: --taxonomy does not work with --assign");
    if (!&epik_amd_taxonomy_create || !&epik_amd_taxonomy_destroy || !&epik_amd_taxonomy_read || !&epik_amd_taxonomy_add_cells ||
        !&epik_amd_placer_taxa_reads || !&epik_amd_placer_taxa_strands || !&epik_amd_placer_taxa_frames || !&epik_amd_placer_taxa_mates)
        throw std::runtime_error("GPU placer: this libepik_amd has no taxonomic assignment");
    if (label.size() != _original_tree.get_node_count()) throw std::runtime_error("GPU placer: the labels do not fit the tree");
    _taxa_tau_q = tau_q, _taxa_per_read = per_read, _num_taxa = (uint32_t)taxon_parent.size();
    if (!_taxa.empty()) return;
    for (auto* h : _handles) {
        epik_amd_taxonomy* taxa = nullptr;
        if (epik_amd_taxonomy_create(h, taxon_parent.data(), _num_taxa, label.data(), cohort_mode() ? _cohort_samples : 1, &taxa) != EPIK_AMD_OK) {
            const std::string message = epik_amd_last_error();
            for (auto* made : _taxa) epik_amd_taxonomy_destroy(made);
            _taxa.clear();
            throw std::runtime_error("GPU placer: " + message);
        }
        _taxa.push_back(taxa);
    }
}

void placer::read_taxonomy(uint64_t* direct, uint64_t* assigned, epik_amd_taxa_totals* totals)
{
    const auto check = [](int rc) {
        if (rc != EPIK_AMD_OK) throw std::runtime_error(std::string("GPU placer: ") + epik_amd_last_error());
    };
    if (_taxa.empty()) throw std::runtime_error("GPU placer: no taxonomy (set_taxonomy)");
    // integer adds: the sum is the same bits whichever handle placed which batch
    for (size_t g = 1; g < _taxa.size(); ++g) {
        check(epik_amd_taxonomy_read(_taxa[g], direct, assigned, totals, nullptr));
        check(epik_amd_taxonomy_add_cells(_taxa[0], direct, assigned, totals));
        epik_amd_taxonomy_destroy(_taxa[g]);  // (summed once: a second read finds it all in the first)
        _taxa[g] = nullptr;
    }
    _taxa.resize(1);
    uint64_t bad_samples = 0;
    check(epik_amd_taxonomy_read(_taxa[0], direct, assigned, totals, &bad_samples));
    if (bad_samples) throw std::runtime_error("GPU placer: " + std::to_string(bad_samples) + " reads of no sample of the taxonomy object");
}

void placer::read_cohort(uint64_t* mass, uint64_t* best, epik_amd_profile_totals* totals, double* kr,
                         epik_amd_squash_merge* merges, uint32_t* num_merges, cohort_epca* epca, cohort_kmeans* kmeans,
                         cohort_diversity* diversity, cohort_edges* edges, cohort_permanova* permanova,
                         cohort_edgetest* edgetest, cohort_pcoa* pcoa, cohort_permdisp* permdisp, cohort_unifrac* unifrac,
                         cohort_model* model, cohort_mantel* mantel, cohort_anosim* anosim, cohort_edgemodel* edgemodel)
{
    if (edgemodel && !&epik_amd_cohort_edgemodel_strata) throw std::runtime_error("GPU placer: this libepik_amd has no edge model");
    if ((mantel && !&epik_amd_cohort_mantel) || (anosim && !&epik_amd_cohort_anosim))
        throw std::runtime_error("GPU placer: this libepik_amd has no Mantel test or no ANOSIM");
    if (model && !&epik_amd_cohort_model_metric) throw std::runtime_error("GPU placer: this libepik_amd has no sequential model");
    if (((permanova && permanova->strata) || (permdisp && permdisp->strata) || (edgetest && edgetest->strata) || (model && model->strata)) &&
        (!&epik_amd_cohort_permanova_strata || !&epik_amd_cohort_permdisp_strata || !&epik_amd_cohort_edgetest_strata ||
         !&epik_amd_cohort_model_strata))
        throw std::runtime_error("GPU placer: this libepik_amd has no permutations within strata");
    const uint32_t distance = unifrac ? unifrac->distance : EPIK_AMD_DISTANCE_KR;
    if (unifrac && (!&epik_amd_cohort_unifrac || !&epik_amd_cohort_permanova_metric || !&epik_amd_cohort_pcoa_metric ||
                    !&epik_amd_cohort_permdisp_metric))
        throw std::runtime_error("GPU placer: this libepik_amd has no UniFrac distances");
    if (permdisp && !&epik_amd_cohort_permdisp) throw std::runtime_error("GPU placer: this libepik_amd has no PERMDISP");
    if (pcoa && !&epik_amd_cohort_pcoa) throw std::runtime_error("GPU placer: this libepik_amd has no principal coordinates");
    if (edgetest && !&epik_amd_cohort_edgetest) throw std::runtime_error("GPU placer: this libepik_amd has no edge test");
    if (permanova && !&epik_amd_cohort_permanova) throw std::runtime_error("GPU placer: this libepik_amd has no PERMANOVA");
    if (edges && (!&epik_amd_cohort_correlation || !&epik_amd_cohort_dispersion))
        throw std::runtime_error("GPU placer: this libepik_amd has no edge correlation and dispersion");
    if (diversity && (!&epik_amd_cohort_alpha || !&epik_amd_cohort_rarefy))
        throw std::runtime_error("GPU placer: this libepik_amd has no alpha diversity and rarefaction");
    if (kmeans && !&epik_amd_cohort_kmeans) throw std::runtime_error("GPU placer: this libepik_amd has no phylogenetic k-means");
    if (num_merges && !&epik_amd_cohort_squash) throw std::runtime_error("GPU placer: this libepik_amd has no squash clustering");
    if (epca && !&epik_amd_cohort_epca) throw std::runtime_error("GPU placer: this libepik_amd has no edge principal components");
    const auto check = [](int rc) {
        if (rc != EPIK_AMD_OK) throw std::runtime_error(std::string("GPU placer: ") + epik_amd_last_error());
    };
    if (_cohorts.empty()) throw std::runtime_error("GPU placer: no cohort (set_cohort)");
    // integer adds: the sum is the same bits whichever handle placed which batch
    for (size_t g = 1; g < _cohorts.size(); ++g) {
        check(epik_amd_cohort_read(_cohorts[g], mass, best, totals, nullptr));
        check(epik_amd_cohort_add_cells(_cohorts[0], mass, best, totals));
        epik_amd_cohort_destroy(_cohorts[g]);  // (summed once: a second read_cohort finds it all in the first)
        _cohorts[g] = nullptr;
    }
    _cohorts.resize(1);
    uint64_t bad_samples = 0;
    check(epik_amd_cohort_read(_cohorts[0], mass, best, totals, &bad_samples));
    if (bad_samples) throw std::runtime_error("GPU placer: " + std::to_string(bad_samples) + " reads of no sample of the cohort");
    std::vector<uint32_t> parent;
    std::vector<double> length;
    for (const auto& node : _original_tree.nodes()) {
        parent.push_back(node.parent < 0 ? EPIK_AMD_TREE_NO_PARENT : (uint32_t)node.parent);
        length.push_back(node.branch_length);
    }
    epik_amd_tree* tree = nullptr;
    check(epik_amd_tree_create(_devices[0], parent.data(), length.data(), (uint32_t)parent.size(), &tree));
    int rc = epik_amd_cohort_kr(_cohorts[0], tree, length.data(), kr);
    if (unifrac) unifrac->matrix.assign(unifrac->metrics.size(), std::vector<double>((size_t)_cohort_samples * _cohort_samples, 0.0));
    for (size_t i = 0; rc == EPIK_AMD_OK && unifrac && i < unifrac->metrics.size(); ++i)
        rc = epik_amd_cohort_unifrac(_cohorts[0], tree, length.data(), unifrac->metrics[i], unifrac->matrix[i].data());
    if (rc == EPIK_AMD_OK && num_merges) rc = epik_amd_cohort_squash(_cohorts[0], tree, length.data(), merges, num_merges);
    if (rc == EPIK_AMD_OK && epca) {
        const size_t N = parent.size(), K = epca->num_components;
        epca->mu.assign(K, 0.0), epca->proj.assign((size_t)_cohort_samples * K, 0.0), epca->edge.assign(K * N, 0.0);
        epca->first.resize(N);
        for (size_t b = 0; b < N; ++b) epca->first[b] = (uint32_t)b;  // (post-order ids: a parent comes after its children)
        for (size_t b = 0; b < N; ++b)
            if (parent[b] != EPIK_AMD_TREE_NO_PARENT && parent[b] < N)
                epca->first[parent[b]] = std::min(epca->first[parent[b]], epca->first[b]);
        rc = epik_amd_cohort_epca(_cohorts[0], tree, epca->num_components, epca->mu.data(), epca->proj.data(), epca->edge.data(),
                                  &epca->info);
    }
    if (rc == EPIK_AMD_OK && kmeans) {
        const size_t N = parent.size(), K = kmeans->num_clusters;
        kmeans->samples.assign(_cohort_samples, epik_amd_kmeans_sample{}), kmeans->clusters.assign(K, epik_amd_kmeans_cluster{});
        kmeans->centroids.assign(K * N, 0.0);
        rc = epik_amd_cohort_kmeans(_cohorts[0], tree, length.data(), kmeans->num_clusters, kmeans->max_iterations,
                                    kmeans->samples.data(), kmeans->clusters.data(), kmeans->centroids.data(), &kmeans->info);
    }
    if (rc == EPIK_AMD_OK && diversity && diversity->with_alpha) {
        diversity->alpha.assign(_cohort_samples, epik_amd_alpha{});
        rc = epik_amd_cohort_alpha(_cohorts[0], tree, length.data(), diversity->alpha.data());
    }
    if (rc == EPIK_AMD_OK && diversity && diversity->num_depths) {
        diversity->curve.assign((size_t)_cohort_samples * diversity->num_depths * 2, 0.0);
        rc = epik_amd_cohort_rarefy(_cohorts[0], tree, length.data(), diversity->depth_step, diversity->num_depths,
                                    diversity->curve.data());
    }
    if (rc == EPIK_AMD_OK && edges && edges->num_columns) {
        edges->correlation.assign((size_t)edges->num_columns * parent.size(), epik_amd_correlation{});
        edges->used.assign(edges->num_columns, 0);
        rc = epik_amd_cohort_correlation(_cohorts[0], tree, edges->meta, edges->num_columns, edges->correlation.data(),
                                         edges->used.data());
    }
    if (rc == EPIK_AMD_OK && edges && edges->with_dispersion) {
        edges->dispersion.assign(parent.size(), epik_amd_dispersion{});
        rc = epik_amd_cohort_dispersion(_cohorts[0], tree, edges->dispersion.data());
    }
    if (rc == EPIK_AMD_OK && permanova) {
        const size_t slots = 1 + (permanova->pairwise ? EPIK_AMD_PERMANOVA_PAIR_SLOTS : 0);
        permanova->records.assign(permanova->num_columns * slots, epik_amd_permanova{});
        permanova->group_ss.assign((size_t)permanova->num_columns * EPIK_AMD_PERMANOVA_MAX_GROUPS, 0.0);
        rc = permanova->strata
                 ? epik_amd_cohort_permanova_strata(_cohorts[0], tree, length.data(), distance, permanova->labels, permanova->num_columns,
                                                    permanova->num_permutations, permanova->seed, permanova->pairwise ? 1 : 0,
                                                    permanova->records.data(), nullptr, permanova->group_ss.data(), permanova->strata)
             : distance != EPIK_AMD_DISTANCE_KR
                 ? epik_amd_cohort_permanova_metric(_cohorts[0], tree, length.data(), distance, permanova->labels, permanova->num_columns,
                                                    permanova->num_permutations, permanova->seed, permanova->pairwise ? 1 : 0,
                                                    permanova->records.data(), nullptr, permanova->group_ss.data())
                 : epik_amd_cohort_permanova(_cohorts[0], tree, length.data(), permanova->labels, permanova->num_columns,
                                             permanova->num_permutations, permanova->seed, permanova->pairwise ? 1 : 0,
                                             permanova->records.data(), nullptr, permanova->group_ss.data());
    }
    if (rc == EPIK_AMD_OK && edgetest) {
        edgetest->records.assign((size_t)edgetest->num_columns * parent.size(), epik_amd_edgetest{});
        rc = edgetest->strata
                 ? epik_amd_cohort_edgetest_strata(_cohorts[0], tree, edgetest->labels, edgetest->num_columns, edgetest->num_permutations,
                                                   edgetest->seed, edgetest->records.data(), nullptr, nullptr, edgetest->strata)
                 : epik_amd_cohort_edgetest(_cohorts[0], tree, edgetest->labels, edgetest->num_columns, edgetest->num_permutations,
                                            edgetest->seed, edgetest->records.data(), nullptr, nullptr);
    }
    if (rc == EPIK_AMD_OK && pcoa) {
        pcoa->mu.assign(_cohort_samples, 0.0), pcoa->coord.assign((size_t)_cohort_samples * pcoa->num_components, 0.0);
        rc = distance != EPIK_AMD_DISTANCE_KR
                 ? epik_amd_cohort_pcoa_metric(_cohorts[0], tree, length.data(), distance, pcoa->num_components, pcoa->mu.data(),
                                               pcoa->coord.data(), &pcoa->info)
                 : epik_amd_cohort_pcoa(_cohorts[0], tree, length.data(), pcoa->num_components, pcoa->mu.data(), pcoa->coord.data(),
                                        &pcoa->info);
    }
    if (rc == EPIK_AMD_OK && permdisp) {
        const size_t slots = 1 + (permdisp->pairwise ? EPIK_AMD_PERMDISP_PAIR_SLOTS : 0);
        permdisp->records.assign(permdisp->num_columns * slots, epik_amd_permdisp{});
        permdisp->group_mean.assign((size_t)permdisp->num_columns * EPIK_AMD_PERMDISP_MAX_GROUPS, 0.0);
        permdisp->z.assign((size_t)permdisp->num_columns * _cohort_samples, 0.0);
        rc = permdisp->strata
                 ? epik_amd_cohort_permdisp_strata(_cohorts[0], tree, length.data(), distance, permdisp->labels, permdisp->num_columns,
                                                   permdisp->num_permutations, permdisp->seed, permdisp->pairwise ? 1 : 0,
                                                   permdisp->records.data(), nullptr, permdisp->group_mean.data(), permdisp->z.data(),
                                                   permdisp->strata)
             : distance != EPIK_AMD_DISTANCE_KR
                 ? epik_amd_cohort_permdisp_metric(_cohorts[0], tree, length.data(), distance, permdisp->labels, permdisp->num_columns,
                                                   permdisp->num_permutations, permdisp->seed, permdisp->pairwise ? 1 : 0,
                                                   permdisp->records.data(), nullptr, permdisp->group_mean.data(), permdisp->z.data())
                 : epik_amd_cohort_permdisp(_cohorts[0], tree, length.data(), permdisp->labels, permdisp->num_columns,
                                            permdisp->num_permutations, permdisp->seed, permdisp->pairwise ? 1 : 0,
                                            permdisp->records.data(), nullptr, permdisp->group_mean.data(), permdisp->z.data());
    }
    if (rc == EPIK_AMD_OK && model) {
        model->records.assign((size_t)model->num_terms + 1, epik_amd_model_term{});
        model->aliased.assign(EPIK_AMD_MODEL_MAX_COLUMNS, 0);
        rc = model->strata
                 ? epik_amd_cohort_model_strata(_cohorts[0], tree, length.data(), distance, model->kind, model->labels, model->values,
                                                model->num_terms, model->num_permutations, model->seed, model->records.data(),
                                                &model->info, nullptr, model->aliased.data(), model->strata)
                 : epik_amd_cohort_model_metric(_cohorts[0], tree, length.data(), distance, model->kind, model->labels, model->values,
                                                model->num_terms, model->num_permutations, model->seed, model->records.data(),
                                                &model->info, nullptr, model->aliased.data());
    }
    if (rc == EPIK_AMD_OK && edgemodel) {
        edgemodel->records.assign((size_t)edgemodel->num_terms * parent.size(), epik_amd_edgemodel{});
        edgemodel->aliased.assign(EPIK_AMD_MODEL_MAX_COLUMNS, 0);
        rc = epik_amd_cohort_edgemodel_strata(_cohorts[0], tree, edgemodel->kind, edgemodel->labels, edgemodel->values, edgemodel->num_terms,
                                              edgemodel->num_permutations, edgemodel->seed, edgemodel->records.data(), &edgemodel->info,
                                              nullptr, nullptr, edgemodel->aliased.data(), edgemodel->strata);
    }
    if (rc == EPIK_AMD_OK && mantel) {
        const size_t per_side = (mantel->methods & 1u) + (mantel->methods >> 1 & 1u);
        mantel->records.assign(((size_t)mantel->num_columns + mantel->num_matrices) * per_side, epik_amd_mantel{});
        rc = epik_amd_cohort_mantel(_cohorts[0], tree, length.data(), distance, mantel->values, mantel->num_columns, mantel->matrices,
                                    mantel->present, mantel->num_matrices, mantel->methods, mantel->control, mantel->num_permutations,
                                    mantel->seed, mantel->strata, mantel->records.data(), nullptr);
    }
    if (rc == EPIK_AMD_OK && anosim) {
        anosim->records.assign(anosim->num_columns, epik_amd_anosim{});
        rc = epik_amd_cohort_anosim(_cohorts[0], tree, length.data(), distance, anosim->labels, anosim->num_columns,
                                    anosim->num_permutations, anosim->seed, anosim->strata, anosim->records.data(), nullptr);
    }
    const std::string message = rc != EPIK_AMD_OK ? epik_amd_last_error() : "";
    epik_amd_tree_destroy(tree);
    if (rc != EPIK_AMD_OK) throw std::runtime_error("GPU placer: " + message);
}

void placer::read_profiles(uint64_t* mass, uint64_t* best, epik_amd_profile_totals& totals) const
{
    const size_t n = _original_tree.get_node_count();
    std::vector<uint64_t> m(n), b(n);
    std::fill(mass, mass + n, 0), std::fill(best, best + n, 0);
    totals = {};
    for (auto* profile : _profiles) {
        epik_amd_profile_totals t{};
        if (epik_amd_profile_read(profile, m.data(), b.data(), &t) != EPIK_AMD_OK)
            throw std::runtime_error(std::string("GPU placer: ") + epik_amd_last_error());
        for (size_t i = 0; i < n; ++i) mass[i] += m[i], best[i] += b[i];
        totals.placed += t.placed, totals.no_hit += t.no_hit, totals.too_short += t.too_short;
        totals.too_narrow += t.too_narrow, totals.bad_rows += t.bad_rows;
    }
}

placer::~placer() noexcept
{
    for (auto* profile : _profiles) epik_amd_profile_destroy(profile);
    for (auto* cohort : _cohorts) epik_amd_cohort_destroy(cohort);
    for (auto* tree : _trees) epik_amd_tree_destroy(tree);
    for (auto* taxa : _taxa)
        if (taxa) epik_amd_taxonomy_destroy(taxa);
    for (auto* h : _handles) epik_amd_placer_destroy(h);
}

placed_collection placer::place(const std::vector<seq_record>& seq_records, size_t /*num_threads*/)
{
    auto placed = place_batches({&seq_records}, 0, 1);
    return std::move(placed[0]);
}

namespace {

// 64-bit hash of a sequence, eight bytes at a time (dedup of a batch: place.cpp:73-81 groups by content)
inline uint64_t hash_bytes(std::string_view s)
{
    uint64_t h = 0x9e3779b97f4a7c15ull ^ (uint64_t)s.size();
    const char* p = s.data();
    size_t n = s.size();
    while (n >= 8) {
        uint64_t w;
        std::memcpy(&w, p, 8);
        h = (h ^ w) * 0xff51afd7ed558ccdull;
        h ^= h >> 32;
        p += 8, n -= 8;
    }
    uint64_t w = 0;
    std::memcpy(&w, p, n);
    h = (h ^ w) * 0xc4ceb9fe1a85ec53ull;
    return h ^ (h >> 29);
}

}  // namespace

std::vector<impl::placed_batch> placer::place_flat(const std::vector<const std::vector<seq_record>*>& batches,
                                                   size_t device_index, size_t num_threads,
                                                   const std::vector<const std::vector<seq_record>*>* mate_batches,
                                                   const std::vector<uint32_t>* batch_samples)
{
    if (device_index >= device_count()) throw std::runtime_error("GPU placer: no such device index");
    if (_mates != (mate_batches != nullptr) || (mate_batches && mate_batches->size() != batches.size()))
        throw std::runtime_error("GPU placer: a placer of pairs (set_mates) takes a batch of mates for every batch, any other none");
    if (cohort_mode() != (batch_samples != nullptr) || (batch_samples && batch_samples->size() != batches.size()))
        throw std::runtime_error("GPU placer: a placer of a cohort (set_cohort) takes the sample of every batch, any other none");
    const size_t per = _mates ? 2 : 1;  // reads a unique item sends through the boundary
    std::vector<impl::placed_batch> out(batches.size());
    // identical sequences of a batch are placed once (place.cpp:73-81, 207-212); the unique reads of
    // all batches go through the boundary in one call.  The batches are independent of each other up to
    // that call and after it: `num_threads` threads take them one at a time.
    std::vector<size_t> first_unique(batches.size() + 1, 0), first_byte(batches.size() + 1, 0);
    parallel_for(batches.size(), num_threads, [&](size_t b) {
        const auto& batch = *batches[b];
        const std::vector<seq_record>* mates = mate_batches ? (*mate_batches)[b] : nullptr;
        if (mates && mates->size() != batch.size()) throw std::runtime_error("GPU placer: a batch and its mates differ in size");
        impl::placed_batch pb;  // (the thread's own while it grows: neighbours in out[] share cache lines)
        if (batch.size() >= 0xffffffffull) throw std::runtime_error("GPU placer: a batch of 2^32 reads or more");
        // open addressing over the positions of the batch: slot -> index of a unique sequence + 1
        size_t cap = 16;
        while (cap < 2 * batch.size()) cap *= 2;
        std::vector<uint32_t> table(cap, 0), unique_of(batch.size());
        pb.sequences.reserve(batch.size());
        std::vector<uint32_t> n_names;
        n_names.reserve(batch.size());
        size_t bytes = 0;
        for (size_t i = 0; i < batch.size(); ++i) {
            // (pairs: the same, by the PAIR of sequences)
            const std::string_view seq = batch[i].sequence(), mate = mates ? (*mates)[i].sequence() : std::string_view();
            uint64_t hash = hash_bytes(seq);
            if (mates) hash = (hash ^ (hash_bytes(mate) + 0x9e3779b97f4a7c15ull + (hash << 6) + (hash >> 2)));
            size_t slot = (size_t)hash & (cap - 1);
            for (;;) {
                const uint32_t u = table[slot];
                if (u == 0) {
                    table[slot] = (uint32_t)pb.sequences.size() + 1;
                    unique_of[i] = (uint32_t)pb.sequences.size();
                    pb.sequences.push_back(seq);
                    if (mates) pb.mates.push_back(mate);
                    n_names.push_back(1);
                    bytes += seq.size() + mate.size();
                    break;
                }
                if (pb.sequences[u - 1] == seq && (!mates || pb.mates[u - 1] == mate)) {
                    unique_of[i] = u - 1;
                    ++n_names[u - 1];
                    break;
                }
                slot = (slot + 1) & (cap - 1);
            }
        }
        // the headers of every unique sequence, in input order (jplace "nm", jplace.cpp:141-158)
        const size_t n_unique = pb.sequences.size();
        pb.name_begin.assign(n_unique + 1, 0);
        for (size_t u = 0; u < n_unique; ++u) pb.name_begin[u + 1] = pb.name_begin[u] + n_names[u];
        pb.names.resize(batch.size());
        std::vector<uint32_t> at(pb.name_begin.begin(), pb.name_begin.end() - 1);
        for (size_t i = 0; i < batch.size(); ++i) pb.names[at[unique_of[i]]++] = batch[i].header();
        if (_strand != strand_mode::forward || _translate || assigning() || _taxa_per_read) pb.unique_of = std::move(unique_of);  // (the strand / frame / record of each record)
        first_unique[b + 1] = n_unique;
        first_byte[b + 1] = bytes;
        out[b] = std::move(pb);
    });
    for (size_t b = 0; b < batches.size(); ++b) {
        first_unique[b + 1] += first_unique[b];
        first_byte[b + 1] += first_byte[b];
    }
    const size_t n = first_unique.back();
    if (n == 0) {
        for (auto& pb : out) pb.row_begin.assign(1, 0);
        return out;
    }
    std::unique_ptr<char[]> bytes(new char[first_byte.back() + 1]);
    std::unique_ptr<uint64_t[]> offsets(new uint64_t[per * n + 1]);
    offsets[per * n] = first_byte.back();
    parallel_for(batches.size(), num_threads, [&](size_t b) {
        size_t at = first_byte[b], i = per * first_unique[b];
        for (size_t u = 0; u < out[b].sequences.size(); ++u) {
            const auto seq = out[b].sequences[u];
            offsets[i++] = at;
            std::memcpy(bytes.get() + at, seq.data(), seq.size());
            at += seq.size();
            if (!_mates) continue;  // (interleaved: mate 1, mate 2 of every pair)
            const auto mate = out[b].mates[u];
            offsets[i++] = at;
            std::memcpy(bytes.get() + at, mate.data(), mate.size());
            at += mate.size();
        }
    });
    const uint32_t mates_mode = (uint32_t)_strand | _mates_mode;
    // --taxonomy: the entry of the run's placement with every chunk's rows added to this device's taxonomy object;
    // whatever pointer is null stays on the device.  Every unique sequence weighs the number of its records.
    std::unique_ptr<uint32_t[]> taxa_weights;
    std::unique_ptr<epik_amd_taxon_record[]> taxa_records;
    const auto taxa_call = [&](epik_amd_placement* t_rows, uint32_t* t_n_rows, uint32_t* t_counts, uint8_t* t_labels,
                               const uint32_t* t_samples, epik_amd_profile* t_profile, epik_amd_cohort* t_cohort) {
        taxa_weights.reset(new uint32_t[n]);
        for (size_t b = 0; b < batches.size(); ++b)
            for (size_t u = 0; u < out[b].size(); ++u)
                taxa_weights[first_unique[b] + u] = out[b].name_begin[u + 1] - out[b].name_begin[u];
        if (_taxa_per_read) taxa_records.reset(new epik_amd_taxon_record[n]);
        auto* handle = _handles[device_index];
        auto* taxa = _taxa.size() > device_index ? _taxa[device_index] : nullptr;
        if (!taxa) throw std::runtime_error("GPU placer: the taxonomy objects have been read (read_taxonomy ends the placement)");
        const int t_rc =
            _mates ? epik_amd_placer_taxa_mates(handle, bytes.get(), offsets.get(), n, mates_mode, t_rows, t_n_rows, t_counts, t_labels,
                                                taxa, _taxa_tau_q, taxa_records.get(), taxa_weights.get(), t_samples, t_profile, t_cohort)
            : _translate ? epik_amd_placer_taxa_frames(handle, bytes.get(), offsets.get(), n, (uint32_t)_frames, t_rows, t_n_rows, t_counts,
                                                       t_labels, taxa, _taxa_tau_q, taxa_records.get(), taxa_weights.get(), t_samples,
                                                       t_profile, t_cohort)
            : _strand != strand_mode::forward
                ? epik_amd_placer_taxa_strands(handle, bytes.get(), offsets.get(), n, (uint32_t)_strand, t_rows, t_n_rows, t_counts,
                                               t_labels, taxa, _taxa_tau_q, taxa_records.get(), taxa_weights.get(), t_samples, t_profile,
                                               t_cohort)
                : epik_amd_placer_taxa_reads(handle, bytes.get(), offsets.get(), n, t_rows, t_n_rows, t_counts, taxa, _taxa_tau_q,
                                             taxa_records.get(), taxa_weights.get(), t_samples, t_profile, t_cohort);
        if (t_rc != EPIK_AMD_OK) throw std::runtime_error(std::string("GPU placer: ") + epik_amd_last_error());
        if (taxa_records)
            for (size_t b = 0; b < batches.size(); ++b)
                out[b].taxa_records.assign(taxa_records.get() + first_unique[b], taxa_records.get() + first_unique[b] + out[b].size());
        return t_rc;
    };
    if (cohort_mode() && taxonomy_mode()) {
        // the cohort's placement with the taxonomy in front: the same rows go to both, sample by sample; nothing but the
        // records (per_read) comes back
        std::unique_ptr<uint32_t[]> samples(new uint32_t[n]);
        for (size_t b = 0; b < batches.size(); ++b)
            for (size_t u = 0; u < out[b].size(); ++u) samples[first_unique[b] + u] = (*batch_samples)[b];
        auto* cohort = _cohorts.size() > device_index ? _cohorts[device_index] : nullptr;
        if (!cohort) throw std::runtime_error("GPU placer: the cohorts have been read (read_cohort ends a cohort placement)");
        taxa_call(nullptr, nullptr, nullptr, nullptr, samples.get(), nullptr, cohort);
        for (auto& pb : out) pb.row_begin.assign(pb.size() + 1, 0);
        return out;
    }
    if (cohort_mode()) {
        // the rows stay on the device and are summed there into the row of each batch's sample; nothing comes back
        std::unique_ptr<uint32_t[]> weights(new uint32_t[n]), samples(new uint32_t[n]);
        for (size_t b = 0; b < batches.size(); ++b)
            for (size_t u = 0; u < out[b].size(); ++u) {
                weights[first_unique[b] + u] = out[b].name_begin[u + 1] - out[b].name_begin[u];
                samples[first_unique[b] + u] = (*batch_samples)[b];
            }
        auto* handle = _handles[device_index];
        auto* cohort = _cohorts.size() > device_index ? _cohorts[device_index] : nullptr;
        if (!cohort) throw std::runtime_error("GPU placer: the cohorts have been read (read_cohort ends a cohort placement)");
        const int rc = _translate ? epik_amd_placer_cohort_frames(handle, cohort, bytes.get(), offsets.get(), weights.get(),
                                                                  samples.get(), n, (uint32_t)_frames, nullptr)
                       : _strand != strand_mode::forward
                           ? epik_amd_placer_cohort_strands(handle, cohort, bytes.get(), offsets.get(), weights.get(),
                                                            samples.get(), n, (uint32_t)_strand, nullptr)
                           : epik_amd_placer_cohort_reads(handle, cohort, bytes.get(), offsets.get(), weights.get(),
                                                          samples.get(), n);
        if (rc != EPIK_AMD_OK) throw std::runtime_error(std::string("GPU placer: ") + epik_amd_last_error());
        for (auto& pb : out) pb.row_begin.assign(pb.size() + 1, 0);
        return out;
    }
    if (profile_only()) {
        // the rows stay on the device and are summed there; what comes back is the strand / frame byte per sequence
        std::unique_ptr<uint32_t[]> weights(new uint32_t[n]);
        for (size_t b = 0; b < batches.size(); ++b)
            for (size_t u = 0; u < out[b].size(); ++u)
                weights[first_unique[b] + u] = out[b].name_begin[u + 1] - out[b].name_begin[u];
        std::unique_ptr<uint8_t[]> labels;
        if (_translate || _strand != strand_mode::forward) labels.reset(new uint8_t[n]);
        auto* handle = _handles[device_index];
        auto* profile = _profiles[device_index];
        std::unique_ptr<epik_amd_confidence[]> conf;
        if (assigning()) {  // the same placement through the confidence entries: the rows stay, 16 bytes a sequence come back
            conf.reset(new epik_amd_confidence[n]);
        }
        auto* tree = assigning() ? _trees[device_index] : nullptr;
        const int rc = taxonomy_mode() ? taxa_call(nullptr, nullptr, nullptr, labels.get(), nullptr, profile, nullptr)
            : assigning()
            ? (_mates ? epik_amd_placer_confidence_mates(handle, bytes.get(), offsets.get(), n, mates_mode, nullptr, nullptr, nullptr,
                                                         labels.get(), tree, _tau_q, conf.get(), profile, weights.get())
               : _translate ? epik_amd_placer_confidence_frames(handle, bytes.get(), offsets.get(), n, (uint32_t)_frames, nullptr, nullptr,
                                                                nullptr, labels.get(), tree, _tau_q, conf.get(), profile, weights.get())
               : _strand != strand_mode::forward
                   ? epik_amd_placer_confidence_strands(handle, bytes.get(), offsets.get(), n, (uint32_t)_strand, nullptr, nullptr, nullptr,
                                                        labels.get(), tree, _tau_q, conf.get(), profile, weights.get())
                   : epik_amd_placer_confidence_reads(handle, bytes.get(), offsets.get(), n, nullptr, nullptr, nullptr, tree, _tau_q,
                                                      conf.get(), profile, weights.get()))
            : _mates ? epik_amd_placer_profile_mates(handle, profile, bytes.get(), offsets.get(), weights.get(), n,
                                                               mates_mode, labels.get())
                       : _translate ? epik_amd_placer_profile_frames(handle, profile, bytes.get(), offsets.get(), weights.get(), n,
                                                                   (uint32_t)_frames, labels.get())
                       : _strand != strand_mode::forward
                           ? epik_amd_placer_profile_strands(handle, profile, bytes.get(), offsets.get(), weights.get(), n,
                                                             (uint32_t)_strand, labels.get())
                           : epik_amd_placer_profile_reads(handle, profile, bytes.get(), offsets.get(), weights.get(), n);
        if (rc != EPIK_AMD_OK) throw std::runtime_error(std::string("GPU placer: ") + epik_amd_last_error());
        for (size_t b = 0; b < batches.size(); ++b) {
            auto& pb = out[b];
            pb.row_begin.assign(pb.size() + 1, 0);
            if (conf) pb.confidence.assign(conf.get() + first_unique[b], conf.get() + first_unique[b] + pb.size());
            if (!labels) continue;
            const uint8_t* first = labels.get() + first_unique[b];
            (_translate ? pb.frames : pb.strands).assign(first, first + pb.size());
        }
        return out;
    }
    std::unique_ptr<epik_amd_placement[]> rows(new epik_amd_placement[n * _keep_at_most]);
    std::unique_ptr<uint32_t[]> n_rows(new uint32_t[n]), counts(new uint32_t[n * _keep_at_most]);
    std::unique_ptr<uint8_t[]> strands;  // (reverse / both only: forward goes through epik_amd_placer_place as ever)
    std::unique_ptr<uint8_t[]> frames;   // (translated placement only)
    std::unique_ptr<epik_amd_confidence[]> conf;  // (--assign only)
    int rc;
    if (taxonomy_mode()) {
        // the same placements through the taxonomy entries: the rows come back as ever, the cells stay on the device
        if (_translate) frames.reset(new uint8_t[n]);
        else if (_strand != strand_mode::forward) strands.reset(new uint8_t[n]);
        rc = taxa_call(rows.get(), n_rows.get(), counts.get(), _translate ? frames.get() : strands.get(), nullptr, nullptr, nullptr);
    } else if (assigning()) {
        // the same placements through the confidence entries: the records come back beside the rows
        conf.reset(new epik_amd_confidence[n]);
        auto* handle = _handles[device_index];
        auto* tree = _trees[device_index];
        if (_mates) {
            if (_strand != strand_mode::forward) strands.reset(new uint8_t[n]);
            rc = epik_amd_placer_confidence_mates(handle, bytes.get(), offsets.get(), n, mates_mode, rows.get(), n_rows.get(), counts.get(),
                                                  strands.get(), tree, _tau_q, conf.get(), nullptr, nullptr);
        } else if (_translate) {
            frames.reset(new uint8_t[n]);
            rc = epik_amd_placer_confidence_frames(handle, bytes.get(), offsets.get(), n, (uint32_t)_frames, rows.get(), n_rows.get(),
                                                   counts.get(), frames.get(), tree, _tau_q, conf.get(), nullptr, nullptr);
        } else if (_strand != strand_mode::forward) {
            strands.reset(new uint8_t[n]);
            rc = epik_amd_placer_confidence_strands(handle, bytes.get(), offsets.get(), n, (uint32_t)_strand, rows.get(), n_rows.get(),
                                                    counts.get(), strands.get(), tree, _tau_q, conf.get(), nullptr, nullptr);
        } else {
            rc = epik_amd_placer_confidence_reads(handle, bytes.get(), offsets.get(), n, rows.get(), n_rows.get(), counts.get(), tree,
                                                  _tau_q, conf.get(), nullptr, nullptr);
        }
    } else if (_mates) {
        if (_strand != strand_mode::forward) strands.reset(new uint8_t[n]);
        rc = epik_amd_placer_place_mates(_handles[device_index], bytes.get(), offsets.get(), n, mates_mode, rows.get(),
                                         n_rows.get(), counts.get(), strands.get());
    } else if (_translate) {
        frames.reset(new uint8_t[n]);
        rc = epik_amd_placer_place_frames(_handles[device_index], bytes.get(), offsets.get(), n, (uint32_t)_frames,
                                          rows.get(), n_rows.get(), counts.get(), frames.get());
    } else if (_strand != strand_mode::forward) {
        strands.reset(new uint8_t[n]);
        rc = epik_amd_placer_place_strands(_handles[device_index], bytes.get(), offsets.get(), n, (uint32_t)_strand,
                                           rows.get(), n_rows.get(), counts.get(), strands.get());
    } else {
        rc = _sharded ? epik_amd_placer_place_sharded(_handles.data(), (uint32_t)_handles.size(), bytes.get(),
                                                      offsets.get(), n, rows.get(), n_rows.get(), counts.get())
                      : epik_amd_placer_place(_handles[device_index], bytes.get(), offsets.get(), n, rows.get(),
                                              n_rows.get(), counts.get());
    }
    if (rc != EPIK_AMD_OK) throw std::runtime_error(std::string("GPU placer: ") + epik_amd_last_error());
    parallel_for(batches.size(), num_threads, [&](size_t b) {
        auto& pb = out[b];
        const size_t n_unique = pb.sequences.size();
        pb.row_begin.assign(n_unique + 1, 0);
        for (size_t u = 0; u < n_unique; ++u) {
            const size_t i = first_unique[b] + u;
            // (n_rows is a row count here: epik_amd_placer_place widens the counts by itself, so the
            // EPIK_AMD_ROWS_COUNTS_TOO_NARROW mark of the device entry points must never arrive)
            if (n_rows[i] > _keep_at_most)
                throw std::runtime_error("GPU placer: read " + std::to_string(i) + " came back with " +
                                         std::to_string(n_rows[i]) + " rows (keep_at_most " +
                                         std::to_string(_keep_at_most) + ")");
            pb.row_begin[u + 1] = pb.row_begin[u] + n_rows[i];
        }
        pb.rows.resize(pb.row_begin[n_unique]);
        if (strands) {
            pb.strands.assign(strands.get() + first_unique[b], strands.get() + first_unique[b] + n_unique);
        }
        if (frames) pb.frames.assign(frames.get() + first_unique[b], frames.get() + first_unique[b] + n_unique);
        if (conf) pb.confidence.assign(conf.get() + first_unique[b], conf.get() + first_unique[b] + n_unique);
        for (size_t u = 0; u < n_unique; ++u) {
            const size_t i = first_unique[b] + u;
            for (uint32_t r = 0; r < n_rows[i]; ++r) {
                const auto& row = rows[i * _keep_at_most + r];
                const size_t count = counts[i * _keep_at_most + r];
                // rows fabricated for a read without hits carry 0.0 lengths (place.cpp:150)
                double distal = 0.0, pendant = 0.0;
                if (count != 0) {
                    const auto node = _original_tree.get_by_postorder_id(row.branch);
                    if (!node)
                        throw std::runtime_error("Could not find node by post-order id: " + std::to_string(row.branch));
                    distal = (*node)->get_branch_length() / 2;  // place.cpp:435
                    pendant = _pendant_lengths[row.branch];
                }
                pb.rows[pb.row_begin[u] + r] = {row.branch, row.score, row.lwr, count, distal, pendant};
            }
        }
    });
    return out;
}

std::vector<placed_collection> placer::place_batches(const std::vector<const std::vector<seq_record>*>& batches,
                                                     size_t device_index, size_t num_threads)
{
    // the reference's containers (place.h:59-75), filled from the flat form
    auto flat = place_flat(batches, device_index, num_threads);
    std::vector<placed_collection> out(batches.size());
    parallel_for(batches.size(), num_threads, [&](size_t b) {
        const auto& pb = flat[b];
        out[b].sequence_map.reserve(pb.size());
        out[b].placed_seqs.reserve(pb.size());
        for (size_t u = 0; u < pb.size(); ++u) {
            out[b].sequence_map.emplace(pb.sequences[u], std::vector<std::string_view>(pb.names.begin() + pb.name_begin[u],
                                                                                       pb.names.begin() + pb.name_begin[u + 1]));
            out[b].placed_seqs.push_back({pb.sequences[u], std::vector<placement>(pb.rows.begin() + pb.row_begin[u],
                                                                                  pb.rows.begin() + pb.row_begin[u + 1])});
        }
    });
    return out;
}

}  // namespace epik_amd
