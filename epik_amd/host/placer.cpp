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
#pragma weak epik_amd_placer_paint_windows

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

placer::window_batch placer::paint_windows(const std::vector<seq_record>& records, size_t device_index, uint32_t window,
                                           uint32_t step, uint32_t strand_mode, const std::vector<uint32_t>& group, uint32_t tau_q,
                                           bool per_window)
{
    if (_sharded) throw std::runtime_error("GPU placer: --windows does not work with --db-shard > 1");
    if (!&epik_amd_placer_paint_windows) throw std::runtime_error("GPU placer: this libepik_amd has no windowed placement");
    if (group.size() != _original_tree.get_node_count()) throw std::runtime_error("GPU placer: the groups do not fit the tree");
    const uint64_t n = records.size();
    window_batch out;
    out.win_offsets.assign(n + 1, 0);
    std::vector<uint64_t> offsets(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t len = records[i].sequence().size();
        const uint64_t nw = epik_amd_window_span(len, window, step, 0, nullptr, nullptr);
        if (nw == 0) throw std::runtime_error("GPU placer: the window or its step is out of range");
        offsets[i + 1] = offsets[i] + len;
        out.win_offsets[i + 1] = out.win_offsets[i] + nw;
    }
    std::string bytes;
    bytes.reserve(offsets[n]);
    for (const auto& record : records) bytes.append(record.sequence());
    const uint64_t total = out.win_offsets[n];
    out.records.resize(total), out.segments.resize(total), out.n_segments.resize(n), out.strand.resize(total);
    std::vector<epik_amd_placement> rows;
    if (per_window) rows.resize(total * _keep_at_most), out.n_rows.resize(total);
    std::vector<uint64_t> counted(n + 1, 0);
    if (epik_amd_placer_paint_windows(_handles.at(device_index), bytes.data(), offsets.data(), n, window, step, strand_mode, group.data(),
                                      tau_q, per_window ? rows.data() : nullptr, per_window ? out.n_rows.data() : nullptr, nullptr,
                                      out.strand.data(), counted.data(), out.records.data(), out.segments.data(),
                                      out.n_segments.data()) != EPIK_AMD_OK)
        throw std::runtime_error(std::string("GPU placer: ") + epik_amd_last_error());
    if (n && counted != out.win_offsets) throw std::runtime_error("GPU placer: the library counted other windows than the driver");
    if (per_window) {
        out.best.resize(total);
        for (uint64_t v = 0; v < total; ++v) out.best[v] = rows[v * _keep_at_most];
    }
    return out;
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

void placer::read_cohort(cohort_request& request)
{
    const uint32_t* const strata = request.strata;
    const uint32_t distance = request.distance;
    if (request.edgemodel && !&epik_amd_cohort_edgemodel_strata) throw std::runtime_error("GPU placer: this libepik_amd has no edge model");
    if ((request.mantel && !&epik_amd_cohort_mantel) || (request.anosim && !&epik_amd_cohort_anosim))
        throw std::runtime_error("GPU placer: this libepik_amd has no Mantel test or no ANOSIM");
    if (request.model && !&epik_amd_cohort_model_metric) throw std::runtime_error("GPU placer: this libepik_amd has no sequential model");
    if (strata && (request.permanova || request.permdisp || request.edgetest || request.model) &&
        (!&epik_amd_cohort_permanova_strata || !&epik_amd_cohort_permdisp_strata || !&epik_amd_cohort_edgetest_strata ||
         !&epik_amd_cohort_model_strata))
        throw std::runtime_error("GPU placer: this libepik_amd has no permutations within strata");
    if ((request.unifrac || distance != EPIK_AMD_DISTANCE_KR) && (!&epik_amd_cohort_unifrac || !&epik_amd_cohort_permanova_metric ||
                                                          !&epik_amd_cohort_pcoa_metric || !&epik_amd_cohort_permdisp_metric))
        throw std::runtime_error("GPU placer: this libepik_amd has no UniFrac distances");
    if (request.permdisp && !&epik_amd_cohort_permdisp) throw std::runtime_error("GPU placer: this libepik_amd has no PERMDISP");
    if (request.pcoa && !&epik_amd_cohort_pcoa) throw std::runtime_error("GPU placer: this libepik_amd has no principal coordinates");
    if (request.edgetest && !&epik_amd_cohort_edgetest) throw std::runtime_error("GPU placer: this libepik_amd has no edge test");
    if (request.permanova && !&epik_amd_cohort_permanova) throw std::runtime_error("GPU placer: this libepik_amd has no PERMANOVA");
    if ((request.correlation || request.dispersion) && (!&epik_amd_cohort_correlation || !&epik_amd_cohort_dispersion))
        throw std::runtime_error("GPU placer: this libepik_amd has no edge correlation and dispersion");
    if ((request.alpha || request.rarefy) && (!&epik_amd_cohort_alpha || !&epik_amd_cohort_rarefy))
        throw std::runtime_error("GPU placer: this libepik_amd has no alpha diversity and rarefaction");
    if (request.kmeans && !&epik_amd_cohort_kmeans) throw std::runtime_error("GPU placer: this libepik_amd has no phylogenetic k-means");
    if (request.squash && !&epik_amd_cohort_squash) throw std::runtime_error("GPU placer: this libepik_amd has no squash clustering");
    if (request.epca && !&epik_amd_cohort_epca) throw std::runtime_error("GPU placer: this libepik_amd has no edge principal components");
    const auto check = [](int rc) {
        if (rc != EPIK_AMD_OK) throw std::runtime_error(std::string("GPU placer: ") + epik_amd_last_error());
    };
    if (_cohorts.empty()) throw std::runtime_error("GPU placer: no cohort (set_cohort)");
    const size_t S = _cohort_samples, N = _original_tree.get_node_count();
    request.cells = sample_cohort((uint32_t)S, (uint32_t)N);
    request.kr.assign(S * S, 0.0);
    // integer adds: the sum is the same bits whichever handle placed which batch
    for (size_t g = 1; g < _cohorts.size(); ++g) {
        check(epik_amd_cohort_read(_cohorts[g], request.cells.mass.data(), request.cells.best.data(), request.cells.totals.data(), nullptr));
        check(epik_amd_cohort_add_cells(_cohorts[0], request.cells.mass.data(), request.cells.best.data(), request.cells.totals.data()));
        epik_amd_cohort_destroy(_cohorts[g]);  // (summed once: a second read_cohort finds it all in the first)
        _cohorts[g] = nullptr;
    }
    _cohorts.resize(1);
    uint64_t bad_samples = 0;
    check(epik_amd_cohort_read(_cohorts[0], request.cells.mass.data(), request.cells.best.data(), request.cells.totals.data(), &bad_samples));
    if (bad_samples) throw std::runtime_error("GPU placer: " + std::to_string(bad_samples) + " reads of no sample of the cohort");
    std::vector<uint32_t> parent;
    std::vector<double> length;
    for (const auto& node : _original_tree.nodes()) {
        parent.push_back(node.parent < 0 ? EPIK_AMD_TREE_NO_PARENT : (uint32_t)node.parent);
        length.push_back(node.branch_length);
    }
    epik_amd_tree* tree = nullptr;
    check(epik_amd_tree_create(_devices[0], parent.data(), length.data(), (uint32_t)parent.size(), &tree));
    epik_amd_cohort* const cohort = _cohorts[0];
    const double* const len = length.data();
    // the analyses in their fixed order; after the first that fails none runs.  Which entry serves a test -- the plain
    // one, _metric or _strata -- is part of what an older libepik_amd can still run: the newer ones only where needed
    int rc = epik_amd_cohort_kr(cohort, tree, len, request.kr.data());
    const auto run = [&](bool engaged, auto&& call) {
        if (rc == EPIK_AMD_OK && engaged) rc = call();
    };
    if (request.unifrac) request.unifrac->matrix.assign(request.unifrac->metrics.size(), std::vector<double>(S * S, 0.0));
    for (size_t i = 0; request.unifrac && i < request.unifrac->metrics.size(); ++i)
        run(true, [&] { return epik_amd_cohort_unifrac(cohort, tree, len, request.unifrac->metrics[i], request.unifrac->matrix[i].data()); });
    run(request.squash.has_value(), [&] {
        auto& t = *request.squash;
        t.merges.assign(S ? S - 1 : 0, epik_amd_squash_merge{});
        return epik_amd_cohort_squash(cohort, tree, len, t.merges.data(), &t.num_merges);
    });
    run(request.epca.has_value(), [&] {
        auto& t = *request.epca;
        const size_t K = t.num_components;
        t.mu.assign(K, 0.0), t.proj.assign(S * K, 0.0), t.edge.assign(K * N, 0.0);
        t.first.resize(N);
        for (size_t b = 0; b < N; ++b) t.first[b] = (uint32_t)b;  // (post-order ids: a parent comes after its children)
        for (size_t b = 0; b < N; ++b)
            if (parent[b] != EPIK_AMD_TREE_NO_PARENT && parent[b] < N) t.first[parent[b]] = std::min(t.first[parent[b]], t.first[b]);
        return epik_amd_cohort_epca(cohort, tree, t.num_components, t.mu.data(), t.proj.data(), t.edge.data(), &t.info);
    });
    run(request.kmeans.has_value(), [&] {
        auto& t = *request.kmeans;
        const size_t K = t.num_clusters;
        t.samples.assign(S, epik_amd_kmeans_sample{}), t.clusters.assign(K, epik_amd_kmeans_cluster{}), t.centroids.assign(K * N, 0.0);
        return epik_amd_cohort_kmeans(cohort, tree, len, t.num_clusters, t.max_iterations, t.samples.data(), t.clusters.data(),
                                      t.centroids.data(), &t.info);
    });
    run(request.alpha.has_value(), [&] {
        request.alpha->alpha.assign(S, epik_amd_alpha{});
        return epik_amd_cohort_alpha(cohort, tree, len, request.alpha->alpha.data());
    });
    run(request.rarefy.has_value(), [&] {
        auto& t = *request.rarefy;
        t.curve.assign(S * t.num_depths * 2, 0.0);
        return epik_amd_cohort_rarefy(cohort, tree, len, t.depth_step, t.num_depths, t.curve.data());
    });
    run(request.correlation.has_value(), [&] {
        auto& t = *request.correlation;
        t.correlation.assign((size_t)t.num_columns * N, epik_amd_correlation{});
        t.used.assign(t.num_columns, 0);
        return epik_amd_cohort_correlation(cohort, tree, t.meta, t.num_columns, t.correlation.data(), t.used.data());
    });
    run(request.dispersion.has_value(), [&] {
        request.dispersion->dispersion.assign(N, epik_amd_dispersion{});
        return epik_amd_cohort_dispersion(cohort, tree, request.dispersion->dispersion.data());
    });
    run(request.permanova.has_value(), [&] {
        auto& t = *request.permanova;
        t.records.assign(t.num_columns * (1 + (t.pairwise ? (size_t)EPIK_AMD_PERMANOVA_PAIR_SLOTS : 0)), epik_amd_permanova{});
        t.group_ss.assign((size_t)t.num_columns * EPIK_AMD_PERMANOVA_MAX_GROUPS, 0.0);
        return strata ? epik_amd_cohort_permanova_strata(cohort, tree, len, distance, t.labels, t.num_columns, t.num_permutations, t.seed,
                                                         t.pairwise ? 1 : 0, t.records.data(), nullptr, t.group_ss.data(), strata)
               : distance != EPIK_AMD_DISTANCE_KR
                   ? epik_amd_cohort_permanova_metric(cohort, tree, len, distance, t.labels, t.num_columns, t.num_permutations, t.seed,
                                                      t.pairwise ? 1 : 0, t.records.data(), nullptr, t.group_ss.data())
                   : epik_amd_cohort_permanova(cohort, tree, len, t.labels, t.num_columns, t.num_permutations, t.seed, t.pairwise ? 1 : 0,
                                               t.records.data(), nullptr, t.group_ss.data());
    });
    run(request.edgetest.has_value(), [&] {
        auto& t = *request.edgetest;
        t.records.assign((size_t)t.num_columns * N, epik_amd_edgetest{});
        return strata ? epik_amd_cohort_edgetest_strata(cohort, tree, t.labels, t.num_columns, t.num_permutations, t.seed, t.records.data(),
                                                        nullptr, nullptr, strata)
                      : epik_amd_cohort_edgetest(cohort, tree, t.labels, t.num_columns, t.num_permutations, t.seed, t.records.data(),
                                                 nullptr, nullptr);
    });
    run(request.pcoa.has_value(), [&] {
        auto& t = *request.pcoa;
        t.mu.assign(S, 0.0), t.coord.assign(S * t.num_components, 0.0);
        return distance != EPIK_AMD_DISTANCE_KR
                   ? epik_amd_cohort_pcoa_metric(cohort, tree, len, distance, t.num_components, t.mu.data(), t.coord.data(), &t.info)
                   : epik_amd_cohort_pcoa(cohort, tree, len, t.num_components, t.mu.data(), t.coord.data(), &t.info);
    });
    run(request.permdisp.has_value(), [&] {
        auto& t = *request.permdisp;
        t.records.assign(t.num_columns * (1 + (t.pairwise ? (size_t)EPIK_AMD_PERMDISP_PAIR_SLOTS : 0)), epik_amd_permdisp{});
        t.group_mean.assign((size_t)t.num_columns * EPIK_AMD_PERMDISP_MAX_GROUPS, 0.0);
        t.z.assign((size_t)t.num_columns * S, 0.0);
        return strata ? epik_amd_cohort_permdisp_strata(cohort, tree, len, distance, t.labels, t.num_columns, t.num_permutations, t.seed,
                                                        t.pairwise ? 1 : 0, t.records.data(), nullptr, t.group_mean.data(), t.z.data(),
                                                        strata)
               : distance != EPIK_AMD_DISTANCE_KR
                   ? epik_amd_cohort_permdisp_metric(cohort, tree, len, distance, t.labels, t.num_columns, t.num_permutations, t.seed,
                                                     t.pairwise ? 1 : 0, t.records.data(), nullptr, t.group_mean.data(), t.z.data())
                   : epik_amd_cohort_permdisp(cohort, tree, len, t.labels, t.num_columns, t.num_permutations, t.seed, t.pairwise ? 1 : 0,
                                              t.records.data(), nullptr, t.group_mean.data(), t.z.data());
    });
    run(request.model.has_value(), [&] {
        auto& t = *request.model;
        t.records.assign((size_t)t.num_terms + 1, epik_amd_model_term{});
        t.aliased.assign(EPIK_AMD_MODEL_MAX_COLUMNS, 0);
        return strata ? epik_amd_cohort_model_strata(cohort, tree, len, distance, t.kind, t.labels, t.values, t.num_terms, t.num_permutations,
                                                     t.seed, t.records.data(), &t.info, nullptr, t.aliased.data(), strata)
                      : epik_amd_cohort_model_metric(cohort, tree, len, distance, t.kind, t.labels, t.values, t.num_terms, t.num_permutations,
                                                     t.seed, t.records.data(), &t.info, nullptr, t.aliased.data());
    });
    run(request.edgemodel.has_value(), [&] {
        auto& t = *request.edgemodel;
        t.records.assign((size_t)t.num_terms * N, epik_amd_edgemodel{});
        t.aliased.assign(EPIK_AMD_MODEL_MAX_COLUMNS, 0);
        return epik_amd_cohort_edgemodel_strata(cohort, tree, t.kind, t.labels, t.values, t.num_terms, t.num_permutations, t.seed,
                                                t.records.data(), &t.info, nullptr, nullptr, t.aliased.data(), strata);
    });
    run(request.mantel.has_value(), [&] {
        auto& t = *request.mantel;
        const size_t per_side = (t.methods & 1u) + (t.methods >> 1 & 1u);
        t.records.assign(((size_t)t.num_columns + t.num_matrices) * per_side, epik_amd_mantel{});
        return epik_amd_cohort_mantel(cohort, tree, len, distance, t.values, t.num_columns, t.matrices, t.present, t.num_matrices, t.methods,
                                      t.control, t.num_permutations, t.seed, strata, t.records.data(), nullptr);
    });
    run(request.anosim.has_value(), [&] {
        auto& t = *request.anosim;
        t.records.assign(t.num_columns, epik_amd_anosim{});
        return epik_amd_cohort_anosim(cohort, tree, len, distance, t.labels, t.num_columns, t.num_permutations, t.seed, strata,
                                      t.records.data(), nullptr);
    });
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
