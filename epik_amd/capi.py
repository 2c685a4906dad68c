"""ctypes binding of libepik_amd.so -- the C-ABI declared in include/epik_amd.h.

This is the same stub a maintainer of another host language would write (see
INTEGRATION.md).  The library is built in-tree by `__graft_entry__.build()` /
`make -C epik_amd/csrc`.  Loading fails loudly when it is missing: there is no
Python or CPU fallback for the placement path.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EPIK_AMD_LIB") or os.path.join(_HERE, "libepik_amd.so")

ABI_VERSION = 3

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED = 0, 1, 2, 3, 4

#: numpy mirror of `epik_amd_placement` {branch, score, lwr} (16 bytes)
PLACEMENT = np.dtype([("branch", np.uint32), ("score", np.float32), ("lwr", np.float64)])
#: numpy mirror of `epik_amd_confidence` {clade, clade_mass_q, edpl} (16 bytes)
CONFIDENCE = np.dtype([("clade", np.uint32), ("clade_mass_q", np.uint32), ("edpl", np.float64)])
#: numpy mirror of `epik_amd_taxon_record` {taxon, taxon_mass_q, first_taxon, total_q} (16 bytes)
TAXON_RECORD = np.dtype([("taxon", np.uint32), ("taxon_mass_q", np.uint32), ("first_taxon", np.uint32), ("total_q", np.uint32)])
#: numpy mirrors of `epik_amd_window_record` (16 bytes) and `epik_amd_window_segment` (32 bytes)
WINDOW_RECORD = np.dtype([("call", np.uint32), ("call_mass_q", np.uint32), ("first_group", np.uint32), ("total_q", np.uint32)])
WINDOW_SEGMENT = np.dtype([("call", np.uint32), ("first_window", np.uint32), ("num_windows", np.uint32), ("reserved", np.uint32),
                           ("call_mass", np.uint64), ("total", np.uint64)])
#: numpy mirror of `epik_amd_taxa_totals` (48 bytes)
TAXA_TOTALS = np.dtype([(name, np.uint64) for name in ("placed", "no_hit", "too_short", "too_narrow", "no_mass", "bad_reads")])
#: epik_amd_squash_merge (32 bytes)
SQUASH_MERGE = np.dtype([("a", np.uint32), ("b", np.uint32), ("dist", np.float64), ("len_a", np.float64), ("len_b", np.float64)])
SQUASH_NONE = 0xFFFFFFFF
#: epik_amd_epca_info (32 bytes)
EPCA_INFO = np.dtype([("used", np.uint32), ("components", np.uint32), ("sweeps", np.uint32), ("converged", np.uint32),
                      ("trace", np.float64), ("scale", np.float64)])
EPCA_MAX_COMPONENTS = 64
#: epik_amd_pcoa_info (48 bytes)
PCOA_INFO = np.dtype([("used", np.uint32), ("components", np.uint32), ("sweeps", np.uint32), ("converged", np.uint32),
                      ("trace", np.float64), ("scale", np.float64), ("pos", np.float64), ("neg", np.float64)])
PCOA_MAX_COMPONENTS = 64
EPCA_MAX_SWEEPS = 64
#: epik_amd_kmeans_info (16 bytes), epik_amd_kmeans_sample (16 bytes), epik_amd_kmeans_cluster (24 bytes)
KMEANS_INFO = np.dtype([("used", np.uint32), ("clusters", np.uint32), ("iterations", np.uint32), ("converged", np.uint32)])
KMEANS_SAMPLE = np.dtype([("cluster", np.uint32), ("zero", np.uint32), ("dist", np.float64)])
KMEANS_CLUSTER = np.dtype([("size", np.uint32), ("seed", np.uint32), ("sum_dist", np.float64), ("sum_sq", np.float64)])
KMEANS_MAX_CLUSTERS = 64
KMEANS_MAX_ITERATIONS = 1000
KMEANS_NONE = 0xFFFFFFFF
#: epik_amd_alpha (40 bytes): the five alpha diversity indices of a sample
ALPHA = np.dtype([("pd", np.float64), ("rooted_pd", np.float64), ("bwpd_half", np.float64), ("bwpd_one", np.float64),
                  ("quadratic", np.float64)])
DIVERSITY_BLOCK = 256
#: epik_amd_correlation (32 bytes) and epik_amd_dispersion (64 bytes): a branch's records; NA is the bit pattern NA_BITS
CORRELATION = np.dtype([("mass_pearson", np.float64), ("mass_spearman", np.float64), ("imbalance_pearson", np.float64),
                        ("imbalance_spearman", np.float64)])
DISPERSION = np.dtype([("mass_mean", np.float64), ("mass_var", np.float64), ("mass_sd", np.float64), ("mass_cv", np.float64),
                       ("mass_vmr", np.float64), ("imbalance_mean", np.float64), ("imbalance_var", np.float64),
                       ("imbalance_sd", np.float64)])
CORRELATION_MAX_COLUMNS = 64
#: epik_amd_permanova (56 bytes): a test's record; the doubles of an undefined test are NA_BITS
PERMANOVA = np.dtype([("used", np.uint32), ("groups", np.uint32), ("at_most", np.uint64), ("ss_total", np.float64),
                      ("ss_within", np.float64), ("f", np.float64), ("r2", np.float64), ("p", np.float64)])
PERMANOVA_MAX_COLUMNS = 64
PERMANOVA_MAX_GROUPS = 256
PERMANOVA_MAX_PAIR_GROUPS = 32
PERMANOVA_PAIR_SLOTS = 496
PERMANOVA_MAX_PERMUTATIONS = 999999
PERMANOVA_MISSING = 0xFFFFFFFF
#: epik_amd_permdisp (48 bytes): a test's record; the doubles of an undefined test are NA_BITS
PERMDISP = np.dtype([("used", np.uint32), ("groups", np.uint32), ("clipped", np.uint32), ("pad", np.uint32),
                     ("at_least", np.uint64), ("eta2", np.float64), ("f", np.float64), ("p", np.float64)])
PERMDISP_MAX_COLUMNS = 64
PERMDISP_MAX_GROUPS = 32
PERMDISP_PAIR_SLOTS = 496
PERMDISP_MAX_PERMUTATIONS = 999999
PERMDISP_MISSING = 0xFFFFFFFF
#: epik_amd_mantel (64 bytes) and epik_amd_anosim (48 bytes): a test's record; the doubles of an undefined test are NA_BITS
MANTEL = np.dtype([("used", np.uint32), ("side", np.uint32), ("method", np.uint32), ("partial", np.uint32),
                   ("at_least", np.uint64), ("r", np.float64), ("r_xz", np.float64), ("r_yz", np.float64),
                   ("stat", np.float64), ("p", np.float64)])
ANOSIM = np.dtype([("used", np.uint32), ("groups", np.uint32), ("at_least", np.uint64), ("r", np.float64),
                   ("mean_between", np.float64), ("mean_within", np.float64), ("p", np.float64)])
MANTEL_MAX_SAMPLES = 8192
MANTEL_MAX_COLUMNS = 64
MANTEL_MAX_MATRICES = 8
MANTEL_METHODS = {"pearson": 1, "spearman": 2}
MANTEL_NO_CONTROL = 0xFFFFFFFF
#: epik_amd_edgetest_family (48 bytes) and epik_amd_edgetest (208 bytes): a (column, branch)'s record of the edge test; the
#: families are mass, rank(mass), imbalance, rank(imbalance); the doubles of an undefined family are NA_BITS
EDGETEST_FAMILY = np.dtype([("eta2", np.float64), ("stat", np.float64), ("p", np.float64), ("p_adj", np.float64),
                            ("at_least", np.uint64), ("max_at_least", np.uint64)])
EDGETEST = np.dtype([("used", np.uint32), ("groups", np.uint32), ("family", EDGETEST_FAMILY, (4,)), ("top_mass", np.uint32),
                     ("top_imbalance", np.uint32)])
EDGETEST_MAX_COLUMNS = 64
EDGETEST_MAX_GROUPS = 32
EDGETEST_FAMILIES = 4
EDGETEST_MAX_PERMUTATIONS = 999999
EDGETEST_MISSING = 0xFFFFFFFF
#: epik_amd_model_term (48 bytes) and epik_amd_model_info (40 bytes): a term's record of the sequential model (the whole
#: model's is the last) and the info block; the doubles of an undefined record are NA_BITS
MODEL_TERM = np.dtype([("df", np.uint32), ("columns", np.uint32), ("at_least", np.uint64), ("ss", np.float64), ("f", np.float64),
                       ("r2", np.float64), ("p", np.float64)])
MODEL_INFO = np.dtype([("used", np.uint32), ("terms", np.uint32), ("columns", np.uint32), ("rank", np.uint32),
                       ("df_res", np.int64), ("ss_total", np.float64), ("ss_res", np.float64)])
MODEL_MAX_TERMS = 16
MODEL_MAX_COLUMNS = 64
MODEL_MAX_GROUPS = 32
MODEL_MAX_PERMUTATIONS = 999999
MODEL_MISSING = 0xFFFFFFFF
#: epik_amd_edgemodel_family (72 bytes), epik_amd_edgemodel (144 bytes) and epik_amd_edgemodel_info (152 bytes): a (term,
#: branch)'s record of the edge model, the families mass and imbalance, and the info block; the doubles of an undefined family
#: are NA_BITS
EDGEMODEL_FAMILY = np.dtype([("ss", np.float64), ("r2", np.float64), ("partial_r2", np.float64), ("f", np.float64),
                             ("p", np.float64), ("p_adj", np.float64), ("at_least", np.uint64), ("max_at_least", np.uint64),
                             ("sign", np.int32), ("pad", np.uint32)])
EDGEMODEL = np.dtype([("family", EDGEMODEL_FAMILY, (2,))])
EDGEMODEL_INFO = np.dtype([("used", np.uint32), ("terms", np.uint32), ("columns", np.uint32), ("rank", np.uint32),
                           ("df_res", np.int64), ("df", np.uint32, (16,)), ("term_columns", np.uint32, (16,))])
EDGEMODEL_FAMILIES = 2
NA_BITS = 0x7FF8000000000000
RAREFY_MAX_DEPTHS = 256
RAREFY_MAX_DEPTH = 1 << 20
#: numpy mirror of `epik_amd_pkdb_value` / `i2l::pkdb_value` (8 bytes)
PKDB_VALUE = np.dtype([("branch", np.uint32), ("score", np.float32)])

#: every symbol include/epik_amd.h declares
EXPORTS = (
    "epik_amd_device_count",
    "epik_amd_last_error",
    "epik_amd_placer_create",
    "epik_amd_placer_plan",
    "epik_amd_placer_plan_sizes",
    "epik_amd_placer_build_image",
    "epik_amd_placer_plan_run_counts",
    "epik_amd_placer_run_counts",
    "epik_amd_placer_ring_form",
    "epik_amd_placer_table_form",
    "epik_amd_placer_tail_form",
    "epik_amd_placer_destroy",
    "epik_amd_placer_place",
    "epik_amd_placer_place_device",
    "epik_amd_placer_algorithmic_bytes",
    "epik_amd_placer_create_sharded",
    "epik_amd_placer_accumulate_device",
    "epik_amd_placer_finish_device",
    "epik_amd_placer_partial_info",
    "epik_amd_placer_accumulate_lists_device",
    "epik_amd_placer_finish_lists_device",
    "epik_amd_placer_last_path",
    "epik_amd_placer_stream_build",
    "epik_amd_placer_place_sharded",
    "epik_amd_placer_release_scratch",
    "epik_amd_placer_set_wide_counts",
    "epik_amd_placer_choose_counts",
    "epik_amd_placer_launch_info",
    "epik_amd_placer_set_timing",
    "epik_amd_placer_last_kernel_ms",
    "epik_amd_placer_strand_workspace_bytes",
    "epik_amd_placer_place_strands_device",
    "epik_amd_placer_place_strands",
    "epik_amd_placer_mates_separator",
    "epik_amd_placer_mates_workspace_bytes",
    "epik_amd_placer_place_mates_device",
    "epik_amd_placer_place_mates",
    "epik_amd_codon_table",
    "epik_amd_placer_frame_workspace_bytes",
    "epik_amd_placer_place_frames_device",
    "epik_amd_placer_place_frames",
    "epik_amd_profile_create",
    "epik_amd_profile_destroy",
    "epik_amd_profile_reset",
    "epik_amd_profile_read",
    "epik_amd_profile_info",
    "epik_amd_profile_add_device",
    "epik_amd_placer_profile_reads",
    "epik_amd_placer_profile_strands",
    "epik_amd_placer_profile_frames",
    "epik_amd_placer_profile_mates",
    "epik_amd_tree_create",
    "epik_amd_tree_destroy",
    "epik_amd_tree_info",
    "epik_amd_tree_build_host",
    "epik_amd_tree_lca_host",
    "epik_amd_confidence_device",
    "epik_amd_placer_confidence_reads",
    "epik_amd_placer_confidence_strands",
    "epik_amd_placer_confidence_frames",
    "epik_amd_placer_confidence_mates",
    "epik_amd_cohort_create",
    "epik_amd_cohort_destroy",
    "epik_amd_cohort_reset",
    "epik_amd_cohort_info",
    "epik_amd_cohort_read",
    "epik_amd_cohort_add_cells",
    "epik_amd_cohort_add_device",
    "epik_amd_cohort_kr_device",
    "epik_amd_cohort_kr",
    "epik_amd_cohort_kr_host",
    "epik_amd_cohort_unifrac_device",
    "epik_amd_cohort_unifrac",
    "epik_amd_cohort_unifrac_host",
    "epik_amd_cohort_squash_device",
    "epik_amd_cohort_squash",
    "epik_amd_cohort_squash_host",
    "epik_amd_cohort_epca_device",
    "epik_amd_cohort_epca",
    "epik_amd_cohort_epca_host",
    "epik_amd_cohort_kmeans_device",
    "epik_amd_cohort_kmeans",
    "epik_amd_cohort_kmeans_host",
    "epik_amd_cohort_alpha_device",
    "epik_amd_cohort_alpha",
    "epik_amd_cohort_alpha_host",
    "epik_amd_cohort_rarefy_device",
    "epik_amd_cohort_rarefy",
    "epik_amd_cohort_rarefy_host",
    "epik_amd_cohort_correlation_device",
    "epik_amd_cohort_correlation",
    "epik_amd_cohort_correlation_host",
    "epik_amd_cohort_dispersion_device",
    "epik_amd_cohort_dispersion",
    "epik_amd_cohort_dispersion_host",
    "epik_amd_cohort_permanova_device",
    "epik_amd_cohort_permanova",
    "epik_amd_cohort_permanova_host",
    "epik_amd_cohort_permanova_metric",
    "epik_amd_cohort_permanova_metric_host",
    "epik_amd_cohort_permanova_kr_host",
    "epik_amd_cohort_model_device",
    "epik_amd_cohort_model",
    "epik_amd_cohort_model_metric",
    "epik_amd_cohort_model_host",
    "epik_amd_cohort_model_metric_host",
    "epik_amd_cohort_model_kr_host",
    "epik_amd_cohort_pcoa_device",
    "epik_amd_cohort_pcoa",
    "epik_amd_cohort_pcoa_host",
    "epik_amd_cohort_pcoa_metric",
    "epik_amd_cohort_pcoa_metric_host",
    "epik_amd_cohort_pcoa_kr_host",
    "epik_amd_cohort_edgetest_device",
    "epik_amd_cohort_edgetest",
    "epik_amd_cohort_edgetest_host",
    "epik_amd_cohort_permdisp_device",
    "epik_amd_cohort_permdisp",
    "epik_amd_cohort_permdisp_host",
    "epik_amd_cohort_permdisp_metric",
    "epik_amd_cohort_permdisp_metric_host",
    "epik_amd_cohort_permdisp_kr_host",
    "epik_amd_cohort_permanova_strata_device",
    "epik_amd_cohort_permanova_strata",
    "epik_amd_cohort_permanova_strata_host",
    "epik_amd_cohort_permanova_strata_kr_host",
    "epik_amd_cohort_permdisp_strata_device",
    "epik_amd_cohort_permdisp_strata",
    "epik_amd_cohort_permdisp_strata_host",
    "epik_amd_cohort_permdisp_strata_kr_host",
    "epik_amd_cohort_model_strata_device",
    "epik_amd_cohort_model_strata",
    "epik_amd_cohort_model_strata_host",
    "epik_amd_cohort_model_strata_kr_host",
    "epik_amd_cohort_edgemodel_device",
    "epik_amd_cohort_edgemodel",
    "epik_amd_cohort_edgemodel_host",
    "epik_amd_cohort_edgemodel_strata_device",
    "epik_amd_cohort_edgemodel_strata",
    "epik_amd_cohort_edgemodel_strata_host",
    "epik_amd_cohort_edgetest_strata_device",
    "epik_amd_cohort_edgetest_strata",
    "epik_amd_cohort_edgetest_strata_host",
    "epik_amd_cohort_mantel_device",
    "epik_amd_cohort_mantel",
    "epik_amd_cohort_mantel_host",
    "epik_amd_cohort_mantel_kr_host",
    "epik_amd_cohort_anosim_device",
    "epik_amd_cohort_anosim",
    "epik_amd_cohort_anosim_host",
    "epik_amd_cohort_anosim_kr_host",
    "epik_amd_placer_cohort_reads",
    "epik_amd_placer_cohort_strands",
    "epik_amd_placer_cohort_frames",
    "epik_amd_placer_cohort_mates",
    "epik_amd_taxonomy_create",
    "epik_amd_taxonomy_destroy",
    "epik_amd_taxonomy_reset",
    "epik_amd_taxonomy_info",
    "epik_amd_taxonomy_read",
    "epik_amd_taxonomy_add_cells",
    "epik_amd_taxonomy_add_device",
    "epik_amd_taxonomy_assign_host",
    "epik_amd_placer_taxa_reads",
    "epik_amd_placer_taxa_strands",
    "epik_amd_placer_taxa_frames",
    "epik_amd_placer_taxa_mates",
    "epik_amd_window_span",
    "epik_amd_placer_window_workspace_bytes",
    "epik_amd_placer_place_windows_device",
    "epik_amd_placer_place_windows",
    "epik_amd_placer_paint_windows",
    "epik_amd_windows_paint_device",
    "epik_amd_windows_paint_host",
    "epik_amd_builder_create",
    "epik_amd_builder_add",
    "epik_amd_builder_add_device",
    "epik_amd_builder_finish",
    "epik_amd_builder_copy",
    "epik_amd_builder_destroy",
    "epik_amd_build_host",
    "epik_amd_ancestral_create",
    "epik_amd_ancestral_posteriors",
    "epik_amd_ancestral_posteriors_device",
    "epik_amd_ancestral_destroy",
    "epik_amd_ancestral_host",
    "epik_amd_model_pmatrices",
    "epik_amd_model_gamma_rates",
    "epik_amd_filter_rank_device",
    "epik_amd_filter_rank",
    "epik_amd_builder_rank",
    "epik_amd_filter_rank_host",
    "epik_amd_filter_math_host",
)


class AncestralDesc(ctypes.Structure):
    """`epik_amd_ancestral_desc`."""

    _fields_ = [
        ("num_nodes", ctypes.c_uint32),
        ("sigma", ctypes.c_uint32),
        ("num_categories", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("parent", ctypes.c_void_p),
        ("weights", ctypes.c_void_p),
        ("pi", ctypes.c_void_p),
        ("p_full", ctypes.c_void_p),
        ("p_half", ctypes.c_void_p),
        ("p_pend", ctypes.c_void_p),
    ]


class PlacerDesc(ctypes.Structure):
    """`epik_amd_placer_desc`."""

    _fields_ = [
        ("abi_version", ctypes.c_uint32),
        ("kmer_size", ctypes.c_uint32),
        ("alphabet_size", ctypes.c_uint32),
        ("num_branches", ctypes.c_uint32),
        ("keep_at_most", ctypes.c_uint32),
        ("offset_bits", ctypes.c_uint32),
        ("keep_factor", ctypes.c_double),
        ("threshold", ctypes.c_float),
        ("log_threshold", ctypes.c_float),
        ("num_keys", ctypes.c_uint64),
        ("num_entries", ctypes.c_uint64),
        ("offsets", ctypes.c_void_p),
        ("values", ctypes.c_void_p),
        ("char_class", ctypes.c_void_p),
        ("device", ctypes.c_int32),
        ("shard", ctypes.c_uint32),
        ("keys", ctypes.c_void_p),
        ("num_present", ctypes.c_uint64),
    ]


class Plan(ctypes.Structure):
    """`epik_amd_plan`."""

    _fields_ = [
        ("kernel", ctypes.c_uint32),
        ("layout", ctypes.c_uint32),
        ("team_waves", ctypes.c_uint32),
        ("team_passes", ctypes.c_uint32),
        ("slice_rows", ctypes.c_uint32),
        ("resident_waves", ctypes.c_uint32 * 3),
        ("table_bytes", ctypes.c_uint64),
        ("filter_bytes", ctypes.c_uint64),
        ("posting_bytes", ctypes.c_uint64),
        ("kept_entries", ctypes.c_uint64),
        ("run_coded", ctypes.c_uint32),
        ("posting_bytes_is_bound", ctypes.c_uint32),
    ]


class ListBin(ctypes.Structure):
    """`epik_amd_list_bin`."""

    _fields_ = [("length", ctypes.c_uint64), ("lists", ctypes.c_uint64), ("lists_in_runs", ctypes.c_uint64)]


class PartialInfo(ctypes.Structure):
    """`epik_amd_partial_info`."""

    _fields_ = [
        ("lists", ctypes.c_uint32),
        ("slices", ctypes.c_uint32),
        ("slice_rows", ctypes.c_uint32),
        ("entry_bytes", ctypes.c_uint32),
        ("num_branches", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("postings_per_kmer", ctypes.c_double),
    ]


class ProfileTotals(ctypes.Structure):
    """`epik_amd_profile_totals`."""

    _fields_ = [("placed", ctypes.c_uint64), ("no_hit", ctypes.c_uint64), ("too_short", ctypes.c_uint64),
                ("too_narrow", ctypes.c_uint64), ("bad_rows", ctypes.c_uint64)]


#: fixed point of the like-weight ratios a profile sums (EPIK_AMD_PROFILE_LWR_BITS)
PROFILE_LWR_BITS = 30
MAX_SHARDS = 16
#: count of a partial list that found no room in d_entries
LIST_OVERFLOW = 0xFFFFFFFF
PATH_WAVE, PATH_TEAM_ONE_KERNEL, PATH_TEAM_STREAMED = 0, 1, 2

#: parent of the root in epik_amd_tree_create, and the clades of the reads that get none (EPIK_AMD_CLADE_*)
TREE_NO_PARENT = 0xFFFFFFFF
CLADE_TOO_NARROW, CLADE_TOO_SHORT, CLADE_NO_HIT, CLADE_BAD_ROW = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
CLADE_CLASSES = {CLADE_TOO_NARROW: "too_narrow", CLADE_TOO_SHORT: "too_short", CLADE_NO_HIT: "no_hit", CLADE_BAD_ROW: "bad_row"}

#: the taxa of the reads that get none (EPIK_AMD_TAXON_*)
TAXON_TOO_NARROW, TAXON_TOO_SHORT, TAXON_NO_HIT, TAXON_BAD_ROW, TAXON_NO_MASS = (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC,
                                                                                 0xFFFFFFFB)
TAXON_CLASSES = {TAXON_TOO_NARROW: "too_narrow", TAXON_TOO_SHORT: "too_short", TAXON_NO_HIT: "no_hit", TAXON_BAD_ROW: "bad_row",
                 TAXON_NO_MASS: "no_mass"}

#: painting by windows (EPIK_AMD_WINDOW_*): the group of a branch above the groups, the most windows a read may have, and
#: the calls of the windows that get no group
WINDOW_NO_GROUP, WINDOW_MAX_PER_READ = 0xFFFFFFFF, 1 << 24
WINDOW_TOO_NARROW, WINDOW_TOO_SHORT, WINDOW_NO_HIT, WINDOW_BAD_ROW, WINDOW_NO_MASS, WINDOW_AMBIGUOUS = (
    0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC, 0xFFFFFFFB, 0xFFFFFFFA)
WINDOW_CLASSES = {WINDOW_TOO_NARROW: "too_narrow", WINDOW_TOO_SHORT: "too_short", WINDOW_NO_HIT: "no_hit",
                  WINDOW_BAD_ROW: "bad_row", WINDOW_NO_MASS: "no_mass", WINDOW_AMBIGUOUS: "ambiguous"}

#: strand modes of epik_amd_placer_place_strands[_device], and their names in Placer / epik.py / epik-dna --strand
STRAND_FORWARD, STRAND_REVERSE, STRAND_BOTH = 0, 1, 2
STRANDS = {"forward": STRAND_FORWARD, "reverse": STRAND_REVERSE, "both": STRAND_BOTH}

#: orientation of the mates of a pair (epik_amd_placer_place_mates[_device]): FR, the default (mate 2 arrives as the
#: reverse complement of the fragment's far end: Illumina paired-end), or FF, or-ed into the strand mode
MATES_FF = 0x100
MATE_ORIENTATIONS = {"fr": 0, "ff": MATES_FF}

#: frame modes of epik_amd_placer_place_frames[_device] (+1 +2 +3 / -1 -2 -3 / all six), their names in Placer /
#: epik.py / epik-aa --translate, and the names of the frame bytes 0..5
FRAMES_FORWARD, FRAMES_REVERSE, FRAMES_BOTH = 0, 1, 2
FRAME_MODES = {"forward": FRAMES_FORWARD, "reverse": FRAMES_REVERSE, "both": FRAMES_BOTH}
FRAME_NAMES = ("+1", "+2", "+3", "-1", "-2", "-3")

#: n_rows of a read with more k-mers than the counts of a device-pointer launch hold
ROWS_COUNTS_TOO_NARROW = 0xFFFFFFFF
TAIL_WAVE, TAIL_KERNEL = 0, 1   # epik_amd_placer_tail_form


class EpikAmdError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libepik_amd error {code}: {message}")
        self.code = code


_lib = None


def hip_runtimes(maps_text: str | None = None) -> list:
    """The HIP runtimes (libamdhip64) mapped into this process, from /proc/self/maps (or `maps_text`)."""
    import re
    if maps_text is None:
        try:
            with open("/proc/self/maps") as fh:
                maps_text = fh.read()
        except OSError:
            return []
    found = {os.path.realpath(m.group(1)) for m in re.finditer(r"(/\S*libamdhip64\S*)", maps_text)}
    return sorted(found)


def check_hip_runtime(runtimes: list | None = None) -> None:
    """libepik_amd.so links the system's HIP runtime by SONAME; PyTorch-ROCm ships one of its own.  When torch is
    imported FIRST its runtime satisfies the SONAME and the process holds one runtime (what bench.py, the tests and
    every caller that hands torch tensors to this library do).  The other way round the process ends up with TWO
    runtimes -- two device contexts, and torch reports "No HIP GPUs" at some later point.  Said here, by name."""
    runtimes = hip_runtimes() if runtimes is None else runtimes
    if len(runtimes) > 1:
        raise ImportError(
            "two HIP runtimes are mapped into this process (" + ", ".join(runtimes) + "): libepik_amd.so was loaded "
            "before torch, whose own libamdhip64 then came on top of the system's.  Import torch BEFORE epik_amd.capi.load() "
            "(`import torch` at the top of the program), or use a torch built against the system's ROCm.")


def load() -> ctypes.CDLL:
    """Loads libepik_amd.so (once) and declares the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C epik_amd/csrc` (hipcc, gfx950).  epik_amd has no CPU fallback.")
    if not os.environ.get("EPIK_AMD_LIB"):  # (a library named by hand is the caller's: tools/ablate.py variants)
        from . import provenance
        provenance.check_library()  # no record of a passed ISA lint: refused
    lib = ctypes.CDLL(LIB_PATH)
    check_hip_runtime()
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    lib.epik_amd_device_count.restype = i32
    lib.epik_amd_device_count.argtypes = []
    lib.epik_amd_last_error.restype = ctypes.c_char_p
    lib.epik_amd_last_error.argtypes = []
    lib.epik_amd_placer_create.restype = i32
    lib.epik_amd_placer_create.argtypes = [ctypes.POINTER(PlacerDesc), ctypes.POINTER(vp)]
    lib.epik_amd_placer_create_sharded.restype = i32
    lib.epik_amd_placer_create_sharded.argtypes = [ctypes.POINTER(PlacerDesc), ctypes.c_uint32, ctypes.c_uint32,
                                                   ctypes.POINTER(vp)]
    lib.epik_amd_placer_accumulate_device.restype = i32
    lib.epik_amd_placer_accumulate_device.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, vp, vp]
    lib.epik_amd_placer_finish_device.restype = i32
    lib.epik_amd_placer_finish_device.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.epik_amd_placer_partial_info.restype = i32
    lib.epik_amd_placer_partial_info.argtypes = [vp, ctypes.POINTER(PartialInfo)]
    lib.epik_amd_placer_accumulate_lists_device.restype = i32
    lib.epik_amd_placer_accumulate_lists_device.argtypes = [vp, vp, vp, u64, ctypes.c_uint32, vp, u64, vp, vp, vp, vp, vp, vp]
    lib.epik_amd_placer_finish_lists_device.restype = i32
    lib.epik_amd_placer_finish_lists_device.argtypes = [vp, vp, u64, ctypes.c_uint32, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                                        vp, vp, vp, vp, vp, vp]
    lib.epik_amd_placer_place_sharded.restype = i32
    lib.epik_amd_placer_place_sharded.argtypes = [ctypes.POINTER(vp), ctypes.c_uint32, vp, vp, u64, vp, vp, vp]
    lib.epik_amd_placer_release_scratch.restype = i32
    lib.epik_amd_placer_release_scratch.argtypes = [vp]
    lib.epik_amd_placer_stream_build.restype = i32
    lib.epik_amd_placer_stream_build.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    lib.epik_amd_placer_last_path.restype = i32
    lib.epik_amd_placer_last_path.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
    lib.epik_amd_placer_plan.restype = i32
    lib.epik_amd_placer_plan.argtypes = [ctypes.POINTER(PlacerDesc), ctypes.c_uint32, ctypes.c_uint32, u64,
                                         ctypes.POINTER(Plan)]
    lib.epik_amd_placer_plan_sizes.restype = i32
    lib.epik_amd_placer_plan_sizes.argtypes = [ctypes.c_uint32] * 4 + [ctypes.POINTER(ListBin), u64, ctypes.c_uint32, ctypes.c_uint32,
                                               u64, ctypes.POINTER(Plan)]
    lib.epik_amd_placer_build_image.restype = i32
    lib.epik_amd_placer_build_image.argtypes = [ctypes.POINTER(PlacerDesc), ctypes.c_uint32, ctypes.c_uint32, u64,
                                                vp, vp, vp]
    lib.epik_amd_placer_plan_run_counts.restype = i32
    lib.epik_amd_placer_plan_run_counts.argtypes = [ctypes.POINTER(PlacerDesc), ctypes.c_uint32, ctypes.c_uint32, u64,
                                                    ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    lib.epik_amd_placer_run_counts.restype = i32
    lib.epik_amd_placer_run_counts.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    lib.epik_amd_placer_ring_form.restype = i32
    lib.epik_amd_placer_ring_form.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    lib.epik_amd_placer_table_form.restype = i32
    lib.epik_amd_placer_table_form.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
    if hasattr(lib, "epik_amd_placer_tail_form"):  # (an older library named by EPIK_AMD_LIB)
        lib.epik_amd_placer_tail_form.restype = i32
        lib.epik_amd_placer_tail_form.argtypes = [vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    lib.epik_amd_placer_destroy.restype = None
    lib.epik_amd_placer_destroy.argtypes = [vp]
    lib.epik_amd_placer_place.restype = i32
    lib.epik_amd_placer_place.argtypes = [vp, vp, vp, u64, vp, vp, vp]
    lib.epik_amd_placer_place_device.restype = i32
    lib.epik_amd_placer_place_device.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp]
    lib.epik_amd_placer_algorithmic_bytes.restype = i32
    lib.epik_amd_placer_algorithmic_bytes.argtypes = [vp, vp, vp, u64, vp, vp, ctypes.POINTER(u64)]
    lib.epik_amd_placer_launch_info.restype = i32
    lib.epik_amd_placer_launch_info.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32),
                                                ctypes.POINTER(ctypes.c_uint32),
                                                ctypes.POINTER(ctypes.c_uint32)]
    lib.epik_amd_placer_set_wide_counts.restype = i32
    lib.epik_amd_placer_set_wide_counts.argtypes = [vp, i32]
    lib.epik_amd_placer_choose_counts.restype = i32
    lib.epik_amd_placer_choose_counts.argtypes = [vp, u64]
    lib.epik_amd_placer_set_timing.restype = i32
    lib.epik_amd_placer_set_timing.argtypes = [vp, i32]
    lib.epik_amd_placer_last_kernel_ms.restype = i32
    lib.epik_amd_placer_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    lib.epik_amd_codon_table.restype = i32
    lib.epik_amd_codon_table.argtypes = [vp]
    # (strand and frame placement: the same prototypes)
    for names, argtypes in (
            (("epik_amd_placer_strand_workspace_bytes", "epik_amd_placer_frame_workspace_bytes"),
             [vp, u64, u64, ctypes.c_uint32, ctypes.POINTER(u64)]),
            (("epik_amd_placer_place_strands_device", "epik_amd_placer_place_frames_device"),
             [vp, vp, vp, u64, ctypes.c_uint32, vp, u64, vp, vp, vp, vp, vp]),
            (("epik_amd_placer_place_strands", "epik_amd_placer_place_frames"),
             [vp, vp, vp, u64, ctypes.c_uint32, vp, vp, vp, vp])):
        for name in names:
            getattr(lib, name).restype = i32
            getattr(lib, name).argtypes = argtypes
    # (mates: the strand placement's prototypes over pairs; the device entry is also told the characters of its batch)
    lib.epik_amd_placer_mates_separator.restype = i32
    lib.epik_amd_placer_mates_separator.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8)]
    lib.epik_amd_placer_mates_workspace_bytes.restype = i32
    lib.epik_amd_placer_mates_workspace_bytes.argtypes = [vp, u64, u64, ctypes.c_uint32, ctypes.POINTER(u64)]
    lib.epik_amd_placer_place_mates_device.restype = i32
    lib.epik_amd_placer_place_mates_device.argtypes = [vp, vp, vp, u64, u64, ctypes.c_uint32, vp, u64, vp, vp, vp, vp, vp]
    lib.epik_amd_placer_place_mates.restype = i32
    lib.epik_amd_placer_place_mates.argtypes = [vp, vp, vp, u64, ctypes.c_uint32, vp, vp, vp, vp]
    # (the abundance profile)
    lib.epik_amd_profile_create.restype = i32
    lib.epik_amd_profile_create.argtypes = [vp, ctypes.POINTER(vp)]
    lib.epik_amd_profile_destroy.restype = None
    lib.epik_amd_profile_destroy.argtypes = [vp]
    lib.epik_amd_profile_reset.restype = i32
    lib.epik_amd_profile_reset.argtypes = [vp]
    lib.epik_amd_profile_read.restype = i32
    lib.epik_amd_profile_read.argtypes = [vp, vp, vp, ctypes.POINTER(ProfileTotals)]
    lib.epik_amd_profile_info.restype = i32
    lib.epik_amd_profile_info.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    lib.epik_amd_profile_add_device.restype = i32
    lib.epik_amd_profile_add_device.argtypes = [vp, vp, vp, vp, vp, u64, vp]
    lib.epik_amd_placer_profile_reads.restype = i32
    lib.epik_amd_placer_profile_reads.argtypes = [vp, vp, vp, vp, vp, u64]
    for name in ("epik_amd_placer_profile_strands", "epik_amd_placer_profile_frames", "epik_amd_placer_profile_mates"):
        getattr(lib, name).restype = i32
        getattr(lib, name).argtypes = [vp, vp, vp, vp, vp, u64, ctypes.c_uint32, vp]
    # (placement confidence: the tree, the kernel, the host entries -- their place_* twins' arguments, then tree, tau_q,
    # conf, profile, weights)
    u32 = ctypes.c_uint32
    lib.epik_amd_tree_create.restype = i32
    lib.epik_amd_tree_create.argtypes = [ctypes.c_int32, vp, vp, u32, ctypes.POINTER(vp)]
    lib.epik_amd_tree_destroy.restype = None
    lib.epik_amd_tree_destroy.argtypes = [vp]
    lib.epik_amd_tree_info.restype = i32
    lib.epik_amd_tree_info.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u64)]
    lib.epik_amd_tree_build_host.restype = i32
    lib.epik_amd_tree_build_host.argtypes = [vp, vp, u32, vp, ctypes.POINTER(u64)]
    lib.epik_amd_tree_lca_host.restype = i32
    lib.epik_amd_tree_lca_host.argtypes = [vp, vp, vp, u64, vp]
    lib.epik_amd_confidence_device.restype = i32
    lib.epik_amd_confidence_device.argtypes = [vp, vp, vp, vp, u64, u32, u32, vp, vp]
    lib.epik_amd_placer_confidence_reads.restype = i32
    lib.epik_amd_placer_confidence_reads.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, u32, vp, vp, vp]
    for name in ("epik_amd_placer_confidence_strands", "epik_amd_placer_confidence_frames", "epik_amd_placer_confidence_mates"):
        getattr(lib, name).restype = i32
        getattr(lib, name).argtypes = [vp, vp, vp, u64, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp]
    # (a cohort of samples: the profile's entries with a sample per read, and the KR distance between the samples)
    lib.epik_amd_cohort_create.restype = i32
    lib.epik_amd_cohort_create.argtypes = [vp, u32, ctypes.POINTER(vp)]
    lib.epik_amd_cohort_destroy.restype = None
    lib.epik_amd_cohort_destroy.argtypes = [vp]
    lib.epik_amd_cohort_reset.restype = i32
    lib.epik_amd_cohort_reset.argtypes = [vp]
    lib.epik_amd_cohort_info.restype = i32
    lib.epik_amd_cohort_info.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
    lib.epik_amd_cohort_read.restype = i32
    lib.epik_amd_cohort_read.argtypes = [vp, vp, vp, vp, ctypes.POINTER(u64)]
    lib.epik_amd_cohort_add_cells.restype = i32
    lib.epik_amd_cohort_add_cells.argtypes = [vp, vp, vp, vp]
    lib.epik_amd_cohort_add_device.restype = i32
    lib.epik_amd_cohort_add_device.argtypes = [vp, vp, vp, vp, vp, vp, u64, vp]
    lib.epik_amd_cohort_kr_device.restype = i32
    lib.epik_amd_cohort_kr_device.argtypes = [vp, vp, vp, vp, vp]
    lib.epik_amd_cohort_kr.restype = i32
    lib.epik_amd_cohort_kr.argtypes = [vp, vp, vp, vp]
    lib.epik_amd_cohort_kr_host.restype = i32
    lib.epik_amd_cohort_kr_host.argtypes = [vp, u32, u32, vp, vp, vp]
    lib.epik_amd_cohort_unifrac_device.restype = i32
    lib.epik_amd_cohort_unifrac_device.argtypes = [vp, vp, vp, u32, vp, vp]
    lib.epik_amd_cohort_unifrac.restype = i32
    lib.epik_amd_cohort_unifrac.argtypes = [vp, vp, vp, u32, vp]
    lib.epik_amd_cohort_unifrac_host.restype = i32
    lib.epik_amd_cohort_unifrac_host.argtypes = [vp, u32, u32, vp, vp, u32, vp]
    lib.epik_amd_cohort_squash_device.restype = i32
    lib.epik_amd_cohort_squash_device.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.epik_amd_cohort_squash.restype = i32
    lib.epik_amd_cohort_squash.argtypes = [vp, vp, vp, vp, ctypes.POINTER(u32)]
    lib.epik_amd_cohort_squash_host.restype = i32
    lib.epik_amd_cohort_squash_host.argtypes = [vp, u32, u32, vp, vp, vp, ctypes.POINTER(u32)]
    lib.epik_amd_cohort_epca_device.restype = i32
    lib.epik_amd_cohort_epca_device.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp]
    lib.epik_amd_cohort_epca.restype = i32
    lib.epik_amd_cohort_epca.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    lib.epik_amd_cohort_epca_host.restype = i32
    lib.epik_amd_cohort_epca_host.argtypes = [vp, u32, u32, vp, u32, vp, vp, vp, vp]
    lib.epik_amd_cohort_kmeans_device.restype = i32
    lib.epik_amd_cohort_kmeans_device.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, vp, vp]
    lib.epik_amd_cohort_kmeans.restype = i32
    lib.epik_amd_cohort_kmeans.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, vp]
    lib.epik_amd_cohort_kmeans_host.restype = i32
    lib.epik_amd_cohort_kmeans_host.argtypes = [vp, u32, u32, vp, vp, u32, u32, vp, vp, vp, vp]
    lib.epik_amd_cohort_alpha_device.restype = i32
    lib.epik_amd_cohort_alpha_device.argtypes = [vp, vp, vp, vp, vp]
    lib.epik_amd_cohort_alpha.restype = i32
    lib.epik_amd_cohort_alpha.argtypes = [vp, vp, vp, vp]
    lib.epik_amd_cohort_alpha_host.restype = i32
    lib.epik_amd_cohort_alpha_host.argtypes = [vp, u32, u32, vp, vp, vp]
    lib.epik_amd_cohort_rarefy_device.restype = i32
    lib.epik_amd_cohort_rarefy_device.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    lib.epik_amd_cohort_rarefy.restype = i32
    lib.epik_amd_cohort_rarefy.argtypes = [vp, vp, vp, u32, u32, vp]
    lib.epik_amd_cohort_rarefy_host.restype = i32
    lib.epik_amd_cohort_rarefy_host.argtypes = [vp, u32, u32, vp, vp, u32, u32, vp]
    lib.epik_amd_cohort_correlation_device.restype = i32
    lib.epik_amd_cohort_correlation_device.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    lib.epik_amd_cohort_correlation.restype = i32
    lib.epik_amd_cohort_correlation.argtypes = [vp, vp, vp, u32, vp, vp]
    lib.epik_amd_cohort_correlation_host.restype = i32
    lib.epik_amd_cohort_correlation_host.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp]
    lib.epik_amd_cohort_dispersion_device.restype = i32
    lib.epik_amd_cohort_dispersion_device.argtypes = [vp, vp, vp, vp]
    lib.epik_amd_cohort_dispersion.restype = i32
    lib.epik_amd_cohort_dispersion.argtypes = [vp, vp, vp]
    lib.epik_amd_cohort_dispersion_host.restype = i32
    lib.epik_amd_cohort_dispersion_host.argtypes = [vp, u32, u32, vp, vp]
    lib.epik_amd_cohort_permanova_device.restype = i32
    lib.epik_amd_cohort_permanova_device.argtypes = [vp, vp, vp, u32, u32, u64, i32, vp, vp, vp, vp]
    lib.epik_amd_cohort_permanova.restype = i32
    lib.epik_amd_cohort_permanova.argtypes = [vp, vp, vp, vp, u32, u32, u64, i32, vp, vp, vp]
    lib.epik_amd_cohort_permanova_host.restype = i32
    lib.epik_amd_cohort_permanova_host.argtypes = [vp, u32, u32, vp, vp, vp, u32, u32, u64, i32, vp, vp, vp]
    lib.epik_amd_cohort_permanova_metric.restype = i32
    lib.epik_amd_cohort_permanova_metric.argtypes = [vp, vp, vp, u32, vp, u32, u32, u64, i32, vp, vp, vp]
    lib.epik_amd_cohort_permanova_metric_host.restype = i32
    lib.epik_amd_cohort_permanova_metric_host.argtypes = [vp, u32, u32, vp, vp, u32, vp, u32, u32, u64, i32, vp, vp, vp]
    lib.epik_amd_cohort_permanova_kr_host.restype = i32
    lib.epik_amd_cohort_permanova_kr_host.argtypes = [vp, vp, u32, vp, u32, u32, u64, i32, vp, vp, vp]
    lib.epik_amd_cohort_model_device.restype = i32
    lib.epik_amd_cohort_model_device.argtypes = [vp, vp, vp, vp, vp, u32, u32, u64, vp, vp, vp, vp, vp]
    lib.epik_amd_cohort_model.restype = i32
    lib.epik_amd_cohort_model.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, u64, vp, vp, vp, vp]
    lib.epik_amd_cohort_model_metric.restype = i32
    lib.epik_amd_cohort_model_metric.argtypes = [vp, vp, vp, u32, vp, vp, vp, u32, u32, u64, vp, vp, vp, vp]
    lib.epik_amd_cohort_model_host.restype = i32
    lib.epik_amd_cohort_model_host.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, u64, vp, vp, vp, vp]
    lib.epik_amd_cohort_model_metric_host.restype = i32
    lib.epik_amd_cohort_model_metric_host.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, u32, u64, vp, vp, vp, vp]
    lib.epik_amd_cohort_model_kr_host.restype = i32
    lib.epik_amd_cohort_model_kr_host.argtypes = [vp, vp, u32, vp, vp, vp, u32, u32, u64, vp, vp, vp, vp]
    lib.epik_amd_cohort_pcoa_device.restype = i32
    lib.epik_amd_cohort_pcoa_device.argtypes = [vp, vp, u32, vp, vp, vp, vp]
    lib.epik_amd_cohort_pcoa.restype = i32
    lib.epik_amd_cohort_pcoa.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    lib.epik_amd_cohort_pcoa_host.restype = i32
    lib.epik_amd_cohort_pcoa_host.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, vp]
    lib.epik_amd_cohort_pcoa_metric.restype = i32
    lib.epik_amd_cohort_pcoa_metric.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp]
    lib.epik_amd_cohort_pcoa_metric_host.restype = i32
    lib.epik_amd_cohort_pcoa_metric_host.argtypes = [vp, u32, u32, vp, vp, u32, u32, vp, vp, vp]
    lib.epik_amd_cohort_pcoa_kr_host.restype = i32
    lib.epik_amd_cohort_pcoa_kr_host.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    lib.epik_amd_cohort_permdisp_device.restype = i32
    lib.epik_amd_cohort_permdisp_device.argtypes = [vp, vp, vp, u32, u32, u64, i32, vp, vp, vp, vp, vp]
    lib.epik_amd_cohort_permdisp.restype = i32
    lib.epik_amd_cohort_permdisp.argtypes = [vp, vp, vp, vp, u32, u32, u64, i32, vp, vp, vp, vp]
    lib.epik_amd_cohort_permdisp_host.restype = i32
    lib.epik_amd_cohort_permdisp_host.argtypes = [vp, u32, u32, vp, vp, vp, u32, u32, u64, i32, vp, vp, vp, vp]
    lib.epik_amd_cohort_permdisp_metric.restype = i32
    lib.epik_amd_cohort_permdisp_metric.argtypes = [vp, vp, vp, u32, vp, u32, u32, u64, i32, vp, vp, vp, vp]
    lib.epik_amd_cohort_permdisp_metric_host.restype = i32
    lib.epik_amd_cohort_permdisp_metric_host.argtypes = [vp, u32, u32, vp, vp, u32, vp, u32, u32, u64, i32, vp, vp, vp, vp]
    lib.epik_amd_cohort_permdisp_kr_host.restype = i32
    lib.epik_amd_cohort_permdisp_kr_host.argtypes = [vp, vp, u32, vp, u32, u32, u64, i32, vp, vp, vp, vp]
    lib.epik_amd_cohort_edgetest_device.restype = i32
    lib.epik_amd_cohort_edgetest_device.argtypes = [vp, vp, vp, u32, u32, u64, vp, vp, vp, vp]
    lib.epik_amd_cohort_edgetest.restype = i32
    lib.epik_amd_cohort_edgetest.argtypes = [vp, vp, vp, u32, u32, u64, vp, vp, vp]
    lib.epik_amd_cohort_edgetest_host.restype = i32
    lib.epik_amd_cohort_edgetest_host.argtypes = [vp, u32, u32, vp, vp, u32, u32, u64, vp, vp, vp]
    # (the edge model: the tree or the cells, the design, P, the seed, the records, the info block, stat, max, aliased)
    design = [vp, vp, vp, u32, u32, u64, vp, vp, vp, vp, vp]
    for form, head, tail in (("_device", [vp, vp], [vp]), ("", [vp, vp], []), ("_host", [vp, u32, u32, vp], [])):
        if not hasattr(lib, "epik_amd_cohort_edgemodel" + form):  # (an older library named by EPIK_AMD_LIB, as below)
            continue
        entry = getattr(lib, "epik_amd_cohort_edgemodel" + form)
        entry.restype = i32
        entry.argtypes = head + design + tail
    # (the strata rule's entries: a sibling's arguments, then strata)
    for name, sibling in (("permanova_strata_device", "permanova_device"), ("permanova_strata", "permanova_metric"),
                          ("permanova_strata_host", "permanova_metric_host"), ("permanova_strata_kr_host", "permanova_kr_host"),
                          ("permdisp_strata_device", "permdisp_device"), ("permdisp_strata", "permdisp_metric"),
                          ("permdisp_strata_host", "permdisp_metric_host"), ("permdisp_strata_kr_host", "permdisp_kr_host"),
                          ("model_strata_device", "model_device"), ("model_strata", "model_metric"),
                          ("model_strata_host", "model_metric_host"), ("model_strata_kr_host", "model_kr_host"),
                          ("edgetest_strata_device", "edgetest_device"), ("edgetest_strata", "edgetest"),
                          ("edgetest_strata_host", "edgetest_host"),
                          ("edgemodel_strata_device", "edgemodel_device"), ("edgemodel_strata", "edgemodel"),
                          ("edgemodel_strata_host", "edgemodel_host")):
        if not hasattr(lib, "epik_amd_cohort_" + name):  # (an older library named by EPIK_AMD_LIB: tools/strata_rate.py's yardstick)
            continue
        getattr(lib, "epik_amd_cohort_" + name).restype = i32
        getattr(lib, "epik_amd_cohort_" + name).argtypes = getattr(lib, "epik_amd_cohort_" + sibling).argtypes + [vp]
    # (Mantel and ANOSIM: the sides or the labels, P, the seed, strata, the record and stat)
    sides = [vp, u32, vp, vp, u32, u32, u32, u32, u64, vp, vp, vp]
    labels = [vp, u32, u32, u64, vp, vp, vp]
    for name, tail in (("mantel", sides), ("anosim", labels)):
        for form, head in (("_device", [vp, vp]), ("", [vp, vp, vp, u32]), ("_host", [vp, u32, u32, vp, vp, u32]),
                           ("_kr_host", [vp, vp, u32])):
            if not hasattr(lib, "epik_amd_cohort_" + name + form):  # (an older library named by EPIK_AMD_LIB, as above)
                continue
            entry = getattr(lib, "epik_amd_cohort_" + name + form)
            entry.restype = i32
            entry.argtypes = head + tail + ([vp] if form == "_device" else [])
    lib.epik_amd_placer_cohort_reads.restype = i32
    lib.epik_amd_placer_cohort_reads.argtypes = [vp, vp, vp, vp, vp, vp, u64]
    for name in ("epik_amd_placer_cohort_strands", "epik_amd_placer_cohort_frames", "epik_amd_placer_cohort_mates"):
        getattr(lib, name).restype = i32
        getattr(lib, name).argtypes = [vp, vp, vp, vp, vp, vp, u64, u32, vp]
    # (taxonomic assignment: the object, its kernel, the rule on the host)
    lib.epik_amd_taxonomy_create.restype = i32
    lib.epik_amd_taxonomy_create.argtypes = [vp, vp, u32, vp, u32, ctypes.POINTER(vp)]
    lib.epik_amd_taxonomy_destroy.restype = None
    lib.epik_amd_taxonomy_destroy.argtypes = [vp]
    lib.epik_amd_taxonomy_reset.restype = i32
    lib.epik_amd_taxonomy_reset.argtypes = [vp]
    lib.epik_amd_taxonomy_info.restype = i32
    lib.epik_amd_taxonomy_info.argtypes = [vp] + [ctypes.POINTER(u32)] * 4
    lib.epik_amd_taxonomy_read.restype = i32
    lib.epik_amd_taxonomy_read.argtypes = [vp, vp, vp, vp, ctypes.POINTER(u64)]
    lib.epik_amd_taxonomy_add_cells.restype = i32
    lib.epik_amd_taxonomy_add_cells.argtypes = [vp, vp, vp, vp]
    lib.epik_amd_taxonomy_add_device.restype = i32
    lib.epik_amd_taxonomy_add_device.argtypes = [vp, vp, vp, vp, vp, vp, u64, u32, vp, vp]
    lib.epik_amd_taxonomy_assign_host.restype = i32
    lib.epik_amd_taxonomy_assign_host.argtypes = [vp, u32, vp, u32, u32, vp, vp, vp, vp, vp, u64, u32, u32, vp, vp, vp, vp,
                                                  ctypes.POINTER(u64)]
    # (the host entries: their place_* twins' arguments, then taxonomy, tau_q, records, weights, samples, profile, cohort)
    lib.epik_amd_placer_taxa_reads.restype = i32
    lib.epik_amd_placer_taxa_reads.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    for name in ("epik_amd_placer_taxa_strands", "epik_amd_placer_taxa_frames", "epik_amd_placer_taxa_mates"):
        getattr(lib, name).restype = i32
        getattr(lib, name).argtypes = [vp, vp, vp, u64, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    # (painting by windows)
    lib.epik_amd_window_span.restype = u64
    lib.epik_amd_window_span.argtypes = [u64, u32, u32, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.epik_amd_placer_window_workspace_bytes.restype = i32
    lib.epik_amd_placer_window_workspace_bytes.argtypes = [vp, u64, u64, u64, u32, ctypes.POINTER(u64)]
    lib.epik_amd_placer_place_windows_device.restype = i32
    lib.epik_amd_placer_place_windows_device.argtypes = [vp, vp, vp, u64, u32, u32, u32, u64, u64, vp, u64, vp, vp, vp, vp, vp, vp]
    lib.epik_amd_placer_place_windows.restype = i32
    lib.epik_amd_placer_place_windows.argtypes = [vp, vp, vp, u64, u32, u32, u32, vp, vp, vp, vp, vp]
    lib.epik_amd_placer_paint_windows.restype = i32
    lib.epik_amd_placer_paint_windows.argtypes = [vp, vp, vp, u64, u32, u32, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.epik_amd_windows_paint_device.restype = i32
    lib.epik_amd_windows_paint_device.argtypes = [i32, vp, vp, vp, vp, u64, u64, u32, vp, u32, u32, vp, vp, vp, vp]
    lib.epik_amd_windows_paint_host.restype = i32
    lib.epik_amd_windows_paint_host.argtypes = [vp, vp, vp, vp, u64, u32, vp, u32, u32, vp, vp, vp]
    # (the database builder)
    lib.epik_amd_builder_create.restype = i32
    lib.epik_amd_builder_create.argtypes = [i32, u32, u32, u32, ctypes.c_float, u64, ctypes.POINTER(vp)]
    lib.epik_amd_builder_add.restype = i32
    lib.epik_amd_builder_add.argtypes = [vp, vp, vp, u64, u64]
    lib.epik_amd_builder_add_device.restype = i32
    lib.epik_amd_builder_add_device.argtypes = [vp, vp, vp, u64, u64]
    lib.epik_amd_builder_finish.restype = i32
    lib.epik_amd_builder_finish.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.epik_amd_builder_copy.restype = i32
    lib.epik_amd_builder_copy.argtypes = [vp, vp, vp, vp]
    lib.epik_amd_builder_destroy.restype = None
    lib.epik_amd_builder_destroy.argtypes = [vp]
    lib.epik_amd_build_host.restype = i32
    lib.epik_amd_build_host.argtypes = [u32, u32, u32, ctypes.c_float, vp, vp, u64, u64, u32, ctypes.POINTER(vp)]
    # (the ancestral reconstruction)
    lib.epik_amd_ancestral_create.restype = i32
    lib.epik_amd_ancestral_create.argtypes = [i32, ctypes.POINTER(AncestralDesc), u64, ctypes.POINTER(vp)]
    lib.epik_amd_ancestral_posteriors.restype = i32
    lib.epik_amd_ancestral_posteriors.argtypes = [vp, vp, u64, u32, vp, vp, ctypes.POINTER(u64)]
    lib.epik_amd_ancestral_posteriors_device.restype = i32
    lib.epik_amd_ancestral_posteriors_device.argtypes = [vp, vp, u64, u32, vp, vp, ctypes.POINTER(u64)]
    lib.epik_amd_ancestral_destroy.restype = None
    lib.epik_amd_ancestral_destroy.argtypes = [vp]
    lib.epik_amd_ancestral_host.restype = i32
    lib.epik_amd_ancestral_host.argtypes = [ctypes.POINTER(AncestralDesc), vp, u64, u32, u32, vp, vp, ctypes.POINTER(u64)]
    lib.epik_amd_model_pmatrices.restype = i32
    lib.epik_amd_model_pmatrices.argtypes = [u32, vp, vp, vp, u64, vp]
    lib.epik_amd_model_gamma_rates.restype = i32
    lib.epik_amd_model_gamma_rates.argtypes = [ctypes.c_double, u32, vp]
    # (the informativeness ranking)
    lib.epik_amd_filter_rank_device.restype = i32
    lib.epik_amd_filter_rank_device.argtypes = [i32, u32, ctypes.c_float, vp, vp, vp, u64, u32, u64, vp, vp, vp]
    lib.epik_amd_filter_rank.restype = i32
    lib.epik_amd_filter_rank.argtypes = [i32, u32, ctypes.c_float, vp, vp, vp, u64, u32, u64, vp, vp]
    lib.epik_amd_builder_rank.restype = i32
    lib.epik_amd_builder_rank.argtypes = [vp, u32, u64, vp, vp]
    lib.epik_amd_filter_rank_host.restype = i32
    lib.epik_amd_filter_rank_host.argtypes = [u32, ctypes.c_float, vp, vp, vp, u64, u32, u64, u32, vp, vp]
    lib.epik_amd_filter_math_host.restype = i32
    lib.epik_amd_filter_math_host.argtypes = [vp, u64, vp, vp]
    _lib = lib
    return lib


def check(code: int) -> None:
    if code != OK:
        raise EpikAmdError(code, (load().epik_amd_last_error() or b"").decode(errors="replace"))


def device_count() -> int:
    lib = load()
    check_hip_runtime()  # (torch may have been imported since load())
    return int(lib.epik_amd_device_count())
