#!/usr/bin/env python3
"""EPIK-compatible launcher for the MI355X placement engine.

The command line is the reference launcher's (reference epik.py:29-59): a `place`
command taking -i/--database, -s/--states {nucl,amino}, --omega (1.5), --mu (1.0),
-o/--outputdir, --threads (1), --max-ram and one FASTA file.  Like the reference
(epik.py:73-98) it only selects the native driver -- `epik-dna` for nucl, `epik-aa` for
amino -- translates the options into that driver's flags (-d -q -j --omega --mu -o
[--max-ram]) and runs it.  New options: --gpus, the number of MI355X devices the reads are
sharded across; --db-shard; --strand, which strand of each nucleotide read is placed
(forward as given, its reverse complement, or both and the better one per read); --translate, with
-s amino: nucleotide reads translated into their frames, per read the best frame; and --profile / --profile-only,
the sample's abundance profile per branch beside the jplace or instead of it; --mates, the second FASTA file of a
paired-end sample: every pair gets one placement; --assign / --assign-mass, per read the LCA clade that holds that share
of its placement mass and the EDPL; --cohort, the input file is a list of samples (name<TAB>path lines): their profiles and
the Kantorovich-Rubinstein distance between every two of them, cohort_samples_ / cohort_profile_ / cohort_kr_<list>.tsv;
--cohort-squash, with --cohort: the squash clustering of the samples, cohort_squash_<list>.tsv and .nwk.
--cohort-epca, with --cohort: the edge principal components of the samples, cohort_epca_<list>.tsv and
cohort_epca_edges_<list>.tsv; --cohort-epca-components K of them (default 5).
--cohort-kmeans K, with --cohort: the phylogenetic k-means of the samples into at most K clusters, cohort_kmeans_<list>.tsv
and cohort_kmeans_centroids_<list>.tsv; --cohort-kmeans-iterations M at the most (default 100).
--cohort-alpha, with --cohort: the alpha diversity indices of every sample, cohort_alpha_<list>.tsv.
--cohort-rarefy KMAX, with --cohort: every sample's rarefaction curve up to depth KMAX, cohort_rarefy_<list>.tsv;
--cohort-rarefy-step STEP between two depths (default max(1, ceil(KMAX / 64))).
--cohort-correlation FILE, with --cohort: the correlation of every branch's mass and imbalance with the columns of the
per-sample metadata in FILE (a TSV), cohort_correlation_<list>.tsv.
--cohort-dispersion, with --cohort: how every branch's mass and imbalance vary across the samples, cohort_dispersion_<list>.tsv.
--cohort-permanova FILE, with --cohort: whether the groups of samples in every factor column of FILE (a TSV) differ
(PERMANOVA over the KR distances), cohort_permanova_<list>.tsv; --cohort-permanova-permutations P (default 999),
--cohort-permanova-seed X (default 1), --cohort-permanova-pairwise for every two groups as well.
--cohort-edge-test FILE, with --cohort: on which branches the groups of every factor column of FILE (a TSV) differ (per
branch ANOVA and Kruskal-Wallis of mass and imbalance by permutation, max-statistic adjusted), cohort_edgetest_<list>.tsv;
--cohort-edge-test-permutations P (default 999), --cohort-edge-test-seed X (default 1).
--cohort-permdisp FILE, with --cohort: whether the groups of every factor column of FILE (a TSV, as --cohort-permanova's, at
most 32 labels a column) differ in spread (PERMDISP: distances to group centroids, permutation of residuals),
cohort_permdisp_<list>.tsv; --cohort-permdisp-permutations P (default 999), --cohort-permdisp-seed X (default 1),
--cohort-permdisp-pairwise.
--cohort-edge-model FILE --cohort-edge-model-terms LIST, with --cohort: the same design fitted to every branch's mass share and
imbalance by permutation, with the max-statistic adjustment over the branches, cohort_edgemodel_<list>.tsv;
--cohort-edge-model-permutations P (default 999), --cohort-edge-model-seed X (default 1).
--cohort-model FILE --cohort-model-terms LIST, with --cohort: the sequential model adonis2(D ~ term1 + term2 + ..., by = "terms")
over the columns of FILE (a TSV, as --cohort-permanova's) that LIST names, comma-separated f:NAME (a factor) or n:NAME (a
numeric covariate) in test order, cohort_model_<list>.tsv; --cohort-model-permutations P (default 999), --cohort-model-seed X
(default 1).
--cohort-strata FILE [--cohort-strata-column NAME], with any of the four tests above: permute within strata only (a subject
sampled several times, a batch); a column of FILE (a TSV, as --cohort-permanova's, any number of labels) gives every sample
its stratum, NAME is required when FILE has several columns; the tests' files end their first line in <TAB>strata=NAME.
--cohort-pcoa, with --cohort: the principal coordinates of the samples over the KR distances, all eigenvalues with the
negative ones of a distance that is not Euclidean, cohort_pcoa_<list>.tsv; --cohort-pcoa-components K axes (default 5).
--cohort-unifrac LIST, with --cohort: the UniFrac distances between every two samples, LIST a comma-separated subset of
unweighted, weighted, generalized, or all; cohort_unifrac_<metric>_<list>.tsv each.  --cohort-distance NAME (kr, unweighted,
weighted, generalized): the distance --cohort-permanova, --cohort-pcoa and --cohort-permdisp run over (default kr).
--windows W --window-groups FILE: long sequences painted by windows of W characters, every window placed by itself and called
for a group of FILE (a taxonomy file); windows_<input>.tsv (segments) and windows_breakpoints_<input>.tsv, no jplace;
--window-step S (default max(1, W / 4)), --window-mass (default 0.8), --window-rank D (default 1), --windows-per-window.

Two more commands, not in the reference's launcher (its databases come from another program, IPK), make the database `place`
starts from: `extend -t TREE -r ALIGNMENT -o DIR [--reduction R]` writes the tree and alignment with ghost nodes that an ancestral
reconstruction is run on, and `build -t TREE --ar-probs FILE --ar-tree FILE -s nucl|amino -k K --omega W [--ghosts inner|outer|both]
[--chunk G] -o DB` builds the database on the GPU from that run's posteriors (epik_amd/dbbuild.py, epik_amd/build.py).
`reconstruct -t TREE -r ALIGNMENT --model STR [--model-file F] -s nucl|amino -k K --omega W [--ghosts ...] [--reduction R] [--chunk G]
[--write-ar-probs F --write-ar-tree F] -o DB` needs no outside tool: it reconstructs the ghost nodes' posteriors on the GPU under
a given model (Felsenstein pruning; epik_amd/ancestral.py) and builds the database from them.
`build` and `reconstruct` take `--filter best|mif0|random [--filter-seed X]`: the order the k-mers are stored in, which --mu and
--max-ram cut a prefix of (epik_amd/filters.py; best is the default and the order written so far); `rank -i DB --filter F
[--filter-seed X] [--host] -o OUT` re-ranks a database that exists.
"""
from __future__ import annotations

import os
import subprocess
import sys

import click

__version__ = "0.2.0"

HERE = os.path.dirname(os.path.realpath(__file__))
DRIVERS = {"nucl": "epik-dna", "amino": "epik-aa"}

# (flags, click keyword arguments) -- one row per option of `place`
COHORT_DISTANCES = ("kr", "unweighted", "weighted", "generalized")  # EPIK_AMD_DISTANCE_* by number

PLACE_OPTIONS = [
    (("-i", "--database"), dict(required=True, type=click.Path(exists=True, dir_okay=False),
                                help="Phylo-k-mer database to place against.")),
    (("-s", "--states"), dict(type=click.Choice(sorted(DRIVERS, reverse=True)), default="nucl",
                              show_default=True, help="nucl for DNA, amino for proteins.")),
    (("--omega",), dict(type=float, default=1.5, show_default=True,
                        help="Score-threshold parameter; may exceed the one the database was built with.")),
    (("--mu",), dict(type=float, default=1.0, show_default=True,
                     help="Proportion of the database to load, in (0, 1].")),
    (("-o", "--outputdir"), dict(required=True, type=click.Path(exists=True, file_okay=False),
                                 help="Directory that receives placements_<input>.jplace.")),
    (("--threads",), dict(type=int, default=1, show_default=True,
                          help="Accepted for compatibility; placement runs on the GPU.")),
    (("--max-ram",), dict(type=str, default="", help="Approximate limit on the loaded database, e.g. 512, 256K, 42M, 4.2G.")),
    (("--gpus",), dict(type=int, default=1, show_default=True, help="MI355X devices to shard the reads across.")),
    (("--db-shard",), dict(type=int, default=1, show_default=True,
                           help="Cut the database in this many shards by k-mer code, one per device (a database "
                                "larger than one device's memory); 1 = the whole database on every device.")),
    (("--strand",), dict(type=click.Choice(["forward", "reverse", "both"]), default="forward", show_default=True,
                         help="Strand of each nucleotide read to place: as given, its reverse complement, or both and "
                              "the better one per read (then also strands_<input>.tsv, one name<TAB>+|- per read).")),
    (("--translate",), dict(type=click.Choice(["forward", "reverse", "both"]), default=None,
                            help="With -s amino: the reads are nucleotide reads; place their frames +1 +2 +3 (forward), "
                                 "-1 -2 -3 (reverse) or all six (both), the best frame per read (then also "
                                 "frames_<input>.tsv, one name<TAB>+1..-3 per read).")),
    (("--mates",), dict(type=click.Path(exists=True, dir_okay=False), default=None,
                        help="Paired-end reads: the FASTA file of the second mates, records in the order of the query "
                             "file; every pair gets ONE placement, named by the query's records (-s nucl).")),
    (("--mate-orientation",), dict(type=click.Choice(["fr", "ff"]), default="fr", show_default=True,
                                   help="With --mates: fr, mate 2 is the reverse complement of the fragment's far end "
                                        "(Illumina paired-end), or ff.")),
    (("--profile",), dict(is_flag=True, help="Also write profile_<input>.tsv: per branch the summed like-weight ratios "
                                             "and the reads placed best on it, with clade sums.")),
    (("--profile-only",), dict(is_flag=True, help="Write profile_<input>.tsv and no jplace: the placements are summed on "
                                                  "the device(s) and never leave them (not with --db-shard > 1).")),
    (("--assign",), dict(is_flag=True, help="Also write assign_<input>.tsv (per read the LCA clade that holds --assign-mass "
                                            "of its placement mass, its size and mass, and the EDPL) and "
                                            "assign_clades_<input>.tsv (reads per branch and clade); computed on the "
                                            "device(s) (not with --db-shard > 1).")),
    (("--assign-mass",), dict(type=click.FloatRange(0.0, 1.0), default=None,
                              help="With --assign: the share of a read's placement mass its clade must hold, in [0, 1] "
                                   "[default: 0.95].")),
    (("--cohort",), dict(is_flag=True, help="The input file is a list of samples, one name<TAB>path line each (paths relative "
                                            "to the list): writes no jplace but cohort_samples_<list>.tsv, "
                                            "cohort_profile_<list>.tsv and cohort_kr_<list>.tsv, the KR distance between "
                                            "every two samples (not with --mates, --profile, --profile-only, --assign or "
                                            "--db-shard > 1).")),
    (("--cohort-squash",), dict(is_flag=True, help="With --cohort: also cluster the samples by squash clustering on the device "
                                                   "and write cohort_squash_<list>.tsv (a line per merge) and "
                                                   "cohort_squash_<list>.nwk (the cluster tree).")),
    (("--cohort-epca",), dict(is_flag=True, help="With --cohort: also compute the edge principal components of the samples on "
                                                 "the device and write cohort_epca_<list>.tsv (the components and every "
                                                 "sample's projections) and cohort_epca_edges_<list>.tsv (the components' "
                                                 "coefficients per inner branch).")),
    (("--cohort-epca-components",), dict(type=click.IntRange(1, 64), default=None,
                                         help="With --cohort-epca: the number of components, in [1, 64] [default: 5].")),
    (("--cohort-kmeans",), dict(type=click.IntRange(1, 64), default=None,
                                help="With --cohort: also cluster the samples into at most this many clusters, in [1, 64], by "
                                     "phylogenetic k-means on the device and write cohort_kmeans_<list>.tsv (the clusters and "
                                     "every sample's cluster and distance) and cohort_kmeans_centroids_<list>.tsv (the "
                                     "centroids' masses).")),
    (("--cohort-kmeans-iterations",), dict(type=click.IntRange(1, 1000), default=None,
                                           help="With --cohort-kmeans: the most iterations, in [1, 1000] [default: 100].")),
    (("--cohort-alpha",), dict(is_flag=True, help="With --cohort: also compute the alpha diversity of every sample on the device "
                                                  "(PD, rooted PD, balance-weighted PD at 0.5 and 1, quadratic entropy) and "
                                                  "write cohort_alpha_<list>.tsv.")),
    (("--cohort-rarefy",), dict(type=click.IntRange(1, 1 << 20), default=None,
                                help="With --cohort: also compute every sample's rarefaction curve on the device, the expected "
                                     "PD and rooted PD of k reads up to this depth, in [1, 1048576], and write "
                                     "cohort_rarefy_<list>.tsv.")),
    (("--cohort-rarefy-step",), dict(type=click.IntRange(1, 1 << 20), default=None,
                                     help="With --cohort-rarefy: the distance between two depths; floor(depth / step) must lie "
                                          "in [1, 256] [default: max(1, ceil(depth / 64))].")),
    (("--cohort-correlation",), dict(type=click.Path(), default=None,
                                     help="With --cohort: a TSV of per-sample metadata (header sample<TAB>name1<TAB>..., 1 to 64 "
                                          "numeric columns, empty or NA for a missing value): also correlate every branch's mass "
                                          "and imbalance with every column on the device (Pearson and Spearman) and write "
                                          "cohort_correlation_<list>.tsv.")),
    (("--cohort-dispersion",), dict(is_flag=True, help="With --cohort: also compute how every branch's mass and imbalance vary "
                                                       "across the samples on the device (mean, variance, standard deviation, "
                                                       "coefficient of variation, variance to mean) and write "
                                                       "cohort_dispersion_<list>.tsv.")),
    (("--cohort-permanova",), dict(type=click.Path(), default=None,
                                   help="With --cohort: a TSV of per-sample factors (header sample<TAB>factor1<TAB>..., 1 to 64 "
                                        "columns of labels, empty or NA for a missing one): also test whether the groups of every "
                                        "column differ (PERMANOVA over the KR distances) on the device and write "
                                        "cohort_permanova_<list>.tsv.")),
    (("--cohort-permanova-permutations",), dict(type=click.IntRange(1, 999999), default=None,
                                                help="With --cohort-permanova: the number of permutations [default: 999].")),
    (("--cohort-permanova-seed",), dict(type=click.IntRange(0, (1 << 64) - 1), default=None,
                                        help="With --cohort-permanova: the seed of the permutations, a uint64 [default: 1].")),
    (("--cohort-permanova-pairwise",), dict(is_flag=True, help="With --cohort-permanova: also test every two groups of every "
                                                               "column (at most 32 groups a column).")),
    (("--cohort-edge-test",), dict(type=click.Path(), default=None,
                                   help="With --cohort: a TSV of per-sample factors as --cohort-permanova's (at most 32 labels a "
                                        "column): also test on which branches the groups of every column differ (ANOVA and "
                                        "Kruskal-Wallis of every branch's mass and imbalance by permutation, with the max-statistic "
                                        "adjustment) on the device and write cohort_edgetest_<list>.tsv.")),
    (("--cohort-edge-test-permutations",), dict(type=click.IntRange(1, 999999), default=None,
                                                help="With --cohort-edge-test: the number of permutations [default: 999].")),
    (("--cohort-edge-test-seed",), dict(type=click.IntRange(0, (1 << 64) - 1), default=None,
                                        help="With --cohort-edge-test: the seed of the permutations, a uint64 [default: 1].")),
    (("--cohort-permdisp",), dict(type=click.Path(), default=None,
                                  help="With --cohort: a TSV of factors (as --cohort-permanova's, at most 32 labels a column): also "
                                       "test on the device whether the groups of every column differ in spread (PERMDISP, distances "
                                       "to group centroids over the KR distances) and write cohort_permdisp_<list>.tsv.")),
    (("--cohort-permdisp-permutations",), dict(type=click.IntRange(1, 999999), default=None,
                                               help="With --cohort-permdisp: the number of permutations [default: 999].")),
    (("--cohort-permdisp-seed",), dict(type=click.IntRange(0, (1 << 64) - 1), default=None,
                                       help="With --cohort-permdisp: the seed of the permutations, a uint64 [default: 1].")),
    (("--cohort-permdisp-pairwise",), dict(is_flag=True, help="With --cohort-permdisp: also test every two groups of every column.")),
    (("--cohort-edge-model",), dict(type=click.Path(), default=None,
                                    help="With --cohort: a TSV as --cohort-model's; also fit on the device the sequential linear model "
                                         "of --cohort-edge-model-terms to every branch's mass share and imbalance, by permutation, "
                                         "and write cohort_edgemodel_<list>.tsv.")),
    (("--cohort-edge-model-terms",), dict(type=str, default=None,
                                          help="With --cohort-edge-model (required): the terms in test order, as --cohort-model-terms.")),
    (("--cohort-edge-model-permutations",), dict(type=click.IntRange(1, 999999), default=None,
                                                 help="With --cohort-edge-model: the number of permutations [default: 999].")),
    (("--cohort-edge-model-seed",), dict(type=click.IntRange(0, (1 << 64) - 1), default=None,
                                         help="With --cohort-edge-model: the seed of the permutations, a uint64 [default: 1].")),
    (("--cohort-model",), dict(type=click.Path(), default=None,
                               help="With --cohort: a TSV of factors and covariates (laid out as --cohort-permanova's): also fit on "
                                    "the device the sequential model of the terms of --cohort-model-terms, each tested after the "
                                    "ones before it, and write cohort_model_<list>.tsv.")),
    (("--cohort-model-terms",), dict(type=str, default=None,
                                     help="With --cohort-model (required): the terms in test order, comma-separated f:NAME (a "
                                          "factor) or n:NAME (a numeric covariate).")),
    (("--cohort-model-permutations",), dict(type=click.IntRange(1, 999999), default=None,
                                            help="With --cohort-model: the number of permutations [default: 999].")),
    (("--cohort-model-seed",), dict(type=click.IntRange(0, (1 << 64) - 1), default=None,
                                    help="With --cohort-model: the seed of the permutations, a uint64 [default: 1].")),
    (("--cohort-mantel",), dict(type=click.Path(), default=None,
                                help="With --cohort: a metadata TSV (as --cohort-correlation's): also test on the device, for every "
                                     "column, whether the distance between samples grows with the difference in it (the Mantel "
                                     "test), and write cohort_mantel_<list>.tsv.")),
    (("--cohort-mantel-matrix",), dict(type=str, multiple=True,
                                       help="With --cohort: NAME=FILE, a square TSV laid out as cohort_kr_<list>.tsv, as one more "
                                            "side of the Mantel test; up to 8 times.")),
    (("--cohort-mantel-method",), dict(type=click.Choice(("pearson", "spearman", "both")), default=None,
                                       help="With the Mantel test: the correlation [default: pearson].")),
    (("--cohort-mantel-partial",), dict(type=str, default=None,
                                        help="With the Mantel test: the column or matrix NAME held fixed (the partial Mantel test).")),
    (("--cohort-mantel-permutations",), dict(type=click.IntRange(1, 999999), default=None,
                                             help="With the Mantel test: the number of permutations [default: 999].")),
    (("--cohort-mantel-seed",), dict(type=click.IntRange(0, (1 << 64) - 1), default=None,
                                     help="With the Mantel test: the seed of the permutations, a uint64 [default: 1].")),
    (("--cohort-anosim",), dict(type=click.Path(), default=None,
                                help="With --cohort: a TSV of factors (as --cohort-permanova's): also test on the device whether the "
                                     "ranked distances between the groups of every column exceed those within (ANOSIM), and write "
                                     "cohort_anosim_<list>.tsv.")),
    (("--cohort-anosim-permutations",), dict(type=click.IntRange(1, 999999), default=None,
                                             help="With --cohort-anosim: the number of permutations [default: 999].")),
    (("--cohort-anosim-seed",), dict(type=click.IntRange(0, (1 << 64) - 1), default=None,
                                     help="With --cohort-anosim: the seed of the permutations, a uint64 [default: 1].")),
    (("--cohort-strata",), dict(type=click.Path(), default=None,
                                help="With --cohort-permanova, --cohort-permdisp, --cohort-edge-test or --cohort-model: a TSV (laid "
                                     "out as --cohort-permanova's, any number of labels) whose column gives every sample its "
                                     "stratum: those tests permute within strata only (repeated measures, batches).")),
    (("--cohort-strata-column",), dict(type=str, default=None,
                                       help="With --cohort-strata: the column of its file; required when the file has several.")),
    (("--cohort-pcoa",), dict(is_flag=True, help="With --cohort: also compute the principal coordinates of the samples over "
                                                 "their KR distances on the device and write cohort_pcoa_<list>.tsv (all "
                                                 "eigenvalues, the negative ones included, and every sample's coordinates).")),
    (("--cohort-pcoa-components",), dict(type=click.IntRange(1, 64), default=None,
                                         help="With --cohort-pcoa: the number of axes, in [1, 64] [default: 5].")),
    (("--cohort-unifrac",), dict(type=str, default=None,
                                 help="With --cohort: also compute UniFrac distances between every two samples on the device: a "
                                      "comma-separated subset of unweighted, weighted, generalized, or all; writes "
                                      "cohort_unifrac_<metric>_<list>.tsv each.  The tree is rooted where the database's is.")),
    (("--cohort-distance",), dict(type=click.Choice(COHORT_DISTANCES), default=None,
                                  help="With --cohort-permanova, --cohort-pcoa or --cohort-permdisp: the distance they run over "
                                       "[default: kr]; another one is named at the end of the first line of their files.")),
    (("--taxonomy",), dict(type=click.Path(), default=None,
                           help="A taxonomy file, one leaf_label<TAB>A;B;C line per reference leaf: also write taxa_<input>.tsv "
                                "(per taxon the reads assigned to it and the mass placed in it, with clade sums) or, with "
                                "--cohort, cohort_taxa_<list>.tsv, the sample x taxon table; summed on the device(s) (not with "
                                "--assign or --db-shard > 1).")),
    (("--taxonomy-mass",), dict(type=float, default=None,
                                help="With --taxonomy: the share of a read's placement mass its taxon must hold, in (0.5, 1] "
                                     "[default: 0.95].")),
    (("--taxonomy-per-read",), dict(is_flag=True, help="With --taxonomy: also write taxa_reads_<input>.tsv, per read its taxon, "
                                                       "that taxon's share of the mass and the taxon of its best row.")),
    (("--windows",), dict(type=click.IntRange(1, (1 << 31) - 1), default=None,
                          help="Paint long sequences by windows of this many characters: every window is placed by itself and "
                               "called for a group of --window-groups; writes windows_<input>.tsv (segments) and "
                               "windows_breakpoints_<input>.tsv and no jplace (not with --mates, --translate, --profile, "
                               "--profile-only, --assign, --taxonomy, --cohort or --db-shard > 1).")),
    (("--window-step",), dict(type=click.IntRange(1, (1 << 31) - 1), default=None,
                              help="With --windows: the distance between two windows, in [1, window] [default: max(1, window / 4)].")),
    (("--window-mass",), dict(type=float, default=None,
                              help="With --windows: the share of a window's placement mass its group must hold, in (0.5, 1] "
                                   "[default: 0.8].")),
    (("--window-groups",), dict(type=click.Path(), default=None,
                                help="With --windows (required): a taxonomy file, one leaf_label<TAB>A;B;C line per reference leaf.")),
    (("--window-rank",), dict(type=click.IntRange(1, (1 << 32) - 1), default=None,
                              help="With --windows: the groups are the taxa of this many elements of the taxopath [default: 1].")),
    (("--windows-per-window",), dict(is_flag=True, help="With --windows: also write windows_all_<input>.tsv, a line per window.")),
]


def driver_path(states: str) -> str:
    """The native driver: next to this script when installed, else the in-tree build."""
    name = DRIVERS[states]
    for folder in (HERE, os.path.join(HERE, "epik_amd", "bin")):
        candidate = os.path.join(folder, name)
        if os.path.exists(candidate):
            return candidate
    return os.path.join(HERE, "epik_amd", "bin", name)


def driver_command(database, states, omega, mu, outputdir, threads, max_ram, gpus, input_file, db_shard=1,
                   strand="forward", translate=None, profile=False, profile_only=False, mates=None,
                   mate_orientation="fr", assign=False, assign_mass=None, cohort=False, cohort_squash=False,
                   cohort_epca=False, cohort_epca_components=None, cohort_kmeans=None, cohort_kmeans_iterations=None,
                   cohort_alpha=False, cohort_rarefy=None, cohort_rarefy_step=None, taxonomy=None, taxonomy_mass=None,
                   taxonomy_per_read=False, cohort_correlation=None, cohort_dispersion=False, cohort_permanova=None,
                   cohort_permanova_permutations=None, cohort_permanova_seed=None, cohort_permanova_pairwise=False,
                   cohort_edge_test=None, cohort_edge_test_permutations=None, cohort_edge_test_seed=None,
                   cohort_pcoa=False, cohort_pcoa_components=None, cohort_permdisp=None, cohort_permdisp_permutations=None,
                   cohort_permdisp_seed=None, cohort_permdisp_pairwise=False, cohort_unifrac=None, cohort_distance=None,
                   cohort_model=None, cohort_model_terms=None, cohort_model_permutations=None, cohort_model_seed=None,
                   cohort_edge_model=None, cohort_edge_model_terms=None, cohort_edge_model_permutations=None, cohort_edge_model_seed=None,
                   cohort_strata=None, cohort_strata_column=None, cohort_mantel=None, cohort_mantel_matrix=(),
                   cohort_mantel_method=None, cohort_mantel_partial=None, cohort_mantel_permutations=None, cohort_mantel_seed=None,
                   cohort_anosim=None, cohort_anosim_permutations=None, cohort_anosim_seed=None, windows=None, window_step=None,
                   window_mass=None, window_groups=None, window_rank=None, windows_per_window=False):
    for flag, given in (("--window-step", window_step is not None), ("--window-mass", window_mass is not None),
                        ("--window-groups", window_groups is not None), ("--window-rank", window_rank is not None),
                        ("--windows-per-window", windows_per_window)):
        if given and windows is None:
            raise click.UsageError(f"{flag} needs --windows")
    if windows is not None:
        if window_groups is None:
            raise click.UsageError("--windows needs --window-groups")
        for flag, given in (("--mates", mates is not None), ("--translate", translate is not None), ("--profile", profile),
                            ("--profile-only", profile_only), ("--assign", assign), ("--taxonomy", taxonomy is not None),
                            ("--cohort", cohort), ("--db-shard > 1", db_shard != 1)):
            if given:
                raise click.UsageError(f"--windows does not work with {flag}")
        if window_step is not None and int(window_step) > int(windows):
            raise click.UsageError(f"--window-step must be a whole number in [1, {int(windows)}], not '{int(window_step)}'")
        if window_mass is not None and not 0.5 < float(window_mass) <= 1.0:
            raise click.UsageError("--window-mass must lie in (0.5, 1]")
    with_mantel = cohort_mantel is not None or len(cohort_mantel_matrix) > 0
    for flag, given in (("--cohort-mantel", cohort_mantel is not None), ("--cohort-mantel-matrix", len(cohort_mantel_matrix) > 0),
                        ("--cohort-anosim", cohort_anosim is not None)):
        if given and not cohort:
            raise click.UsageError(f"{flag} needs --cohort")
    for flag, given in (("--cohort-mantel-method", cohort_mantel_method is not None),
                        ("--cohort-mantel-partial", cohort_mantel_partial is not None),
                        ("--cohort-mantel-permutations", cohort_mantel_permutations is not None),
                        ("--cohort-mantel-seed", cohort_mantel_seed is not None)):
        if given and not with_mantel:
            raise click.UsageError(f"{flag} needs --cohort-mantel or --cohort-mantel-matrix")
    for flag, given in (("--cohort-anosim-permutations", cohort_anosim_permutations is not None),
                        ("--cohort-anosim-seed", cohort_anosim_seed is not None)):
        if given and cohort_anosim is None:
            raise click.UsageError(f"{flag} needs --cohort-anosim")
    if len(cohort_mantel_matrix) > 8:
        raise click.UsageError("--cohort-mantel-matrix may be given 8 times at the most")
    if taxonomy_mass is not None and taxonomy is None:
        raise click.UsageError("--taxonomy-mass needs --taxonomy")
    if taxonomy_per_read and taxonomy is None:
        raise click.UsageError("--taxonomy-per-read needs --taxonomy")
    if taxonomy is not None and assign:
        raise click.UsageError("--taxonomy does not work with --assign")
    if taxonomy is not None and db_shard != 1:
        raise click.UsageError("--taxonomy does not work with --db-shard > 1")
    if taxonomy_mass is not None and not 0.5 < float(taxonomy_mass) <= 1.0:
        raise click.UsageError("--taxonomy-mass must lie in (0.5, 1]")
    if assign_mass is not None and not assign:
        raise click.UsageError("--assign-mass needs --assign")
    if assign and db_shard != 1:
        raise click.UsageError("--assign does not work with --db-shard > 1")
    if cohort_squash and not cohort:
        raise click.UsageError("--cohort-squash needs --cohort")
    if cohort_epca and not cohort:
        raise click.UsageError("--cohort-epca needs --cohort")
    if cohort_epca_components is not None and not cohort_epca:
        raise click.UsageError("--cohort-epca-components needs --cohort-epca")
    if cohort_kmeans is not None and not cohort:
        raise click.UsageError("--cohort-kmeans needs --cohort")
    if cohort_kmeans_iterations is not None and cohort_kmeans is None:
        raise click.UsageError("--cohort-kmeans-iterations needs --cohort-kmeans")
    if cohort_alpha and not cohort:
        raise click.UsageError("--cohort-alpha needs --cohort")
    if cohort_rarefy is not None and not cohort:
        raise click.UsageError("--cohort-rarefy needs --cohort")
    if cohort_rarefy_step is not None and cohort_rarefy is None:
        raise click.UsageError("--cohort-rarefy-step needs --cohort-rarefy")
    if cohort_rarefy is not None:
        step = int(cohort_rarefy_step) if cohort_rarefy_step is not None else max(1, -(-int(cohort_rarefy) // 64))
        if not 1 <= int(cohort_rarefy) // step <= 256:
            raise click.UsageError(f"--cohort-rarefy-step {step}: floor({int(cohort_rarefy)} / {step}) depths of --cohort-rarefy "
                                   "must lie in [1, 256]")
    if cohort_correlation is not None and not cohort:
        raise click.UsageError("--cohort-correlation needs --cohort")
    if cohort_dispersion and not cohort:
        raise click.UsageError("--cohort-dispersion needs --cohort")
    if cohort_permanova is not None and not cohort:
        raise click.UsageError("--cohort-permanova needs --cohort")
    for flag, given in (("--cohort-permanova-permutations", cohort_permanova_permutations is not None),
                        ("--cohort-permanova-seed", cohort_permanova_seed is not None),
                        ("--cohort-permanova-pairwise", cohort_permanova_pairwise)):
        if given and cohort_permanova is None:
            raise click.UsageError(f"{flag} needs --cohort-permanova")
    if cohort_edge_test is not None and not cohort:
        raise click.UsageError("--cohort-edge-test needs --cohort")
    for flag, given in (("--cohort-edge-test-permutations", cohort_edge_test_permutations is not None),
                        ("--cohort-edge-test-seed", cohort_edge_test_seed is not None)):
        if given and cohort_edge_test is None:
            raise click.UsageError(f"{flag} needs --cohort-edge-test")
    if cohort_permdisp is not None and not cohort:
        raise click.UsageError("--cohort-permdisp needs --cohort")
    for flag, given in (("--cohort-permdisp-permutations", cohort_permdisp_permutations is not None),
                        ("--cohort-permdisp-seed", cohort_permdisp_seed is not None),
                        ("--cohort-permdisp-pairwise", cohort_permdisp_pairwise)):
        if given and cohort_permdisp is None:
            raise click.UsageError(f"{flag} needs --cohort-permdisp")
    if cohort_model is not None and not cohort:
        raise click.UsageError("--cohort-model needs --cohort")
    for flag, given in (("--cohort-model-terms", cohort_model_terms is not None),
                        ("--cohort-model-permutations", cohort_model_permutations is not None),
                        ("--cohort-model-seed", cohort_model_seed is not None)):
        if given and cohort_model is None:
            raise click.UsageError(f"{flag} needs --cohort-model")
    if cohort_model is not None and cohort_model_terms is None:
        raise click.UsageError("--cohort-model needs --cohort-model-terms")
    if cohort_edge_model is not None and not cohort:
        raise click.UsageError("--cohort-edge-model needs --cohort")
    for flag, given in (("--cohort-edge-model-terms", cohort_edge_model_terms is not None),
                        ("--cohort-edge-model-permutations", cohort_edge_model_permutations is not None),
                        ("--cohort-edge-model-seed", cohort_edge_model_seed is not None)):
        if given and cohort_edge_model is None:
            raise click.UsageError(f"{flag} needs --cohort-edge-model")
    if cohort_edge_model is not None and cohort_edge_model_terms is None:
        raise click.UsageError("--cohort-edge-model needs --cohort-edge-model-terms")
    if cohort_strata_column is not None and cohort_strata is None:
        raise click.UsageError("--cohort-strata-column needs --cohort-strata")
    if cohort_strata is not None and cohort_permanova is None and cohort_permdisp is None and cohort_edge_test is None \
            and cohort_model is None and not with_mantel and cohort_anosim is None and cohort_edge_model is None:
        raise click.UsageError("--cohort-strata needs --cohort-permanova, --cohort-permdisp, --cohort-edge-test or --cohort-model")
    if cohort_pcoa and not cohort:
        raise click.UsageError("--cohort-pcoa needs --cohort")
    if cohort_pcoa_components is not None and not cohort_pcoa:
        raise click.UsageError("--cohort-pcoa-components needs --cohort-pcoa")
    if cohort_unifrac is not None:
        if not cohort:
            raise click.UsageError("--cohort-unifrac needs --cohort")
        names = str(cohort_unifrac).split(",")
        for i, name in enumerate(names):
            if str(cohort_unifrac) == "all":
                break
            if name not in COHORT_DISTANCES[1:]:
                raise click.UsageError(f"--cohort-unifrac: '{name}' is no UniFrac distance (unweighted, weighted, generalized, or all)")
            if name in names[:i]:
                raise click.UsageError(f"--cohort-unifrac: '{name}' is given twice")
    if cohort_distance is not None:
        if cohort_distance not in COHORT_DISTANCES:
            raise click.UsageError(f"--cohort-distance must be kr, unweighted, weighted or generalized, not '{cohort_distance}'")
        if cohort_permanova is None and not cohort_pcoa and cohort_permdisp is None and cohort_model is None and not with_mantel \
                and cohort_anosim is None:
            raise click.UsageError("--cohort-distance needs --cohort-permanova, --cohort-pcoa or --cohort-permdisp")
    if cohort:
        for flag, given in (("--mates", mates is not None), ("--profile", profile), ("--profile-only", profile_only),
                            ("--assign", assign), ("--db-shard > 1", db_shard != 1)):
            if given:
                raise click.UsageError(f"--cohort does not work with {flag}")
    argv = [driver_path(states), "-d", str(database), "-q", str(input_file), "-j", str(threads),
            "--omega", str(omega), "--mu", str(mu), "-o", str(outputdir)]
    if max_ram:
        argv += ["--max-ram", max_ram]
    if gpus != 1:
        argv += ["--gpus", str(gpus)]
    if db_shard != 1:
        argv += ["--db-shard", str(db_shard)]
    if strand != "forward":
        argv += ["--strand", str(strand)]
    if translate is not None:
        argv += ["--translate", str(translate)]
    if mates is not None:
        argv += ["--mates", str(mates)]
        if mate_orientation != "fr":
            argv += ["--mate-orientation", str(mate_orientation)]
    if profile:
        argv += ["--profile"]
    if profile_only:
        argv += ["--profile-only"]
    if assign:
        argv += ["--assign"]
        if assign_mass is not None:
            argv += ["--assign-mass", repr(float(assign_mass))]
    if cohort:
        argv += ["--cohort"]
    if cohort_squash:
        argv += ["--cohort-squash"]
    if cohort_epca:
        argv += ["--cohort-epca"]
        if cohort_epca_components is not None:
            argv += ["--cohort-epca-components", str(int(cohort_epca_components))]
    if cohort_kmeans is not None:
        argv += ["--cohort-kmeans", str(int(cohort_kmeans))]
        if cohort_kmeans_iterations is not None:
            argv += ["--cohort-kmeans-iterations", str(int(cohort_kmeans_iterations))]
    if cohort_alpha:
        argv += ["--cohort-alpha"]
    if cohort_rarefy is not None:
        argv += ["--cohort-rarefy", str(int(cohort_rarefy))]
        if cohort_rarefy_step is not None:
            argv += ["--cohort-rarefy-step", str(int(cohort_rarefy_step))]
    if cohort_correlation is not None:
        argv += ["--cohort-correlation", str(cohort_correlation)]
    if cohort_dispersion:
        argv += ["--cohort-dispersion"]
    if cohort_permanova is not None:
        argv += ["--cohort-permanova", str(cohort_permanova)]
        if cohort_permanova_permutations is not None:
            argv += ["--cohort-permanova-permutations", str(int(cohort_permanova_permutations))]
        if cohort_permanova_seed is not None:
            argv += ["--cohort-permanova-seed", str(int(cohort_permanova_seed))]
        if cohort_permanova_pairwise:
            argv += ["--cohort-permanova-pairwise"]
    if cohort_edge_test is not None:
        argv += ["--cohort-edge-test", str(cohort_edge_test)]
        if cohort_edge_test_permutations is not None:
            argv += ["--cohort-edge-test-permutations", str(int(cohort_edge_test_permutations))]
        if cohort_edge_test_seed is not None:
            argv += ["--cohort-edge-test-seed", str(int(cohort_edge_test_seed))]
    if cohort_permdisp is not None:
        argv += ["--cohort-permdisp", str(cohort_permdisp)]
        if cohort_permdisp_permutations is not None:
            argv += ["--cohort-permdisp-permutations", str(int(cohort_permdisp_permutations))]
        if cohort_permdisp_seed is not None:
            argv += ["--cohort-permdisp-seed", str(int(cohort_permdisp_seed))]
        if cohort_permdisp_pairwise:
            argv += ["--cohort-permdisp-pairwise"]
    if cohort_mantel is not None:
        argv += ["--cohort-mantel", str(cohort_mantel)]
    for matrix in cohort_mantel_matrix:
        argv += ["--cohort-mantel-matrix", str(matrix)]
    for flag, value in (("--cohort-mantel-method", cohort_mantel_method), ("--cohort-mantel-partial", cohort_mantel_partial),
                        ("--cohort-mantel-permutations", cohort_mantel_permutations), ("--cohort-mantel-seed", cohort_mantel_seed)):
        if value is not None:
            argv += [flag, str(value)]
    if cohort_anosim is not None:
        argv += ["--cohort-anosim", str(cohort_anosim)]
        for flag, value in (("--cohort-anosim-permutations", cohort_anosim_permutations), ("--cohort-anosim-seed", cohort_anosim_seed)):
            if value is not None:
                argv += [flag, str(value)]
    if cohort_strata is not None:
        argv += ["--cohort-strata", str(cohort_strata)]
        if cohort_strata_column is not None:
            argv += ["--cohort-strata-column", str(cohort_strata_column)]
    if cohort_edge_model is not None:
        argv += ["--cohort-edge-model", str(cohort_edge_model), "--cohort-edge-model-terms", str(cohort_edge_model_terms)]
        if cohort_edge_model_permutations is not None:
            argv += ["--cohort-edge-model-permutations", str(int(cohort_edge_model_permutations))]
        if cohort_edge_model_seed is not None:
            argv += ["--cohort-edge-model-seed", str(int(cohort_edge_model_seed))]
    if cohort_model is not None:
        argv += ["--cohort-model", str(cohort_model), "--cohort-model-terms", str(cohort_model_terms)]
        if cohort_model_permutations is not None:
            argv += ["--cohort-model-permutations", str(int(cohort_model_permutations))]
        if cohort_model_seed is not None:
            argv += ["--cohort-model-seed", str(int(cohort_model_seed))]
    if cohort_pcoa:
        argv += ["--cohort-pcoa"]
        if cohort_pcoa_components is not None:
            argv += ["--cohort-pcoa-components", str(int(cohort_pcoa_components))]
    if cohort_unifrac is not None:
        argv += ["--cohort-unifrac", str(cohort_unifrac)]
    if cohort_distance is not None:
        argv += ["--cohort-distance", str(cohort_distance)]
    if taxonomy is not None:
        argv += ["--taxonomy", str(taxonomy)]
        if taxonomy_mass is not None:
            argv += ["--taxonomy-mass", repr(float(taxonomy_mass))]
        if taxonomy_per_read:
            argv += ["--taxonomy-per-read"]
    if windows is not None:
        argv += ["--windows", str(int(windows)), "--window-groups", str(window_groups)]
        if window_step is not None:
            argv += ["--window-step", str(int(window_step))]
        if window_mass is not None:
            argv += ["--window-mass", repr(float(window_mass))]
        if window_rank is not None:
            argv += ["--window-rank", str(int(window_rank))]
        if windows_per_window:
            argv += ["--windows-per-window"]
    return argv + [str(input_file)]  # the reference passes the query a second time, positionally


class Launcher(click.Group):
    """The launcher's group.  `commands` holds what came with the database builder (place, extend, build), the set
    tests/test_dbbuild_cpu.py fixes; a command added since is looked up by name here, so it is listed, documented by --help
    and run like the others."""
    later = {}

    def list_commands(self, ctx):
        return sorted(set(super().list_commands(ctx)) | set(self.later))

    def get_command(self, ctx, name):
        return super().get_command(ctx, name) or self.later.get(name)


@click.group(cls=Launcher)
@click.version_option(__version__)
def epik():
    """Phylogenetic placement with informative k-mers on AMD Instinct MI355X."""


def _place(input_file, **options):
    """Places the sequences of a FASTA file:  epik.py place -i DB -o OUTDIR [-s nucl|amino] QUERY.fasta"""
    argv = driver_command(input_file=input_file, **options)
    print(" ".join(argv))
    sys.exit(subprocess.call(argv))


place = click.argument("input_file", type=click.Path(exists=True))(_place)
for flags, kwargs in reversed(PLACE_OPTIONS):
    place = click.option(*flags, **kwargs)(place)
place = epik.command(name="place")(place)


def _fail_usage(err):
    raise click.UsageError(str(err))


@epik.command(name="extend")
@click.option("-t", "--tree", "tree", required=True, type=click.Path(exists=True, dir_okay=False),
              help="The reference tree (Newick, rooted and binary).")
@click.option("-r", "--refalign", "refalign", required=True, type=click.Path(exists=True, dir_okay=False),
              help="The reference alignment (FASTA), a sequence per leaf of the tree.")
@click.option("-o", "--outputdir", required=True, type=click.Path(file_okay=False),
              help="Directory that receives extended.nwk, extended.fasta and columns.tsv.")
@click.option("--reduction", type=float, default=None,
              help="First remove the columns whose share of gaps is at least this [default: keep every column].")
def extend(tree, refalign, outputdir, reduction):
    """Adds the ghost nodes to a reference tree and alignment: what the ancestral reconstruction is run on."""
    from epik_amd import dbbuild
    try:
        paths = dbbuild.extend_files(tree, refalign, outputdir, reduction)
    except dbbuild.BuildInputError as err:
        _fail_usage(err)
    for path in paths.values():
        print(path)


@epik.command(name="build")
@click.option("-t", "--tree", "tree", required=True, type=click.Path(dir_okay=False), help="The reference tree `extend` was given.")
@click.option("--ar-probs", required=True, type=click.Path(dir_okay=False),
              help="The reconstruction's posteriors: a tab-separated table with Node, Site and p_<state> columns "
                   "(RAxML-NG --ancestral: *.ancestralProbs).")
@click.option("--ar-tree", required=True, type=click.Path(dir_okay=False),
              help="The extended tree as the reconstruction wrote it back, inner nodes labelled (*.ancestralTree).")
@click.option("-s", "--states", type=click.Choice(sorted(DRIVERS, reverse=True)), default="nucl", show_default=True,
              help="nucl for DNA, amino for proteins.")
@click.option("-k", "--kmer-size", "kmer_size", required=True, type=int, help="k: 2 to 15 for nucl, 2 to 7 for amino.")
@click.option("--omega", type=float, default=1.5, show_default=True, help="Score-threshold parameter: (omega / sigma)^k.")
@click.option("--ghosts", type=click.Choice(["inner", "outer", "both"]), default="both", show_default=True,
              help="Which ghost nodes of every branch to use: its midpoint (inner), the pendant node (outer), or both.")
@click.option("--chunk", type=int, default=256, show_default=True, help="Ghost nodes handed to the device at a time.")
@click.option("--filter", "filter_name", type=str, default="best", show_default=True,
              help="The order the k-mers are stored in, most informative first (--mu and --max-ram load a prefix of it): best (the "
                   "best score of a k-mer's list), mif0 (the entropy of the branch given the k-mer) or random.")
@click.option("--filter-seed", type=click.IntRange(0, (1 << 64) - 1), default=None,
              help="With --filter random: the seed, a uint64 [default: 0].")
@click.option("--host", is_flag=True, help="Run the host mirrors of the builder and the ranking: no GPU, and slow.")
@click.option("-o", "--output", "output", required=True, type=click.Path(dir_okay=False), help="The database to write (.ekdb).")
def build_db(tree, ar_probs, ar_tree, states, kmer_size, omega, ghosts, chunk, filter_name, filter_seed, host, output):
    """Builds a phylo-k-mer database on the GPU from the posteriors of an extended tree's ghost nodes."""
    from epik_amd import dbbuild
    try:
        dbbuild.check_build_options(states, kmer_size, omega, chunk)  # (before anything is opened)
        dbbuild.check_filter_options(filter_name, filter_seed)
    except dbbuild.BuildInputError as err:
        _fail_usage(err)
    for flag, path in (("-t", tree), ("--ar-probs", ar_probs), ("--ar-tree", ar_tree)):
        if not os.path.isfile(path):
            raise click.UsageError(f"{flag}: the file '{path}' does not exist")
    try:
        info = dbbuild.build_from_files(tree, ar_probs, ar_tree, states, kmer_size, omega, output, ghosts=ghosts, chunk=chunk,
                                        host=host, filter=filter_name, filter_seed=filter_seed)
    except dbbuild.BuildInputError as err:
        _fail_usage(err)
    print(f"{output}: {info['num_keys']} k-mers, {info['num_entries']} phylo-k-mers from {info['ghost_nodes']} ghost nodes "
          f"of {info['num_branches'] - 1} branches")


@click.command(name="reconstruct")
@click.option("-t", "--tree", "tree", required=True, type=click.Path(dir_okay=False), help="The reference tree (Newick, rooted and binary).")
@click.option("-r", "--refalign", "refalign", required=True, type=click.Path(dir_okay=False),
              help="The reference alignment (FASTA), a sequence per leaf of the tree.")
@click.option("--model", required=True, type=str,
              help="The substitution model with its parameters, in RAxML-NG's notation: JC, K80{k}, HKY{k}, GTR{ac/ag/at/cg/ct/gt} "
                   "(nucl), POISSON or USER (amino; USER: the matrix of --model-file); +FU{..}, +FC or +FE; +G4{alpha} or "
                   "+Gn{alpha}; +I{p}.  Nothing is optimised.")
@click.option("--model-file", type=click.Path(dir_okay=False), default=None,
              help="With the model USER: a PAML-format matrix, 190 exchangeabilities and 20 frequencies.")
@click.option("-s", "--states", type=click.Choice(sorted(DRIVERS, reverse=True)), default="nucl", show_default=True,
              help="nucl for DNA, amino for proteins.")
@click.option("-k", "--kmer-size", "kmer_size", required=True, type=int, help="k: 2 to 15 for nucl, 2 to 7 for amino.")
@click.option("--omega", type=float, default=1.5, show_default=True, help="Score-threshold parameter: (omega / sigma)^k.")
@click.option("--ghosts", type=click.Choice(["inner", "outer", "both"]), default="both", show_default=True,
              help="Which ghost nodes of every branch to use: its midpoint (inner), the pendant node (outer), or both.")
@click.option("--reduction", type=float, default=None,
              help="First remove the columns whose share of gaps is at least this [default: keep every column].")
@click.option("--chunk", type=int, default=256, show_default=True, help="Ghost nodes handed to the device builder at a time.")
@click.option("--write-ar-probs", type=click.Path(dir_okay=False), default=None,
              help="Also write the posteriors as the table `build --ar-probs` reads (with --write-ar-tree).")
@click.option("--write-ar-tree", type=click.Path(dir_okay=False), default=None,
              help="Also write the extended tree with the labels of that table, as `build --ar-tree` reads it.")
@click.option("--filter", "filter_name", type=str, default="best", show_default=True,
              help="The order the k-mers are stored in, most informative first (--mu and --max-ram load a prefix of it): best (the "
                   "best score of a k-mer's list), mif0 (the entropy of the branch given the k-mer) or random.")
@click.option("--filter-seed", type=click.IntRange(0, (1 << 64) - 1), default=None,
              help="With --filter random: the seed, a uint64 [default: 0].")
@click.option("--host", is_flag=True, help="Run the host mirrors of the reconstruction, the builder and the ranking: no GPU, and slow.")
@click.option("--threads", type=int, default=1, show_default=True, help="With --host: threads of the host mirrors.")
@click.option("-o", "--output", "output", required=True, type=click.Path(dir_okay=False), help="The database to write (.ekdb).")
def reconstruct(tree, refalign, model, model_file, states, kmer_size, omega, ghosts, reduction, chunk, write_ar_probs, write_ar_tree,
                filter_name, filter_seed, host, threads, output):
    """Builds a phylo-k-mer database from a reference tree and alignment: the ancestral posteriors of the ghost nodes are
    reconstructed on the GPU under the given model, then the database is built from them."""
    from epik_amd import ancestral, dbbuild
    try:  # (before anything is opened)
        dbbuild.check_build_options(states, kmer_size, omega, chunk)
        dbbuild.check_filter_options(filter_name, filter_seed)
        ancestral.Model.parse(model, states).check_model_file(model_file)
    except dbbuild.BuildInputError as err:
        _fail_usage(err)
    except ancestral.ModelError as err:
        _fail_usage(f"--model: {err}")
    for flag, path in (("-t", tree), ("-r", refalign), ("--model-file", model_file)):
        if path is not None and not os.path.isfile(path):
            raise click.UsageError(f"{flag}: the file '{path}' does not exist")
    try:
        info = dbbuild.build_from_alignment(tree, refalign, model, states, kmer_size, omega, output, model_file=model_file, ghosts=ghosts,
                                            reduction=reduction, chunk=chunk, host=host, num_threads=threads,
                                            write_ar_probs=write_ar_probs, write_ar_tree=write_ar_tree, filter=filter_name,
                                            filter_seed=filter_seed)
    except dbbuild.BuildInputError as err:
        _fail_usage(err)
    print(f"{output}: {info['num_keys']} k-mers, {info['num_entries']} phylo-k-mers from {info['ghost_nodes']} ghost nodes "
          f"of {info['num_branches'] - 1} branches, {info['sites']} sites, {info['categories']} rate categories"
          + (f"; {info['dead_sites']} rows without a posterior" if info["dead_sites"] else ""))


Launcher.later["reconstruct"] = reconstruct


@click.command(name="rank")
@click.option("-i", "--database", "database", required=True, type=click.Path(dir_okay=False), help="The database to re-rank (.ekdb).")
@click.option("--filter", "filter_name", required=True, type=str, help="best, mif0 or random: as `build --filter`.")
@click.option("--filter-seed", type=click.IntRange(0, (1 << 64) - 1), default=None,
              help="With --filter random: the seed, a uint64 [default: 0].")
@click.option("--host", is_flag=True, help="Rank on the host mirror: no GPU.")
@click.option("--threads", type=int, default=1, show_default=True, help="With --host: threads of the host mirror.")
@click.option("-o", "--output", "output", required=True, type=click.Path(dir_okay=False), help="The database to write (.ekdb).")
def rank_db(database, filter_name, filter_seed, host, threads, output):
    """Re-ranks the k-mers of a database that exists: read whole at its own omega, ranked on the GPU, written in the new order."""
    from epik_amd import dbbuild
    try:
        dbbuild.check_filter_options(filter_name, filter_seed)  # (before anything is opened)
    except dbbuild.BuildInputError as err:
        _fail_usage(err)
    if not os.path.isfile(database):
        raise click.UsageError(f"-i: the file '{database}' does not exist")
    try:
        info = dbbuild.rerank_file(database, output, filter_name, filter_seed, host=host, num_threads=threads)
    except dbbuild.BuildInputError as err:
        _fail_usage(err)
    print(f"{output}: {info['num_keys']} k-mers, {info['num_entries']} phylo-k-mers ranked by {filter_name}")


Launcher.later["rank"] = rank_db


if __name__ == "__main__":
    epik()
