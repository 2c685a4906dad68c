"""The cohort kernels at the branch-count edges and on the three tree shapes of test_cohort_edges_cpu.py, and the LDS tier
seams of the three accumulating kernels.

The sweep: for every (N, shape) of test_cohort_edges_cpu.SWEEP one handle of S = 34 samples (33 used) made through a placer
of that N, and every analysis that reads the branches -- KR, the three UniFrac metrics, squash, edge PCA, k-means with 5
clusters and with 33, alpha, rarefaction, correlation, dispersion, the edge test -- through the poisoned-buffer raw entries
on a stream of its own, against the host mirror: every byte, no tolerance.  What N steps over, kernel by kernel, is listed in
that file's docstring (kChunk / kUnit = 32: 32, 64 and 96 are the empty tail, 96 squash's last unit without a partner; the
scan block of 256: 256 and 512 are full blocks; kLdsBudget: 3072 | 3073).  The mirrors and the conditions that keep the
comparison from passing vacuously come from test_cohort_edges_cpu.edge_case.  For N <= 96 once more on a device of two
workgroups (EPIK_AMD_MAX_BLOCKS=2).

The seams: cohort_add_kernel, profile_kernel and taxa_kernel keep their cells in LDS beside other workgroups' up to kLdsBudget
(48 KiB: N = 3 072; 2 816 taxa after kStaticLds), one workgroup a CU up to kLdsLimit (160 KiB - 64: N = 10 236; 9 980 taxa),
and in global memory beyond.  Each seam is run from both sides on 700 forged reads against the numpy rule, bit for bit, with
rows on the first and on the last LDS cell (branch or taxon 0 and N - 1) beside the bad rows N and N + 1.  At the upper seam
the dynamic LDS and the kernel's static arrays fill the CU's 163 840 bytes to the last 64: a constant that is off by a cell
is a launch the entry refuses there (EpikAmdError) and nowhere else.
"""
import numpy as np
import pytest

from epik_amd import synth, taxonomy
from test_cohort_cpu import assert_cells, numpy_cohort
from test_cohort_edges_cpu import ANALYSES, SAMPLES, SWEEP, SWEEP_IDS, edge_case
from test_cohort_gpu import ENV, add_host, placer_cls  # noqa: F401 (placer_cls: a fixture)
from test_cohort_lifecycle_gpu import SWITCHES, assert_holds, run_analysis
from test_profile_gpu import assert_profile, forged_rows, numpy_rule
from test_taxa_cpu import FORGED_N, FORGED_TAUS, forged, same_bits as same_records
from test_taxa_gpu import DeviceRows, assert_cells as assert_taxa_cells, chain_and_star

pytestmark = pytest.mark.gpu
U64 = np.uint64
TWO_WORKGROUPS_UP_TO = 96
LDS_BUDGET_BRANCHES, LDS_LIMIT_BRANCHES = 3072, 10_236          # cohort_place.hip, profile_place.hip: kLdsBudget, kLdsLimit over 16
LDS_BUDGET_TAXA, LDS_LIMIT_TAXA = 2816, 9980                    # taxa_place.hip: the same after kStaticLds
DBS = {}


def db_of(num_branches):
    if num_branches not in DBS:
        DBS[num_branches] = synth.make_db(num_branches, kmer_size=4, seed=31, p_present=0.7)
    return DBS[num_branches]


def clear_env(monkeypatch):
    for var in ENV + SWITCHES + ("EPIK_AMD_PROFILE_LDS",):
        monkeypatch.delenv(var, raising=False)


# ---- the sweep -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_branches, shape", SWEEP, ids=SWEEP_IDS)
def test_every_analysis_at_the_branch_count_edges(placer_cls, monkeypatch, num_branches, shape):
    clear_env(monkeypatch)
    parent, bl, first, mass, best, params, want = edge_case(num_branches, shape)
    variants = [("as created", None)] + ([("two workgroups", "2")] if num_branches <= TWO_WORKGROUPS_UP_TO else [])
    for variant, blocks in variants:
        if blocks:
            monkeypatch.setenv("EPIK_AMD_MAX_BLOCKS", blocks)
        with placer_cls.from_synth(db_of(num_branches)) as pl, pl.tree(parent, bl) as tree, pl.cohort(SAMPLES) as cohort:
            assert cohort.num_branches == num_branches and cohort.lds_path
            cohort.add_cells(mass, best, None)
            assert_holds(cohort, mass, best, (variant, "before"))
            for name in ANALYSES:
                entry, p = ("kmeans", {**params, "clusters": 33}) if name == "kmeans33" else (name, params)
                run_analysis(entry, pl, cohort, tree, bl, p, want[name], (num_branches, shape, variant, name))
            assert_holds(cohort, mass, best, (variant, "after"))
        monkeypatch.delenv("EPIK_AMD_MAX_BLOCKS", raising=False)


# ---- the LDS tier seams ----------------------------------------------------------------------------------------------
SEAM_ROWS = {}


def seam_rows(num_branches, keep):
    """(rows, n_rows, counts, weights, samples) of 700 forged reads of three samples on a tree of that many branches: the
    batch of test_profile_gpu.forged_rows -- bad rows N, N + 1 and N + 3 included -- with reads of two good rows on branch 0
    and on branch N - 1, the first and the last cell of mass[] and of best[] in LDS."""
    if (num_branches, keep) not in SEAM_ROWS:
        rng = np.random.default_rng(num_branches)
        rows, n_rows, counts, weights = forged_rows(rng, 700, keep, num_branches)
        for start, branch in ((1, 0), (26, num_branches - 1)):
            at = np.arange(start, 700, 50)
            rows["branch"][at, 0], rows["lwr"][at, 0] = branch, 0.75
            if keep > 1:
                rows["branch"][at, 1], rows["lwr"][at, 1] = branch, 0.125
            n_rows[at], counts[at, 0], weights[at] = min(keep, 2), 3, 1 + at % 3
        samples = (np.arange(700, dtype=np.int64) * 3 // 700).astype(np.uint32)      # runs: a workgroup's LDS holds the read's sample
        samples[5::97] = 3 + 4                                                      # (some reads of no sample)
        samples[300:340] = np.arange(40) % 3                                        # ... and a stretch interleaved
        SEAM_ROWS[num_branches, keep] = (rows, n_rows, counts, weights, samples)
    return SEAM_ROWS[num_branches, keep]


SEAMS = (LDS_BUDGET_BRANCHES, LDS_BUDGET_BRANCHES + 1, LDS_LIMIT_BRANCHES, LDS_LIMIT_BRANCHES + 1)
TAXA_SEAMS = (LDS_BUDGET_TAXA, LDS_BUDGET_TAXA + 1, LDS_LIMIT_TAXA, LDS_LIMIT_TAXA + 1)


@pytest.mark.parametrize("num_branches", SEAMS)
def test_cohort_cells_at_the_lds_tier_seams(placer_cls, monkeypatch, num_branches):
    clear_env(monkeypatch)
    n = num_branches
    with placer_cls.from_synth(db_of(n)) as pl:
        rows, n_rows, counts, weights, samples = seam_rows(n, pl.keep_at_most)
        want = numpy_cohort(rows, n_rows, counts, weights, samples, 3, n)
        mass, best = want[0], want[1]
        assert mass[:, 0].any() and mass[:, n - 1].any() and best[:, 0].any() and best[:, n - 1].any()
        assert sum(t["bad_rows"] for t in want[2]) > 0 and want[3] > 0
        paths = [None] + (["0"] if n == LDS_LIMIT_BRANCHES else [])       # the round trip at 10 236: the same cells in global memory
        for lds in paths:
            if lds:
                monkeypatch.setenv("EPIK_AMD_PROFILE_LDS", lds)
            with pl.cohort(3) as cohort:
                assert cohort.lds_path == (n <= LDS_LIMIT_BRANCHES and lds is None), (n, lds)
                add_host(cohort, rows, n_rows, counts, weights, samples)
                assert_cells(cohort.read(), want, (n, lds))


@pytest.mark.parametrize("num_branches", SEAMS)
def test_profile_cells_at_the_lds_tier_seams(placer_cls, monkeypatch, num_branches):
    clear_env(monkeypatch)
    n = num_branches
    with placer_cls.from_synth(db_of(n)) as pl:
        rows, n_rows, counts, weights, _ = seam_rows(n, pl.keep_at_most)
        want = numpy_rule(rows, n_rows, counts, weights, n)
        assert want[0][0] and want[0][n - 1] and want[1][0] and want[1][n - 1] and min(want[2].values()) > 0
        paths = [None] + (["0"] if n == LDS_LIMIT_BRANCHES else [])
        for lds in paths:
            if lds:
                monkeypatch.setenv("EPIK_AMD_PROFILE_LDS", lds)
            with pl.profile() as profile:
                assert profile.lds_path == (n <= LDS_LIMIT_BRANCHES and lds is None), (n, lds)
                profile.add_host(rows, n_rows, counts, weights)
                assert_profile(profile.read(), want, (n, lds))


@pytest.mark.parametrize("num_taxa", TAXA_SEAMS)
def test_taxa_cells_at_the_lds_tier_seams(placer_cls, monkeypatch, num_taxa):
    """Taxonomies of that many taxa over the tree of the forged rows (199 branches).  Branch 0 carries taxon 0, a leaf of
    the star, and branch 1 the root T - 1: the forged batch puts every fifth read on the branches 0 .. 2 alone, so that
    direct[] and assigned[] of both taxa, the first and the last LDS cell of either array, receive mass."""
    clear_env(monkeypatch)
    keep, t = 7, num_taxa
    rows, n_rows, counts = (a[:700] for a in forged(keep))
    rng = np.random.default_rng(t)
    taxon_parent = chain_and_star(t)
    label = rng.integers(0, t, size=FORGED_N).astype(np.uint32)
    label[::3] = rng.integers(t // 2, t, size=len(label[::3]))
    label[0], label[1] = 0, t - 1
    weights = rng.integers(1, 5, size=700).astype(np.uint32)
    weights[::11] = 0
    weights[5::13] = 0xFFFFFFFF
    samples = (np.arange(700, dtype=np.int64) * 3 // 700).astype(np.uint32)
    samples[5::97] = 3 + 4
    samples[300:340] = np.arange(40) % 3
    tq = FORGED_TAUS[1]
    want, cells = taxonomy.numpy_assign(taxon_parent, label, rows, n_rows, counts, tq, weights, samples, 3)
    for plane in (cells.direct, cells.assigned):
        assert plane[:, 0].any() and plane[:, t - 1].any()
    assert cells.bad_samples > 0 and int(cells.totals["bad_reads"].sum()) > 0
    paths = [None] + (["0"] if t == LDS_LIMIT_TAXA else [])
    with placer_cls.from_synth(db_of(FORGED_N), keep_at_most=keep) as pl:
        dev = DeviceRows(pl.device, rows, n_rows, counts)
        for lds in paths:
            if lds:
                monkeypatch.setenv("EPIK_AMD_PROFILE_LDS", lds)
            with pl.taxonomy(taxon_parent, label, 3) as tx:
                assert tx.lds_path == (t <= LDS_LIMIT_TAXA and lds is None), (t, lds)
                dev.add(tx, tq, dev.u32(weights), dev.u32(samples))
                got = dev.records()
                assert same_records(got, want), (t, lds, np.nonzero(got != want)[0][:10])
                assert_taxa_cells(tx.read(), cells, (t, lds))
