"""One cohort handle through a life: the ten analyses of a cohort (KR, squash, edge PCA, k-means, alpha, rarefaction,
correlation, dispersion, PERMANOVA, the edge test) on one handle whose cells change from stage to stage, in an order that
changes from stage to stage, with parameters that shrink and grow against the stage before -- what a host driver that uses
one handle for several cohorts does, and what the tests of the single analyses (a fresh cohort, one add_cells, the analysis)
never do.  Stale state in a workspace -- padding samples of the planes, centroid planes beyond K', list entries beyond L,
sorted copies in the rank rows, counters and maxima of the column before -- shows only here.

Every comparison is bit for bit against the host mirror (cohort_mod.*_host, which the _cpu tests hold to the numpy
restatements): no tolerance in this file.  The mirrors are computed once per shape from a stage's intended cells, before
anything touches the device, and shared by the variants of the walk; at every stage cohort.read() is asserted equal to those
cells first, so the mirror is the mirror of what read() returns.

That the walk sees stale state was shown once on two scratch builds of edgetest_place.hip: without the
per-column reset of the maxima this file fails, and so does test_edgetest_gpu.py (a column's maxima reach the next column of
the same call); with the reset dropped only before a call's first column test_edgetest_gpu.py passes and every variant of the
walk fails at the edge test of the last stage.

And the device entries back to back on two streams with no host synchronisation between: include/epik_amd.h promises that
each synchronises the device before it touches a workspace.
"""
from dataclasses import dataclass, field

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod
from test_cohort_cpu import random_cells, same_bits
from test_cohort_gpu import ENV, kr_case, placer_cls  # noqa: F401 (placer_cls: a fixture)
from test_correlation_cpu import is_na, metadata, same_records
from test_correlation_gpu import assert_correlation, device_correlation_raw, device_dispersion_raw, wide_metadata
from test_diversity_cpu import draw_best
from test_diversity_gpu import device_alpha_raw, device_rarefy_raw
from test_edgetest_cpu import same_edgetest
from test_edgetest_gpu import device_edgetest_raw, group_labels
from test_epca_cpu import assert_epca
from test_epca_gpu import device_epca_raw
from test_kmeans_cpu import assert_kmeans
from test_kmeans_gpu import device_kmeans_raw
from test_permanova_cpu import factor_columns, same_permanova
from test_permanova_gpu import SLOTS, device_permanova_raw, sparser
from test_squash_cpu import host_all_records
from test_squash_gpu import device_all_records
from test_unifrac_cpu import METRICS
from test_unifrac_gpu import device_matrix

pytestmark = pytest.mark.gpu
U64 = np.uint64
COUNT_SAMPLES = 128          # cohort_device.hpp: kCohortCountSamples, where the ranking goes from counting to sorting
SWITCHES = ("EPIK_AMD_EDGETEST_LDS", "EPIK_AMD_PERMANOVA_LDS", "EPIK_AMD_EPCA_LDS", "EPIK_AMD_CORRELATION_LDS")
ANALYSES = ("kr", "squash", "epca", "kmeans", "alpha", "rarefy", "correlation", "dispersion", "permanova", "edgetest")
UNIFRAC = tuple(METRICS)      # "unweighted", "weighted", "generalized": names that mirrors() and run_analysis() take as well
STAGES = ("dense","thin", "zero", "two", "same", "sum")
DEPTH_STEP = 7
# the parameters of the six stages: each moves against the stage before
CLUSTERS = (64, 5, 33, 1, 64, 5)
COMPONENTS = (5, 1, 8, 5, 2, 8)
DEPTHS = (7, 40, 200, 7, 40, 7)                      # the curve's partials grow twice, then the larger buffer serves
META_COLUMNS = (3, 64, 1, 3, 64, 1)
PERMANOVA_P = (9, 99, 1025, 9, 99, 9)
PAIRWISE = (False, True, False, True, False, True)
EDGETEST_P = (9, 1024, 63, 9, 256, 99)               # the edge test's workspace grows in the second stage
EDGETEST_COLUMNS = (1, 4, 2, 2, 3, 2)                 # (from the fourth stage on the last column is one with groups: its
                                                     # maxima are what the next stage's first column finds)
EDGETEST_GROUPS = (2, 5, 32, 2, 4, 32)               # the kG = 2 kernel, the LDS accumulators, again, kG = 2, kG = 4, LDS
SHORT_P = (9, 99, 1025, 9, 9, 9)                     # both P schedules where the full ones take too long


@dataclass
class Stage:
    name: str
    mass: np.ndarray
    best: np.ndarray
    order: tuple
    params: dict
    want: dict = field(default_factory=dict)
    first_half: tuple = None         # "sum": (mass, best) of the first add_cells, and its mirrors in want["half"]


def stage_cells(rng, num_branches, num_samples):
    """name -> (mass, best) of the six stages."""
    s, n = num_samples, num_branches
    dense = random_cells(rng, s, n, empty=1, bits=42)
    bests = [draw_best(rng, s, n, DEPTH_STEP, depths) for depths in DEPTHS]
    # thin: nine cells in ten zeroed, then four rows in ten of those with mass emptied: the lists shrink, every position moves
    thin = sparser(rng, dense)
    with_mass = np.flatnonzero(thin.any(axis=1))
    gone = rng.choice(with_mass, size=(len(with_mass) * 4 + 5) // 10, replace=False)
    thin[gone] = 0
    bests[1][gone] = 0
    two = np.zeros_like(dense)
    two[[3, s - 2]] = dense[[3, s - 2]]
    best_two = np.zeros_like(dense)
    best_two[[3, s - 2]] = bests[3][[0, 1]]
    same = np.zeros_like(dense)
    same[::2] = dense[0]
    best_same = np.zeros_like(dense)
    best_same[::2] = bests[4][0]
    more = random_cells(rng, s, n, empty=2, bits=41)
    cells = {"dense": (dense, bests[0]), "thin": (thin, bests[1]), "zero": (np.zeros_like(dense), np.zeros_like(dense)),
             "two": (two, best_two), "same": (same, best_same), "sum": (dense + more, bests[0] + bests[5])}
    return cells, (dense, bests[0]), (more, bests[5])


def mirrors(mass, best, first, bl, params, only=ANALYSES):
    """name -> the host mirror's answer for these cells and parameters."""
    p, want = params, {}
    if "kr" in only:
        want["kr"] = cohort_mod.kr_host(mass, first, bl)
    for metric in UNIFRAC:               # (not among ANALYSES: the walk leaves them to test_unifrac_gpu; the edge sweep asks)
        if metric in only:
            want[metric] = cohort_mod.unifrac_host(mass, first, bl, metric)
    if "squash" in only:
        want["squash"] = host_all_records(mass, first, bl)
    if "epca" in only:
        want["epca"] = cohort_mod.epca_host(mass, first, p["components"])
    if "kmeans" in only:
        want["kmeans"] = cohort_mod.kmeans_host(mass, first, bl, p["clusters"], 100)
    if "alpha" in only:
        want["alpha"] = cohort_mod.alpha_host(mass, first, bl)
    if "rarefy" in only:
        want["rarefy"] = cohort_mod.rarefy_host(best, first, bl, DEPTH_STEP, p["depths"])
    if "correlation" in only:
        want["correlation"] = cohort_mod.correlation_host(mass, first, p["meta"])
    if "dispersion" in only:
        want["dispersion"] = cohort_mod.dispersion_host(mass, first)
    if "permanova" in only:
        want["permanova"] = cohort_mod.permanova_host(mass, first, bl, p["factors"], p["permanova_p"], p["permanova_seed"], p["pairwise"])
    if "edgetest" in only:
        want["edgetest"] = cohort_mod.edgetest_host(mass, first, p["labels"], p["edgetest_p"], p["edgetest_seed"])
    return want


def stage_params(rng, k, mass, short):
    s = mass.shape[0]
    meta = metadata(rng, mass) if META_COLUMNS[k] <= 3 else wide_metadata(rng, s)
    labels = group_labels(rng, s, EDGETEST_GROUPS[k])[:, :EDGETEST_COLUMNS[k]]
    assert labels.shape[1] == EDGETEST_COLUMNS[k] and len(set(labels[:, 0].tolist())) == EDGETEST_GROUPS[k]
    return {"clusters": CLUSTERS[k], "components": COMPONENTS[k], "depths": DEPTHS[k],
            "meta": np.ascontiguousarray(meta[:, :META_COLUMNS[k]]), "factors": factor_columns(rng, mass, PAIRWISE[k]),
            "permanova_p": (SHORT_P if short else PERMANOVA_P)[k], "pairwise": PAIRWISE[k], "permanova_seed": int(rng.integers(0, 1 << 63)) * 2 + 1,
            "labels": np.ascontiguousarray(labels), "edgetest_p": (SHORT_P if short else EDGETEST_P)[k],
            "edgetest_seed": int(rng.integers(0, 1 << 63)) * 2 + 1}


def defined_families(edgetest):
    return int((~is_na(edgetest.records["family"]["p"])).sum())


WALK = {}                    # the stages of one shape at a time: the variants of a shape follow each other


def walk_of(num_branches, num_samples, short=False):
    """The six stages of a shape with their mirrors, and the conditions that keep the walk from passing vacuously, asserted on
    the mirrors alone."""
    key = (num_branches, num_samples, short)
    if key in WALK:
        return WALK[key]
    WALK.clear()
    parent, bl, first, db = kr_case(num_branches)
    rng = np.random.default_rng(4200 + num_branches + num_samples)
    cells, half_a, half_b = stage_cells(rng, num_branches, num_samples)
    orders = np.random.default_rng(51)
    stages = []
    for k, name in enumerate(STAGES):
        mass, best = cells[name]
        stage = Stage(name, mass, best, tuple(orders.permutation(ANALYSES).tolist()), stage_params(rng, k, mass, short))
        stage.want = mirrors(mass, best, first, bl, stage.params)
        if name == "sum":
            stage.first_half = half_a
            stage.want["half"] = mirrors(*half_a, first, bl, stage.params, only=("kr", "alpha", "dispersion"))
            assert np.array_equal(half_a[0] + half_b[0], mass) and np.array_equal(half_a[1] + half_b[1], best)
        stages.append(stage)
    # every analysis follows at least five different ones (or none) over the six stages
    for a in ANALYSES:
        before = {(st.order[st.order.index(a) - 1] if st.order.index(a) else None) for st in stages}
        assert len(before) >= 5, (a, before)
    used = [int(st.mass.any(axis=1).sum()) for st in stages]
    dense, thin, zero, two, same, total = stages
    s, n = num_samples, num_branches
    assert used == [s - 1, used[1], 0, 2, (s + 1) // 2, s] and 2 * used[1] > s - 1 > used[1] * 3 // 2, used
    if s > COUNT_SAMPLES:                # the used count crosses the limit of the counted ranks, down and up again
        assert used[0] > COUNT_SAMPLES > used[1] and used[5] > COUNT_SAMPLES
    for st in (dense, thin, total):      # defined families of the edge test on more than N branches
        assert defined_families(st.want["edgetest"]) > n, (st.name, defined_families(st.want["edgetest"]))
        assert int(st.want["kmeans"].info["converged"]) == 1 and int(st.want["epca"].info["converged"]) == 1
    whole = lambda st: st.want["permanova"].records[0, 0]
    assert int(whole(dense)["used"]) == s - 1 > int(whole(thin)["used"]) == used[1] >= int(whole(thin)["groups"]) + 1
    assert not is_na(whole(dense)["p"]) and not is_na(whole(thin)["p"]) and not is_na(whole(total)["p"])
    assert not is_na(thin.want["permanova"].records["p"][:, 1:]).all()                 # some pair of groups is tested
    # zero: every analysis's "nothing"
    w = zero.want
    assert (w["kr"] == np.where(np.eye(s, dtype=bool), 0.0, -1.0)).all() and w["squash"][1] == 0
    assert int(w["epca"].info["used"]) == 0 and int(w["epca"].info["components"]) == 0
    assert int(w["kmeans"].info["used"]) == 0 and (w["kmeans"].samples["cluster"] == capi.KMEANS_NONE).all()
    assert (w["rarefy"] == -1.0).all() and not w["correlation"][1].any() and is_na(w["correlation"][0].view(np.float64)).all()
    assert is_na(w["dispersion"].view(np.float64)).all() and is_na(w["permanova"].records["p"]).all()
    assert not w["permanova"].records["used"].any() and defined_families(w["edgetest"]) == 0
    assert not w["edgetest"].records["used"].any() and is_na(w["edgetest"].max).all()
    # two: two used samples, nothing to test
    w = two.want
    assert int(w["epca"].info["used"]) == 2 and int(w["kmeans"].info["used"]) == 2 and w["squash"][1] == 1
    assert defined_families(w["edgetest"]) == 0 and w["edgetest"].records["used"].max() == 2
    assert is_na(w["permanova"].records["p"]).all()
    # same: identical samples; the ranks tie throughout; some branches defined and some not
    w = same.want
    fam = ~is_na(w["edgetest"].records["family"]["p"])
    assert fam[..., 0].any() and not fam[..., 0].all() and fam[..., 2].any() and not fam[..., 1].any() and not fam[..., 3].any()
    assert int(w["edgetest"].records["used"].max()) == (s + 1) // 2
    assert (w["kr"][::2, ::2] == 0.0).all()
    WALK[key] = (parent, bl, first, db, stages)
    return WALK[key]


def device_kr_raw(pl, cohort, tree, bl):
    """kr_device into a poisoned buffer on a stream of its own."""
    import torch
    s = cohort.num_samples
    d_out = torch.full((s * s * 8,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    cohort.kr_device(tree, bl, d_out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.float64).reshape(s, s).copy()


def run_analysis(name, pl, cohort, tree, bl, params, want, what):
    """One analysis into poisoned buffers on a stream of its own, against its mirror: every byte."""
    import torch
    p = params
    if name == "kr":
        got = device_kr_raw(pl, cohort, tree, bl)
        assert same_bits(got, want), (what, np.argwhere(got.view(U64) != want.view(U64))[:8])
    elif name in UNIFRAC:
        _, got = device_matrix(pl, cohort, tree, bl, name)
        assert same_bits(got, want), (what, np.argwhere(got.view(U64) != want.view(U64))[:8])
    elif name == "squash":
        records, count = device_all_records(pl, cohort, tree, bl, torch.cuda.Stream())
        assert count == want[1] and records.tobytes() == want[0].tobytes(), (what, count, want[1])
    elif name == "epca":
        assert_epca(device_epca_raw(pl, cohort, tree, p["components"], torch.cuda.Stream()), want, what)
    elif name == "kmeans":
        assert_kmeans(device_kmeans_raw(pl, cohort, tree, bl, p["clusters"], 100, torch.cuda.Stream()), want, what)
    elif name == "alpha":
        assert same_records(device_alpha_raw(pl, cohort, tree, bl), want), what
    elif name == "rarefy":
        got = device_rarefy_raw(pl, cohort, tree, bl, DEPTH_STEP, p["depths"])
        assert same_bits(got, want), (what, np.argwhere(got.view(U64) != want.view(U64))[:8])
    elif name == "correlation":
        assert_correlation(device_correlation_raw(pl, cohort, tree, p["meta"]), want, what)
    elif name == "dispersion":
        assert same_records(device_dispersion_raw(pl, cohort, tree), want), what
    elif name == "permanova":
        got, kr_before, kr_after = device_permanova_raw(pl, cohort, tree, bl, p["factors"], p["permanova_p"], p["permanova_seed"], p["pairwise"])
        same_permanova(got, want, what)
        assert same_bits(kr_before, kr_after), what
    else:
        got = device_edgetest_raw(pl, cohort, tree, p["labels"], p["edgetest_p"], p["edgetest_seed"], cohort.num_branches)
        same_edgetest(got, want, what)


def assert_holds(cohort, mass, best, what):
    cells = cohort.read()
    assert np.array_equal(cells.mass, mass) and np.array_equal(cells.best, best), what
    assert not cells.totals.view(U64).any() and cells.bad_samples == 0, what


# S = 70 pads to 96: 26 padding samples, a wave, two tiles of 32 and the 16-tiles of k-means crossed; S = 130 crosses the
# counted ranks both ways.  (999, 70) comes last: the two-stream test shares its stages
SHAPES = ((7, 70), (999, 130), (999, 70))
VARIANTS = {"as created": {}, "the general paths": {switch: "0" for switch in SWITCHES}, "two workgroups": {"EPIK_AMD_MAX_BLOCKS": "2"}}
WALKS = [(n, s, v) for n, s in SHAPES for v in VARIANTS if v == "as created" or s == 70]


@pytest.mark.parametrize("num_branches, num_samples, variant", WALKS, ids=[f"{n}-{s}-{v.replace(' ', '_')}" for n, s, v in WALKS])
def test_every_analysis_after_the_cells_change(placer_cls, monkeypatch, num_branches, num_samples, variant):
    for var in ENV + SWITCHES:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db, stages = walk_of(num_branches, num_samples)
    for key, value in VARIANTS[variant].items():
        monkeypatch.setenv(key, value)
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(num_samples) as cohort:
        for stage in stages:
            if stage.name == "sum":
                # the cells change without a reset: the first half, three analyses on it, then the second half on top
                cohort.reset()
                cohort.add_cells(*stage.first_half, None)
                assert_holds(cohort, *stage.first_half, (variant, stage.name, "the first half"))
                for name in ("alpha", "kr", "dispersion"):
                    run_analysis(name, pl, cohort, tree, bl, stage.params, stage.want["half"][name], (variant, "the first half", name))
                cohort.add_cells(stage.mass - stage.first_half[0], stage.best - stage.first_half[1], None)
            else:
                cohort.reset()
                if stage.name != "zero":
                    cohort.add_cells(stage.mass, stage.best, None)
            assert_holds(cohort, stage.mass, stage.best, (variant, stage.name))
            for name in stage.order:
                run_analysis(name, pl, cohort, tree, bl, stage.params, stage.want[name], (variant, stage.name, name))
            assert_holds(cohort, stage.mass, stage.best, (variant, stage.name, "after"))


def test_device_entries_back_to_back_on_two_streams(placer_cls, monkeypatch):
    """kr, permanova, edgetest, correlation, kmeans, rarefy, squash, epca, alpha and dispersion, alternating between two
    non-blocking streams with no host synchronisation between the calls: each entry drains the device before it touches a
    workspace that the one before may still read or write."""
    import torch
    for var in ENV + SWITCHES:
        monkeypatch.delenv(var, raising=False)
    n, s = 999, 70
    parent, bl, first, db, stages = walk_of(n, s)
    mass, best = stages[0].mass, stages[0].best
    p = dict(stages[1].params)           # the parameters of the second stage on the cells of the first
    want = mirrors(mass, best, first, bl, p)
    m_cor, m_per, m_edge = p["meta"].shape[1], p["factors"].shape[1], p["labels"].shape[1]
    slots = SLOTS if p["pairwise"] else 1
    rows = (p["permanova_p"] + 1, p["edgetest_p"] + 1)
    k, comps, depths = p["clusters"], p["components"], p["depths"]
    sizes = {"kr": s * s * 8, "permanova": m_per * slots * 56, "ssw": m_per * slots * rows[0] * 8, "group_ss": m_per * 256 * 8,
             "edgetest": m_edge * n * 208, "stat": m_edge * 4 * n * rows[1] * 8, "max": m_edge * 4 * rows[1] * 8,
             "correlation": m_cor * n * 32, "used": m_cor * 4, "samples": s * 16, "clusters": k * 24, "centroids": k * n * 8,
             "kmeans_info": 16, "rarefy": s * depths * 16, "merges": (s - 1) * 32, "num_merges": 4, "mu": comps * 8,
             "proj": s * comps * 8, "edge": comps * n * 8, "epca_info": 32, "alpha": s * 40, "dispersion": n * 64}
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(s) as cohort:
        cohort.add_cells(mass, best, None)
        d = {name: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}") for name, nbytes in sizes.items()}
        at = {name: buf.data_ptr() for name, buf in d.items()}
        streams = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        a, b = streams[0].cuda_stream, streams[1].cuda_stream
        assert a != b and 0 not in (a, b)
        cohort.kr_device(tree, bl, at["kr"], a)
        cohort.permanova_device(at["kr"], p["factors"], p["permanova_p"], p["permanova_seed"], p["pairwise"], at["permanova"], at["ssw"],
                                at["group_ss"], b)
        cohort.edgetest_device(tree, p["labels"], p["edgetest_p"], p["edgetest_seed"], at["edgetest"], at["stat"], at["max"], a)
        cohort.correlation_device(tree, p["meta"], at["correlation"], at["used"], b)
        cohort.kmeans_device(tree, bl, k, 100, at["samples"], at["clusters"], at["centroids"], at["kmeans_info"], a)
        cohort.rarefy_device(tree, bl, DEPTH_STEP, depths, at["rarefy"], b)
        cohort.squash_device(tree, bl, at["merges"], at["num_merges"], a)
        cohort.epca_device(tree, comps, at["mu"], at["proj"], at["edge"], at["epca_info"], b)
        cohort.alpha_device(tree, bl, at["alpha"], a)
        cohort.dispersion_device(tree, at["dispersion"], b)
        torch.cuda.synchronize()
        h = {name: buf.cpu().numpy() for name, buf in d.items()}
        assert_holds(cohort, mass, best, "after the ten")
    f64 = lambda name, *shape: h[name].view(np.float64).reshape(*shape)
    assert same_bits(f64("kr", s, s), want["kr"])
    same_permanova(cohort_mod.Permanova(h["permanova"].view(capi.PERMANOVA).reshape(m_per, slots), f64("ssw", m_per, slots, rows[0]),
                                        f64("group_ss", m_per, 256)), want["permanova"], "permanova")
    same_edgetest(cohort_mod.Edgetest(h["edgetest"].view(capi.EDGETEST).reshape(m_edge, n), f64("stat", m_edge, 4, n, rows[1]),
                                      f64("max", m_edge, 4, rows[1])), want["edgetest"], "edgetest")
    assert_correlation((h["correlation"].view(capi.CORRELATION).reshape(m_cor, n), h["used"].view(np.uint32)), want["correlation"], "correlation")
    assert_kmeans((h["samples"].view(capi.KMEANS_SAMPLE), h["clusters"].view(capi.KMEANS_CLUSTER), f64("centroids", k, n),
                   h["kmeans_info"].view(capi.KMEANS_INFO)[0]), want["kmeans"], "kmeans")
    assert same_bits(f64("rarefy", s, depths, 2), want["rarefy"])
    assert int(h["num_merges"].view(np.uint32)[0]) == want["squash"][1] and h["merges"].tobytes() == want["squash"][0].tobytes()
    assert_epca((f64("mu", comps), f64("proj", s, comps), f64("edge", comps, n), h["epca_info"].view(capi.EPCA_INFO)[0]), want["epca"], "epca")
    # (a cell that was not written still holds the poison, which no mirror gives)
    assert same_records(h["alpha"].view(capi.ALPHA), want["alpha"]) and same_records(h["dispersion"].view(capi.DISPERSION), want["dispersion"])
