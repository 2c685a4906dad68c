"""Phylogenetic k-means of a cohort's samples, no device: the rule of include/epik_amd.h restated here in numpy against
epik_amd_cohort_kmeans_host -- every byte of the sample records, the cluster records, the centroids and the info block --,
a case derived by hand, forged and planted cohorts, properties on random cohorts, the C ABI's refusals, the drivers' and
the launcher's flags, the two files and the stand-alone host binary (plain and under ASan + UBSan).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod
from test_capi_cpu import _header_symbols
from test_cohort_cpu import host_bins, numpy_first, random_cells, same_bits, tree_case  # noqa: F401 (host_bins: a fixture)
from test_epca_cpu import sequential_sum
from test_squash_cpu import BALANCED, numpy_planes, sequential_kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
NONE = 0xFFFFFFFF


# ---- the rule, restated ----------------------------------------------------------------------------------------------
def numpy_kmeans(mass, first, branch_length, num_clusters, max_iterations):
    """(samples, clusters, centroids, info, D) by the header's text; D [L][K'] is the last step 1's."""
    mass = np.asarray(mass, dtype=U64)
    s, n = mass.shape
    k_all = int(num_clusters)
    c_all, b_all, total = numpy_planes(mass, first)
    half = 0.5 * np.asarray(branch_length, dtype=np.float64)
    used = np.flatnonzero(total > 0)
    count = len(used)
    kc = min(k_all, count)
    samples = np.zeros(s, dtype=capi.KMEANS_SAMPLE)
    samples["cluster"], samples["dist"] = NONE, -1.0
    clusters = np.zeros(k_all, dtype=capi.KMEANS_CLUSTER)
    clusters["seed"] = NONE
    centroids = np.zeros((k_all, n))
    info = np.zeros(1, dtype=capi.KMEANS_INFO)
    info[0] = (0, 0, 0, 1)
    if count == 0:
        return samples, clusters, centroids, info[0], np.zeros((0, 0))
    c, b = c_all[used], b_all[used]
    # the average of the members' planes: the sum over the members in ascending j from +0.0, one division
    average = lambda rows: (sequential_sum(c[rows], 0) / np.float64(len(rows)), sequential_sum(b[rows], 0) / np.float64(len(rows)))
    # the seeding: nearest the grand mean, then farthest first
    centres = [int(np.argmin(sequential_kr(*average(np.arange(count)), c, b, half)))]   # (argmin: the first of the smallest)
    mind = sequential_kr(c[centres[0]], b[centres[0]], c, b, half)
    for _ in range(1, kc):
        candidates = mind.copy()
        candidates[centres] = -1.0                                                  # (a distance is >= 0: 0 still qualifies)
        centres.append(int(np.argmax(candidates)))                                  # (argmax: the first of the largest)
        mind = np.minimum(mind, sequential_kr(c[centres[-1]], b[centres[-1]], c, b, half))
    cc, cb = c[centres].copy(), b[centres].copy()
    assign = np.full(count, -1)
    iterations = 0
    while True:
        iterations += 1
        d = np.stack([sequential_kr(cc[k], cb[k], c, b, half) for k in range(kc)], axis=1)
        new = np.argmin(d, axis=1)
        changed = int((new != assign).sum())
        assign = new
        if changed == 0 or iterations == max_iterations:
            break
        for k in range(kc):
            members = np.flatnonzero(assign == k)
            if len(members):
                cc[k], cb[k] = average(members)
    dist = d[np.arange(count), assign]
    samples["cluster"][used], samples["dist"][used] = assign, dist
    for k in range(kc):
        members = np.flatnonzero(assign == k)
        clusters[k] = (len(members), used[centres[k]], sequential_sum(dist[members], 0), sequential_sum(dist[members] * dist[members], 0))
    centroids[:kc] = cc - cb
    info[0] = (count, kc, iterations, int(changed == 0))
    return samples, clusters, centroids, info[0], d


def as_parts(x):
    return (x.samples, x.clusters, x.centroids, x.info) if isinstance(x, cohort_mod.Kmeans) else tuple(x)[:4]


def assert_kmeans(got, want, what=""):
    """Every byte of the four outputs; `got` and `want` are tuples or `cohort.Kmeans`."""
    (samples, clusters, centroids, info), (w_samples, w_clusters, w_centroids, w_info) = as_parts(got), as_parts(want)
    assert np.asarray(info).tobytes() == np.asarray(w_info).tobytes(), (what, info, w_info)
    assert samples.tobytes() == w_samples.tobytes(), (what, samples, w_samples)
    assert clusters.tobytes() == w_clusters.tobytes(), (what, clusters, w_clusters)
    assert same_bits(centroids, w_centroids), (what, np.argwhere(np.asarray(centroids).view(U64) != np.asarray(w_centroids).view(U64))[:5])


def planted_cells(num_samples, groups, num_branches):
    """Samples drawn around `groups` centres, sample i of group i % groups, sample 4 emptied."""
    rng = np.random.default_rng(77 + num_samples + groups)
    centres = rng.dirichlet(np.full(num_branches, 0.05), size=groups)
    mass = np.stack([rng.multinomial(20_000, centres[i % groups]) for i in range(num_samples)]).astype(U64) << U64(20)
    if num_samples > 4:
        mass[4] = 0
    return mass


CELLS = {}


def cells_case(tree_name, num_samples):
    """(mass, first, branch_length) of a case of the first test."""
    key = (tree_name, num_samples)
    if key not in CELLS:
        parent, bl = tree_case(tree_name)
        CELLS[key] = (random_cells(np.random.default_rng(4000 + num_samples), num_samples, len(parent), empty=1, bits=42),
                      numpy_first(parent), bl)
    return CELLS[key]


@pytest.mark.parametrize("tree_name", ["one", "tree15", "tree2999"])
@pytest.mark.parametrize("num_samples", [1, 2, 3, 4, 33, 34, 70])
def test_kmeans_host_equals_the_numpy_restatement_bit_for_bit(tree_name, num_samples):
    mass, first, bl = cells_case(tree_name, num_samples)
    used = int((mass.sum(axis=1, dtype=U64) > 0).sum())
    for k in (1, 2, 5, 33, 64):
        for max_iterations in (1, 100):
            want = numpy_kmeans(mass, first, bl, k, max_iterations)
            got = cohort_mod.kmeans_host(mass, first, bl, k, max_iterations)
            assert_kmeans(got, want, (tree_name, num_samples, k, max_iterations))
            assert int(got.info["used"]) == used and got.num_clusters == min(k, used)
            if used:
                assert int(got.info["converged"]) == (0 if max_iterations == 1 else 1), (k, got.info)
                assert int(got.info["iterations"]) == 1 if max_iterations == 1 else 2 <= int(got.info["iterations"]) < 100


# ---- a case by hand --------------------------------------------------------------------------------------------------
def test_five_samples_on_the_balanced_tree_by_hand():
    # ((0,1)2,(3,4)5)6, every length 1, so 0.5 * bl = 0.5.  s0 = 9 on leaf 0, s1 = 4 on leaf 3, s2 empty, s3 = 2 on leaf 0,
    # s4 = 6 on leaf 4: the used samples j = 0 .. 3 are s0, s1, s3, s4.  A sample on leaf 0 has C = 1 on branches 0, 2, 6
    # and B = 1 on 2, 6; on leaf 3: C = 1 on 3, 5, 6 and B = 1 on 5, 6; on leaf 4: C = 1 on 4, 5, 6 and B = 1 on 5, 6.
    # KR(leaf 0, leaf 3) = 0.5 * (1 [b0] + 2 [b2] + 1 [b3] + 2 [b5]) = 3, KR(leaf 3, leaf 4) = 0.5 * (1 + 1) = 1, and s3 is
    # a copy of s0.  The grand mean M holds 1/2 on leaf 0 and 1/4 on each of leaves 3 and 4:
    #   C = (.5, 0, .5, .25, .25, .5, 1), B = (0, 0, .5, 0, 0, .5, 1);
    #   KR(M, s0) = 0.5 * (.5 + 1 + .25 + .25 + 1) = 1.5,  KR(M, s1) = 0.5 * (.5 + 1 + .75 + .25 + 1) = 1.75 = KR(M, s4).
    # Centre 0 is j = 0 (s0), the first of the smallest; mind = (0, 3, 0, 3).  Centre 1 is j = 1 (s1), the first of the
    # largest; mind = min(., (3, 0, 3, 1)) = (0, 0, 0, 1).  Centre 2 is j = 3 (s4); mind = 0 everywhere.  Centre 3 is the
    # only sample left, j = 2 (s3).
    # K = 1: iteration 1 puts everyone with s0's planes (changed = 4), the update makes the centroid M; iteration 2 gives
    #   (1.5, 1.75, 1.5, 1.75) and changes nothing.
    # K = 2: iteration 1: (0, 1, 0, 1) by D = ((0, 3), (3, 0), (0, 3), (3, 1)); centroid 1 becomes 1/2 on each of leaves 3, 4
    #   and KR(s1, it) = 0.5 * (.5 + .5) = 0.5 = KR(s4, it), while it is 3 from s0: iteration 2 changes nothing.
    # K = 3: everyone is a centre or a copy of one: all distances 0.  K >= 4: K' = 4; s3 seeds cluster 3 but lies at 0 from
    #   cluster 0 too, and the first smallest wins: cluster 3 stays empty and keeps s3's planes.
    first = numpy_first(BALANCED)
    bl = np.ones(7)
    mass = np.zeros((5, 7), U64)
    mass[0, 0], mass[1, 3], mass[3, 0], mass[4, 4] = 9, 4, 2, 6
    table = {1: ([0, 0, 0, 0], [1.5, 1.75, 1.5, 1.75], [0]),
             2: ([0, 1, 0, 1], [0, 0.5, 0, 0.5], [0, 1]),
             3: ([0, 1, 0, 2], [0, 0, 0, 0], [0, 1, 4]),
             4: ([0, 1, 0, 2], [0, 0, 0, 0], [0, 1, 4, 3]),
             64: ([0, 1, 0, 2], [0, 0, 0, 0], [0, 1, 4, 3])}
    for k, (cluster, dist, seeds) in table.items():
        got = cohort_mod.kmeans_host(mass, first, bl, k)
        assert_kmeans(got, numpy_kmeans(mass, first, bl, k, 100), k)
        assert tuple(got.info.tolist()) == (4, min(k, 4), 2, 1), (k, got.info)
        assert list(got.samples["cluster"]) == cluster[:2] + [NONE] + cluster[2:], k
        assert same_bits(got.samples["dist"], dist[:2] + [-1.0] + dist[2:]), k
        assert list(got.clusters["seed"]) == seeds + [NONE] * (k - len(seeds)), k
        sizes = [cluster.count(i) for i in range(len(seeds))]
        assert list(got.clusters["size"]) == sizes + [0] * (k - len(seeds)), k
        sums = [sum(d for c, d in zip(cluster, dist) if c == i) for i in range(len(seeds))]
        squares = [sum(d * d for c, d in zip(cluster, dist) if c == i) for i in range(len(seeds))]
        assert same_bits(got.clusters["sum_dist"], sums + [0.0] * (k - len(seeds))), k
        assert same_bits(got.clusters["sum_sq"], squares + [0.0] * (k - len(seeds))), k
        assert not got.centroids[len(seeds):].view(U64).any()
    leaf = lambda *pairs: [dict(pairs).get(b, 0.0) for b in range(7)]
    assert same_bits(cohort_mod.kmeans_host(mass, first, bl, 1).centroids, [leaf((0, 0.5), (3, 0.25), (4, 0.25))])
    assert same_bits(cohort_mod.kmeans_host(mass, first, bl, 2).centroids, [leaf((0, 1.0)), leaf((3, 0.5), (4, 0.5))])
    assert same_bits(cohort_mod.kmeans_host(mass, first, bl, 4).centroids, [leaf((0, 1.0)), leaf((3, 1.0)), leaf((4, 1.0)), leaf((0, 1.0))])


# ---- forged cohorts --------------------------------------------------------------------------------------------------
def forged_kmeans_cohorts():
    """name -> (mass, parent, branch_length, K)"""
    parent, bl = tree_case("tree15")
    n = len(parent)
    rng = np.random.default_rng(44)
    x, y, z = (random_cells(rng, 1, n, bits=42)[0] for _ in range(3))
    zero = np.zeros(n, U64)
    one_parent, one_bl = tree_case("one")
    hand = np.zeros((5, 7), U64)
    hand[0, 0], hand[1, 3], hand[3, 0], hand[4, 4] = 9, 4, 2, 6
    cases = {
        "all empty": (np.stack([zero, zero, zero]), parent, bl, 5),
        "one used sample": (np.stack([zero, x, zero]), parent, bl, 5),
        "all identical": (np.stack([x, x, x, x]), parent, bl, 3),
        "more clusters than samples": (np.stack([x, zero, y, z]), parent, bl, 64),
        "the empty cluster keeps its seed": (hand, BALANCED, np.ones(7), 4),
        "the tree of one branch": (random_cells(rng, 5, 1, bits=42) + U64(1), one_parent, one_bl, 3),
    }
    for k in (2, 3, 4):
        cases[f"two identical pairs, K = {k}"] = (np.stack([x, y, x, y]), parent, bl, k)
    return cases


@pytest.mark.parametrize("name", sorted(forged_kmeans_cohorts()))
def test_forged_cohorts(name):
    mass, parent, bl, k = forged_kmeans_cohorts()[name]
    first = numpy_first(parent)
    want = numpy_kmeans(mass, first, bl, k, 100)
    got = cohort_mod.kmeans_host(mass, first, bl, k, 100)
    assert_kmeans(got, want, name)
    info, samples, clusters = tuple(got.info.tolist()), got.samples, got.clusters
    if name == "all empty":
        assert info == (0, 0, 0, 1) and (samples["cluster"] == NONE).all() and (samples["dist"] == -1.0).all()
        assert (clusters["seed"] == NONE).all() and not clusters["size"].any() and not got.centroids.view(U64).any()
    elif name == "one used sample":
        assert info == (1, 1, 2, 1) and list(samples["cluster"]) == [NONE, 0, NONE] and samples["dist"][1] == 0.0
        assert list(clusters["size"]) == [1, 0, 0, 0, 0] and list(clusters["seed"]) == [1] + [NONE] * 4
    elif name == "all identical":          # x + x + x + x and its quarter are exact: everyone at 0 from cluster 0
        assert info == (4, 3, 2, 1) and not samples["cluster"].any() and not samples["dist"].view(U64).any()
        assert list(clusters["size"]) == [4, 0, 0] and list(clusters["seed"]) == [0, 1, 2]
    elif name == "more clusters than samples":
        assert info == (3, 3, 2, 1) and sorted(samples["cluster"][[0, 2, 3]]) == [0, 1, 2] and not samples["dist"][[0, 2, 3]].any()
        assert (clusters["size"][:3] == 1).all() and not clusters["size"][3:].any() and (clusters["seed"][3:] == NONE).all()
    elif name == "the empty cluster keeps its seed":
        assert list(clusters["size"]) == [2, 1, 1, 0] and list(clusters["seed"]) == [0, 1, 4, 3]
        assert same_bits(got.centroids[3], got.centroids[0]) and got.centroids[3, 0] == 1.0
    elif name == "the tree of one branch":  # every used sample has C = 1, B = 0: all identical
        assert info == (5, 3, 2, 1) and not samples["cluster"].any() and not samples["dist"].view(U64).any()
    else:                                   # x, y, x, y: two points; a third and a fourth cluster are seeded by the copies
        assert info == (4, min(k, 4), 2, 1) and list(samples["cluster"]) == [0, 1, 0, 1] and not samples["dist"].view(U64).any()
        assert list(clusters["size"]) == [2, 2, 0, 0][:k] and sorted(clusters["seed"][:2]) == [0, 1]


# ---- planted cohorts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree_name", ["tree15", "tree2999"])
@pytest.mark.parametrize("num_samples,groups", [(7, 3), (34, 3), (70, 4), (70, 7)])
def test_planted_groups_are_recovered(tree_name, num_samples, groups):
    parent, bl = tree_case(tree_name)
    first = numpy_first(parent)
    mass = planted_cells(num_samples, groups, len(parent))
    got = cohort_mod.kmeans_host(mass, first, bl, groups)
    assert_kmeans(got, numpy_kmeans(mass, first, bl, groups, 100), (tree_name, num_samples, groups))
    assert tuple(got.info.tolist()) == (num_samples - 1, groups, 2, 1)
    cluster = got.samples["cluster"]
    assert cluster[4] == NONE
    used = np.flatnonzero(cluster != NONE)
    # the clusters are exactly the groups: the same partition
    assert len({(int(cluster[i]), i % groups) for i in used}) == groups and len(set(cluster[used].tolist())) == groups


# ---- properties on random cohorts ------------------------------------------------------------------------------------
def test_properties_on_random_cohorts():
    for tree_name, num_samples, k in (("tree15", 33, 5), ("tree2999", 34, 2), ("tree2999", 70, 33), ("tree15", 70, 64)):
        mass, first, bl = cells_case(tree_name, num_samples)
        samples, clusters, centroids, info, d = numpy_kmeans(mass, first, bl, k, 100)
        got = cohort_mod.kmeans_host(mass, first, bl, k, 100)
        assert_kmeans(got, (samples, clusters, centroids, info))
        count, kc = int(got.info["used"]), got.num_clusters
        assert int(got.clusters["size"].sum()) == count and int(got.info["converged"]) == 1
        used = got.samples["cluster"] != NONE
        assert same_bits(got.samples["dist"][used], d.min(axis=1)) and d.shape == (count, kc)
        assert (got.samples["cluster"][used] == d.argmin(axis=1)).all()
        # a centroid is a mass distribution: its cells are >= 0 (C >= B in every member, and sums, rounding and division
        # are monotone) and sum to 1.  Every plane value is at most 1 and carries one rounding of its own, at most `count`
        # of the sum and one of the division, each 2^-53 relative; a cell is the difference of two such values and
        # rounds once more, and numpy's sum of the N cells adds at most N * 2^-53: N * (count + 3) * 2^-52 in all.
        assert (got.centroids >= 0).all()
        assert np.abs(got.centroids[:kc].sum(axis=1) - 1.0).max() <= len(first) * (count + 3) * 2.0 ** -52
        # K = 1: the one centroid is the grand mean M and dist is KR(M, j)
        one = cohort_mod.kmeans_host(mass, first, bl, 1, 100)
        c, b, total = numpy_planes(mass, first)
        c, b = c[total > 0], b[total > 0]
        mc, mb = sequential_sum(c, 0) / np.float64(count), sequential_sum(b, 0) / np.float64(count)
        assert same_bits(one.samples["dist"][used], sequential_kr(mc, mb, c, b, 0.5 * bl)) and same_bits(one.centroids[0], mc - mb)
        assert tuple(one.info.tolist()) == (count, 1, 2, 1)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_kmeans_symbols_exist_and_refuse_what_the_header_says():
    lib = capi.load()
    for name in ("epik_amd_cohort_kmeans_device", "epik_amd_cohort_kmeans", "epik_amd_cohort_kmeans_host"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == _header_symbols() and capi.ABI_VERSION == 3
    assert (capi.KMEANS_INFO.itemsize, capi.KMEANS_SAMPLE.itemsize, capi.KMEANS_CLUSTER.itemsize) == (16, 16, 24)
    assert [capi.KMEANS_SAMPLE.fields[k][1] for k in ("cluster", "zero", "dist")] == [0, 4, 8]
    assert [capi.KMEANS_CLUSTER.fields[k][1] for k in ("size", "seed", "sum_dist", "sum_sq")] == [0, 4, 8, 16]
    assert (capi.KMEANS_MAX_CLUSTERS, capi.KMEANS_MAX_ITERATIONS, capi.KMEANS_NONE) == (64, 1000, NONE)
    err = lambda: lib.epik_amd_last_error().decode()
    info = np.zeros(1, dtype=capi.KMEANS_INFO)
    assert lib.epik_amd_cohort_kmeans_device(None, None, None, 2, 100, None, None, None, None, None) == capi.ERR_INVALID and "null cohort" in err()
    assert lib.epik_amd_cohort_kmeans(None, None, None, 2, 100, None, None, None, info.ctypes.data) == capi.ERR_INVALID and "null cohort" in err()
    first = cohort_mod.first_of([2, 2, -1])
    mass = np.ones((2, 3), U64)
    bl = np.ones(3)
    samples, clusters, centroids = np.zeros(2, capi.KMEANS_SAMPLE), np.zeros(64, capi.KMEANS_CLUSTER), np.zeros((64, 3))
    host = lib.epik_amd_cohort_kmeans_host
    args = lambda m=mass, s=2, n=3, f=first, l=bl, k=2, it=100, a=samples, c=clusters, e=centroids, i=info: (
        m.ctypes.data if m is not None else None, s, n, f.ctypes.data if f is not None else None,
        l.ctypes.data if l is not None else None, k, it, *(x.ctypes.data if x is not None else None for x in (a, c, e, i)))
    assert host(*args()) == capi.OK and tuple(info[0].tolist()) == (2, 2, 2, 1)
    assert host(*args(k=64, it=1000)) == capi.OK and host(*args(k=1, it=1)) == capi.OK
    for bad in (0, 65, 0xFFFFFFFF):
        assert host(*args(k=bad)) == capi.ERR_INVALID and "num_clusters" in err() and "[1, 64]" in err()
    for bad in (0, 1001, 0xFFFFFFFF):
        assert host(*args(it=bad)) == capi.ERR_INVALID and "max_iterations" in err() and "[1, 1000]" in err()
    assert host(*args(s=0)) == capi.ERR_INVALID and "num_samples is 0" in err()
    assert host(*args(n=0)) == capi.ERR_INVALID
    for missing in ("m", "f", "l", "a", "c", "e", "i"):
        assert host(*args(**{missing: None})) == capi.ERR_INVALID and "null argument" in err(), missing
    above = np.array([0, 2, 0], dtype=np.uint32)
    assert host(*args(f=above)) == capi.ERR_INVALID and "branch 1" in err() and "first" in err()
    for bad in (-1.0, np.inf, np.nan):
        assert host(*args(l=np.array([1.0, 1.0, bad]))) == capi.ERR_INVALID and "branch 2" in err() and "length" in err()
    for k, it in ((0, 100), (65, 100), (2, 0), (2, 1001)):
        with pytest.raises(capi.EpikAmdError):
            cohort_mod.kmeans_host(mass, first, bl, k, it)
    with pytest.raises(ValueError):
        cohort_mod.kmeans_host(mass, first[:2], bl, 2)


# ---- the drivers and the launcher ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_drivers_refuse_kmeans_without_cohort_and_name_the_flag(host_bins, tmp_path, binary):
    base = [os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "none.list"), "-o", str(tmp_path)]
    for extra, flag, needs in ((["--cohort-kmeans", "3"], "--cohort-kmeans", "--cohort "),
                               (["--cohort-kmeans", "3", "--cohort-kmeans-iterations", "9"], "--cohort-kmeans", "--cohort "),
                               (["--cohort", "--cohort-kmeans-iterations", "9"], "--cohort-kmeans-iterations", "--cohort-kmeans "),
                               (["--cohort", "--cohort-kmeans", "0"], "--cohort-kmeans ", "[1, 64]"),
                               (["--cohort", "--cohort-kmeans", "65"], "--cohort-kmeans ", "[1, 64]"),
                               (["--cohort", "--cohort-kmeans", "x"], "--cohort-kmeans ", "[1, 64]"),
                               (["--cohort", "--cohort-kmeans=-3"], "--cohort-kmeans ", "[1, 64]"),
                               (["--cohort", "--cohort-kmeans", "3", "--cohort-kmeans-iterations", "0"], "--cohort-kmeans-iterations", "[1, 1000]"),
                               (["--cohort", "--cohort-kmeans", "3", "--cohort-kmeans-iterations", "1001"], "--cohort-kmeans-iterations", "[1, 1000]"),
                               (["--cohort", "--cohort-kmeans", "3", "--cohort-kmeans-iterations", "2x"], "--cohort-kmeans-iterations", "[1, 1000]")):
        run = subprocess.run(base + extra, capture_output=True, text=True)
        assert run.returncode == 255, run.stdout + run.stderr
        assert run.stderr.startswith("Error:") and flag in run.stderr and needs in run.stderr, (extra, run.stderr)
        assert "Loading database" not in run.stdout and "HIP device" not in run.stderr and not list(tmp_path.iterdir())
    out = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort-kmeans arg" in out.stdout and "--cohort-kmeans-iterations" in out.stdout
    assert "cohort_kmeans_<list>.tsv" in out.stdout and "cohort_kmeans_centroids_<list>.tsv" in out.stdout


def test_launcher_passes_the_flags_only_when_given():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw)
    assert "--cohort-kmeans" not in " ".join(default)
    assert epik.driver_command(**kw, cohort_kmeans=None, cohort_kmeans_iterations=None) == default
    assert "--cohort-kmeans" not in " ".join(epik.driver_command(**kw, cohort=True))
    assert epik.driver_command(**kw, cohort=True, cohort_kmeans=3)[:-1] == default[:-1] + ["--cohort", "--cohort-kmeans", "3"]
    assert epik.driver_command(**kw, cohort=True, cohort_kmeans=3, cohort_kmeans_iterations=7)[:-1] == \
        default[:-1] + ["--cohort", "--cohort-kmeans", "3", "--cohort-kmeans-iterations", "7"]
    assert epik.driver_command(**kw, cohort=True, cohort_squash=True, cohort_epca=True, cohort_kmeans=2)[:-1] == \
        default[:-1] + ["--cohort", "--cohort-squash", "--cohort-epca", "--cohort-kmeans", "2"]
    with pytest.raises(click.UsageError):
        epik.driver_command(**kw, cohort_kmeans=3)
    with pytest.raises(click.UsageError):
        epik.driver_command(**kw, cohort=True, cohort_kmeans_iterations=3)
    me = os.path.join(ROOT, "epik.py")
    out = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort-kmeans" in out.stdout and "--cohort-kmeans-iterations" in out.stdout
    run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, "--cohort-kmeans", "3", me], capture_output=True, text=True)
    assert run.returncode == 2 and "--cohort" in run.stderr, (run.stdout, run.stderr)
    for bad in (["--cohort-kmeans", "65"], ["--cohort-kmeans", "3", "--cohort-kmeans-iterations", "0"]):
        run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, "--cohort", *bad, me], capture_output=True, text=True)
        assert run.returncode == 2 and bad[-2] in run.stderr, (run.stdout, run.stderr)


def test_the_two_files_read_back_and_keep_names(tmp_path):
    names = ["a", "skin 3", "it's", "none", "z.9_-"]
    parent, bl = tree_case("tree15")
    first = numpy_first(parent)
    mass = random_cells(np.random.default_rng(8), 5, len(parent), bits=42)
    mass[3] = 0
    used = mass.sum(axis=1, dtype=U64) > 0
    kmeans = cohort_mod.kmeans_host(mass, first, bl, 3)
    text = cohort_mod.format_kmeans_tsv(names, kmeans)
    lines = text.split("\n")
    assert lines[0] == f"# epik_amd kmeans v1  samples=5 used=4 clusters=3 iterations={int(kmeans.info['iterations'])} converged=1"
    assert lines[1] == "# unused\tnone"
    c0 = kmeans.clusters[0]
    assert lines[2] == "# cluster\t0\t%d\t%s\t%.17g\t%.17g" % (c0["size"], names[c0["seed"]], c0["sum_dist"], c0["sum_sq"])
    assert lines[5] == "name\tcluster\tdist" and [ln.split("\t")[0] for ln in lines[6:10]] == ["a", "skin 3", "it's", "z.9_-"]
    assert len(lines) == 11 and lines[-1] == ""
    path = tmp_path / "cohort_kmeans_x.tsv"
    path.write_bytes(text.encode())
    back_names, cluster, dist, info = cohort_mod.read_kmeans_tsv(str(path))
    assert back_names == ["a", "skin 3", "it's", "z.9_-"] and info["unused"] == ["none"]
    assert list(cluster) == list(kmeans.samples["cluster"][used]) and same_bits(dist, kmeans.samples["dist"][used])
    assert (info["samples"], info["used"], info["clusters"], info["iterations"], info["converged"]) == (5, 4, 3, int(kmeans.info["iterations"]), 1)
    assert list(info["size"]) == list(kmeans.clusters["size"]) and info["seed"] == [names[s] for s in kmeans.clusters["seed"]]
    assert same_bits(info["sum_dist"], kmeans.clusters["sum_dist"]) and same_bits(info["sum_sq"], kmeans.clusters["sum_sq"])
    cent_text = cohort_mod.format_kmeans_centroids_tsv(kmeans)
    assert cent_text.split("\n")[0] == "cluster\tedge_num\tmass" and cent_text.count("\n") == 1 + int((kmeans.centroids != 0).sum())
    cent_path = tmp_path / "cohort_kmeans_centroids_x.tsv"
    cent_path.write_bytes(cent_text.encode())
    assert same_bits(cohort_mod.read_kmeans_centroids_tsv(str(cent_path), 3, len(first)), kmeans.centroids)
    path.write_text("# something else\n")
    with pytest.raises(ValueError):
        cohort_mod.read_kmeans_tsv(str(path))
    cent_path.write_text("name\tpc1\n")
    with pytest.raises(ValueError):
        cohort_mod.read_kmeans_centroids_tsv(str(cent_path), 3, len(first))
    with pytest.raises(ValueError):
        cohort_mod.format_kmeans_tsv(names[:4], kmeans)
    # nothing used: the first line, the unused samples, the column names alone
    empty = cohort_mod.kmeans_host(np.zeros((2, len(first)), U64), first, bl, 5)
    assert cohort_mod.format_kmeans_tsv(["x y", "q"], empty) == (
        "# epik_amd kmeans v1  samples=2 used=0 clusters=0 iterations=0 converged=1\n# unused\tx y\n# unused\tq\nname\tcluster\tdist\n")
    assert cohort_mod.format_kmeans_centroids_tsv(empty) == "cluster\tedge_num\tmass\n"


# ---- the host code stand-alone -----------------------------------------------------------------------------------------
def _kmeans_input(path, mass, first, bl):
    with open(path, "wb") as fh:
        fh.write(np.array(mass.shape, dtype="<u8").tobytes() + np.ascontiguousarray(mass, U64).tobytes() +
                 np.ascontiguousarray(first, np.uint32).tobytes() + np.ascontiguousarray(bl, np.float64).tobytes())


@pytest.mark.parametrize("sanitized", [False, True])
def test_host_test_binary_kmeans_is_the_library_s(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    parent, bl = tree_case("tree15")
    first = numpy_first(parent)
    for num_samples, k, iterations in ((1, 5, 100), (3, 5, 100), (7, 3, 100), (7, 64, 1)):
        mass = random_cells(np.random.default_rng(9), num_samples, len(parent), empty=1, bits=42)
        _kmeans_input(tmp_path / "in.bin", mass, first, bl)
        run = subprocess.run([binary, "kmeans", str(tmp_path / "out.bin"), str(tmp_path / "in.bin"), str(k), str(iterations)],
                             capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (num_samples, run.stderr)
        got = cohort_mod.kmeans_host(mass, first, bl, k, iterations)
        want = got.samples.tobytes() + got.clusters.tobytes() + got.centroids.tobytes() + np.asarray(got.info).tobytes()
        assert (tmp_path / "out.bin").read_bytes() == want, num_samples
    for bad in ("0", "65"):
        run = subprocess.run([binary, "kmeans", str(tmp_path / "o.bin"), str(tmp_path / "in.bin"), bad, "100"], capture_output=True, text=True)
        assert run.returncode == 1 and "num_clusters" in run.stderr
    run = subprocess.run([binary, "kmeans", str(tmp_path / "o.bin"), str(tmp_path / "in.bin"), "3", "1001"], capture_output=True, text=True)
    assert run.returncode == 1 and "max_iterations" in run.stderr
