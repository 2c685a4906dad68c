"""The cohort analyses at the branch counts where the kernels that walk the branches have their seams, on three tree shapes.

Every other test of a cohort analysis takes its tree from test_cohort_gpu.kr_case: three random binary trees of N = 7, 999
and 5 199 branches and the ladder of 10 399.  N mod 32 is 7, 7, 15 and 31 there and N mod 256 is 7, 231, 79 and 159: never
0, never 1; N is never 1 or 2 and never even, and no node has more than two children.  `cohort_edge_tree` builds a tree of any
N in three shapes, and EDGES lists the N that step over a constant of a kernel:

  32, 64, 96      cohort_place.hip / unifrac_place.hip kChunk = 32, epca_place.hip / kmeans_place.hip / squash_place.hip
                  kUnit = 32: one, two and three full units and an EMPTY tail (`kc = N - b0 < 32 ? ... : 32` never takes its
                  first arm, `N % 32 == 0` in the row kernels); 96 is also squash's odd unit count with no tail, whose last
                  unit has no partner in the double buffer (`second = b0 + kUnit < full`)
  31, 33, 63, 65  a unit short of a branch and over by one; 1, 2, 3: a tail alone
  256, 512        cohort_normalise_kernel's scan block kBlock = 256 and EPIK_AMD_DIVERSITY_BLOCK = 256: one and two blocks
                  that are exactly full; 255, 257: short of a branch and over by one
  3072 | 3073     cohort_place.hip kLdsBudget = 48 KiB = 16 * 3072: the last tree whose cells share a CU's LDS with other
                  workgroups' and the first that takes a CU for one workgroup (the handle is made through a placer of that N)

  "random"        a multifurcating post-order tree built on a stack: unary nodes, nodes of up to four children, a root that
                  adopts what is left; any N >= 1, even N included
  "star"          test_assign_cpu.star: first[N - 1] = 0, first[b] = b everywhere else, a root of N - 1 children; N >= 2
  "ladder"        test_assign_cpu.caterpillar: the deepest tree; odd N

Here, without a GPU: first_of against the parent walk, kr_host and unifrac_host against the numpy restatements bit for bit,
and every other mirror run once, with the conditions asserted that keep the GPU sweep of test_cohort_edges_gpu.py (which
holds the device to these mirrors bit for bit) from passing vacuously.  `edge_case` computes the mirrors once per tree and
shares them with that file.
"""
import numpy as np
import pytest

from epik_amd import cohort as cohort_mod
from test_assign_cpu import caterpillar, star
from test_cohort_cpu import numpy_first, numpy_kr, random_cells, same_bits
from test_cohort_lifecycle_gpu import DEPTH_STEP, defined_families, mirrors
from test_correlation_cpu import metadata
from test_diversity_cpu import draw_best
from test_edgetest_gpu import group_labels
from test_unifrac_cpu import METRICS, numpy_unifrac

U64 = np.uint64
EDGES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 255, 256, 257, 512, 3072, 3073)
LADDERS = (31, 33, 63, 65, 255, 257, 3073)
SHAPES = ("random", "star", "ladder")
SAMPLES = 34                 # one is empty: 33 used cross the tile of 32 and k-means' tiles of 16; 30 padding samples
EMPTY = 1
SWEEP = [(n, shape) for n in EDGES for shape in SHAPES
         if shape == "random" or (shape == "star" and n >= 2) or (shape == "ladder" and n in LADDERS)]
SWEEP_IDS = [f"{n}-{shape}" for n, shape in SWEEP]
ANALYSES = ("kr",) + tuple(METRICS) + ("squash", "epca", "kmeans", "kmeans33", "alpha", "rarefy", "correlation", "dispersion", "edgetest")


def cohort_edge_tree(num_branches, shape):
    """(parent, branch_length) of a post-order tree of that many branches, the root last, every fifth length 0.0."""
    n = int(num_branches)
    if shape == "star":
        assert n >= 2
        parent, bl = star(n - 1)
    elif shape == "ladder":
        parent, bl = caterpillar(n)
    else:
        assert shape == "random" and n >= 1
        rng = np.random.default_rng(7000 + n)
        parent, open_subtrees = np.full(n, -1, dtype=np.int64), []
        for b in range(n):
            # b adopts the last 1 .. 4 open subtrees (they end at b - 1, so first[b] .. b stays one range) or is a leaf
            take = len(open_subtrees) if b == n - 1 else 0
            if b < n - 1 and open_subtrees and rng.random() < 0.45:
                take = min(len(open_subtrees), int(rng.integers(1, 5)))
            for child in open_subtrees[len(open_subtrees) - take:]:
                parent[child] = b
            del open_subtrees[len(open_subtrees) - take:]
            open_subtrees.append(b)
        bl = rng.uniform(0.01, 0.3, size=n)
    bl = np.array(bl, dtype=np.float64)
    bl[::5] = 0.0
    parent = np.asarray(parent, dtype=np.int64)
    assert len(parent) == n and parent[n - 1] == -1 and (parent[:n - 1] > np.arange(n - 1)).all()
    return parent, bl


def edge_cells(num_branches, shape):
    """(mass, best, params) of the sweep at that tree: S = 34, sample 1 empty and every other one with mass."""
    n, s = num_branches, SAMPLES
    rng = np.random.default_rng(8000 + 3 * n + SHAPES.index(shape))
    mass = random_cells(rng, s, n, empty=EMPTY, bits=42)
    if n <= 3:
        # (of one, two or three cells random_cells zeroes all in some samples, and all but one in several, which are then the
        # same sample in shares, at KR distance 0: on these trees every cell of a used sample holds mass)
        fill = rng.integers(1, 1 << 42, size=mass.shape, dtype=np.uint64)
        mass = np.where(mass == 0, fill, mass)
        mass[EMPTY] = 0
    best = draw_best(rng, s, n, DEPTH_STEP, 40)
    labels = np.stack([group_labels(rng, s, 3)[:, 0], group_labels(rng, s, 32)[:, 0]], axis=1)
    params = {"clusters": 5, "components": 5, "depths": 40, "meta": np.ascontiguousarray(metadata(rng, mass)),
              "labels": np.ascontiguousarray(labels, dtype=np.uint32), "edgetest_p": 9,
              "edgetest_seed": int(rng.integers(0, 1 << 63)) * 2 + 1}
    return mass, best, params


EDGE_CASES = {}


def edge_case(num_branches, shape):
    """(parent, bl, first, mass, best, params, want): the tree, the cells and name -> the host mirror's answer for ANALYSES,
    computed once; and the conditions that keep a comparison with them from passing vacuously, asserted on the mirrors alone."""
    key = (num_branches, shape)
    if key in EDGE_CASES:
        return EDGE_CASES[key]
    n, s = num_branches, SAMPLES
    parent, bl = cohort_edge_tree(n, shape)
    first = numpy_first(parent)
    mass, best, params = edge_cells(n, shape)
    want = mirrors(mass, best, first, bl, params, only=tuple(a for a in ANALYSES if a != "kmeans33"))
    want["kmeans33"] = mirrors(mass, best, first, bl, {**params, "clusters": 33}, only=("kmeans",))["kmeans"]
    what = (n, shape)
    used = mass.any(axis=1)
    assert int(used.sum()) == s - 1 == 33 and not used[EMPTY], what
    assert int(want["epca"].info["converged"]) == 1 and int(want["epca"].info["used"]) == 33, (what, want["epca"].info)
    assert want["squash"][1] == 32, (what, want["squash"][1])
    assert int(want["kmeans"].info["used"]) == 33 and int(want["kmeans33"].info["used"]) == 33, what
    inner = want["kr"][np.ix_(used, used)][~np.eye(33, dtype=bool)]
    assert (want["kr"][EMPTY] == np.where(np.arange(s) == EMPTY, 0.0, -1.0)).all(), what
    labels = params["labels"]
    assert len(set(labels[used, 0].tolist())) == 3 and len(set(labels[used, 1].tolist())) == 32, what
    families = want["edgetest"].records["family"]["p"].size
    assert families == 2 * n * 4, (what, families)
    if n == 1:
        # one branch holds every sample's whole mass: C = 1 and B = 0 in every sample, nothing differs and nothing is tested
        assert (inner == 0.0).all() and defined_families(want["edgetest"]) == 0, what
    else:
        assert (inner > 0.0).all(), (what, float(inner.min()))
        assert 3 * defined_families(want["edgetest"]) > families, (what, defined_families(want["edgetest"]), families)
    EDGE_CASES[key] = (parent, bl, first, mass, best, params, want)
    return EDGE_CASES[key]


def test_the_sweep_is_the_issue_s():
    assert len(SWEEP) == 16 + 15 + 7 and (1, "star") not in SWEEP and all(n % 2 for n in LADDERS)
    assert {n % 32 for n in EDGES} >= {0, 1, 31} and {n % 256 for n in EDGES} >= {0, 1, 255}


def test_the_shapes_are_what_they_are_called():
    parent, _ = cohort_edge_tree(512, "random")
    children = np.bincount(parent[:-1], minlength=512)
    assert children.max() >= 4 and (children == 1).any() and (children == 3).any()        # multifurcations and unary nodes
    first = numpy_first(parent)
    assert first[511] == 0 and ((first[parent[:-1]] <= first[:-1]) & (parent[:-1] > np.arange(511))).all()
    parent, _ = cohort_edge_tree(3072, "star")
    first = numpy_first(parent)
    assert first[3071] == 0 and np.array_equal(first[:3071], np.arange(3071)) and (parent[:3071] == 3071).all()
    parent, _ = cohort_edge_tree(257, "ladder")
    assert np.array_equal(numpy_first(parent)[2::2], np.zeros(128))                       # every inner node's clade starts at 0
    for n in (1, 2):
        parent, bl = cohort_edge_tree(n, "random")
        assert parent.tolist() == [0, -1][2 - n:] or parent.tolist() == [1, -1][2 - n:]
        assert bl[0] == 0.0


@pytest.mark.parametrize("num_branches, shape", SWEEP, ids=SWEEP_IDS)
def test_the_mirrors_at_the_branch_count_edges(num_branches, shape):
    parent, bl, first, mass, best, params, want = edge_case(num_branches, shape)
    assert np.array_equal(first, cohort_mod.first_of(parent))
    restated = numpy_kr(mass, first, bl)
    assert same_bits(want["kr"], restated), np.argwhere(want["kr"].view(U64) != restated.view(U64))[:10]
    for name in METRICS:
        restated = numpy_unifrac(mass, first, bl, name)
        assert same_bits(want[name], restated), (name, np.argwhere(want[name].view(U64) != restated.view(U64))[:10])
        used = mass.any(axis=1)
        inner = want[name][np.ix_(used, used)]
        assert (inner >= 0.0).all() and (inner <= 1.0).all(), name
    # the other mirrors ran in edge_case, which asserted what the GPU sweep relies on; their shapes
    assert want["alpha"].shape == (SAMPLES,) and want["rarefy"].shape == (SAMPLES, 40, 2)
    assert want["correlation"][0].shape == (3, num_branches) and want["dispersion"].shape == (num_branches,)
    assert want["edgetest"].records.shape == (2, num_branches) and want["kmeans33"].clusters.shape == (33,)
