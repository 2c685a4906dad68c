"""Alpha diversity and rarefaction curves of a cohort's samples, no device: the rule of include/epik_amd.h restated here in
numpy against epik_amd_cohort_alpha_host and epik_amd_cohort_rarefy_host, bit for bit; the curve against the enumeration of
every subset and against exact binomial fractions, within a derived bound; a case worked out by hand; properties; forged
cells; the C ABI's refusals; the drivers' and the launcher's flags; the two files; and the stand-alone host binary (plain
and under ASan + UBSan).
"""
import itertools
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod
from test_capi_cpu import _header_symbols
from test_cohort_cpu import host_bins, numpy_first, random_cells, same_bits, tree_case  # noqa: F401 (host_bins: a fixture)
from test_squash_cpu import BALANCED, numpy_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
BLOCK = 256
FIELDS = ("pd", "rooted_pd", "bwpd_half", "bwpd_one", "quadratic")
DEPTHS = ((1, 1), (1, 256), (7, 40), (64, 64))      # (depth_step, num_depths)


# ---- the rule, restated ----------------------------------------------------------------------------------------------
def blocked_sum(terms):
    """BS(t) along the last axis: the terms of a block added one after the other from +0.0 (np.add.accumulate adds in
    ascending order; the leading +0.0 is the rule's first acc), then the blocks the same way."""
    terms = np.asarray(terms, dtype=np.float64)
    zero = np.zeros(terms.shape[:-1] + (1,))
    partials = [np.add.accumulate(np.concatenate([zero, terms[..., g:g + BLOCK]], axis=-1), axis=-1)[..., -1]
                for g in range(0, terms.shape[-1], BLOCK)]
    return np.add.accumulate(np.concatenate([zero, np.stack(partials, axis=-1)], axis=-1), axis=-1)[..., -1]


def integer_sides(cells, first):
    """(total [S], clade [S][N], below [S][N]) in wrapping uint64."""
    cells = np.asarray(cells, dtype=U64)
    s, n = cells.shape
    prefix = np.zeros((s, n + 1), dtype=U64)
    np.cumsum(cells, axis=1, dtype=U64, out=prefix[:, 1:])
    clade = prefix[:, 1:] - prefix[:, np.asarray(first, dtype=np.int64)]
    return prefix[:, n], clade, clade - cells


def numpy_alpha(mass, first, branch_length):
    """capi.ALPHA [S] by the header's text."""
    mass = np.asarray(mass, dtype=U64)
    half = 0.5 * np.asarray(branch_length, dtype=np.float64)
    c, b, total = numpy_planes(mass, first)
    _, clade, below = integer_sides(mass, first)
    t = total[:, None]
    one = lambda flag: np.where(flag, 1.0, 0.0)

    def balance(d):
        w = np.minimum(d, 1.0 - d)
        return np.where(w > 0.0, w, 0.0)

    with np.errstate(invalid="ignore"):
        wb, wc = balance(b), balance(c)
        terms = {"pd": half * (one((below > 0) & (below < t)) + one((clade > 0) & (clade < t))),
                 "rooted_pd": half * (one(below > 0) + one(clade > 0)),
                 "bwpd_half": half * (np.sqrt(2.0 * wb) + np.sqrt(2.0 * wc)),
                 "bwpd_one": half * (2.0 * wb + 2.0 * wc),
                 "quadratic": half * (b * (1.0 - b) + c * (1.0 - c))}
    out = np.zeros(len(mass), dtype=capi.ALPHA)
    for f in FIELDS:
        with np.errstate(invalid="ignore"):
            out[f] = np.where(total == 0, -1.0, blocked_sum(terms[f]))
    return out


def chances(n, sides, depth_step, depths):
    """Q(m, k_j) of the rule for every m of `sides` (uint64) and j < depths: float64 [len(sides)][depths].  Q depends on m
    alone, so every distinct m is walked once."""
    values, inverse = np.unique(np.asarray(sides, dtype=U64), return_inverse=True)
    q = np.ones(len(values))
    out = np.zeros((len(values), depths))
    for k in range(depths * depth_step):
        left = n - k                                               # n - k >= 1
        r = np.float64(1.0) / np.float64(left)
        live = values < U64(left)
        factor = np.where(live, U64(left) - values, U64(0)).astype(np.float64)    # (double)(n - m - k)
        q = np.where(values == 0, 1.0, np.where(live, (q * factor) * r, 0.0))
        if (k + 1) % depth_step == 0:
            out[:, (k + 1) // depth_step - 1] = q
    return out[inverse]


def numpy_rarefy(best, first, branch_length, depth_step, num_depths):
    """float64 [S][J][2] by the header's text."""
    best = np.asarray(best, dtype=U64)
    s, n_branches = best.shape
    half = 0.5 * np.asarray(branch_length, dtype=np.float64)
    reads, cc, cb = integer_sides(best, first)
    curve = np.full((s, num_depths, 2), -1.0)
    for i in range(s):
        n = int(reads[i])
        if not 0 < n < 1 << 53:
            continue
        depths = min(num_depths, n // depth_step)
        if depths == 0:
            continue
        sides = np.concatenate([cb[i], cc[i], U64(n) - cb[i], U64(n) - cc[i]])
        q = chances(n, sides, depth_step, depths)
        miss_b, miss_c, all_b, all_c = (q[x * n_branches:(x + 1) * n_branches] for x in range(4))
        ru_b, ru_c = 1.0 - miss_b, 1.0 - miss_c
        uu_b, uu_c = (1.0 - miss_b) - all_b, (1.0 - miss_c) - all_c
        uu_b, uu_c = np.where(uu_b > 0.0, uu_b, 0.0), np.where(uu_c > 0.0, uu_c, 0.0)
        curve[i, :depths, 0] = blocked_sum((half[:, None] * (uu_b + uu_c)).T)
        curve[i, :depths, 1] = blocked_sum((half[:, None] * (ru_b + ru_c)).T)
    return curve


def same_records(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def draw_best(rng, num_samples, num_branches, depth_step, num_depths):
    """best[S][N] whose read counts n_s are, sample by sample: above the deepest depth (a whole curve), exactly a k_j, 1, 0,
    a third of the deepest depth (a curve that ends early), then small counts (most curves end early), every eighth whole."""
    deepest = depth_step * num_depths
    counts = [deepest + 37, depth_step * max(1, num_depths // 2), 1, 0, deepest // 3 + 1]
    while len(counts) < num_samples:
        counts.append(deepest + 5 if len(counts) % 32 == 8 else int(rng.integers(2, min(deepest, 200) + 2)))
    best = np.zeros((num_samples, num_branches), dtype=U64)
    for s in range(num_samples):
        shares = rng.dirichlet(np.full(num_branches, 0.3)) if num_branches > 1 else np.ones(1)
        best[s] = rng.multinomial(counts[s], shares).astype(U64)
    return best


CELLS = {}


def cells_case(tree_name, num_samples, depth_step=7, num_depths=40):
    """(mass, best, first, branch_length) of a case of the restatement tests."""
    key = (tree_name, num_samples, depth_step, num_depths)
    if key not in CELLS:
        parent, bl = tree_case(tree_name)
        rng = np.random.default_rng(6000 + num_samples + depth_step)
        CELLS[key] = (random_cells(rng, num_samples, len(parent), empty=1, bits=42),
                      draw_best(rng, num_samples, len(parent), depth_step, num_depths), numpy_first(parent), bl)
    return CELLS[key]


@pytest.mark.parametrize("tree_name", ["one", "tree15", "tree2999"])
@pytest.mark.parametrize("num_samples", [1, 2, 3, 33, 70])
def test_alpha_host_equals_the_numpy_restatement_bit_for_bit(tree_name, num_samples):
    mass, _, first, bl = cells_case(tree_name, num_samples)
    got, want = cohort_mod.alpha_host(mass, first, bl), numpy_alpha(mass, first, bl)
    assert got.dtype == capi.ALPHA and same_records(got, want), (got, want)
    empty = mass.sum(axis=1, dtype=U64) == 0
    assert all((got[f][empty] == -1.0).all() and (got[f][~empty] >= 0.0).all() for f in FIELDS)
    if num_samples > 1:
        assert empty[1] and (len(first) == 1 or (got["pd"][~empty] > 0).all())


@pytest.mark.parametrize("tree_name", ["one", "tree15", "tree2999"])
@pytest.mark.parametrize("num_samples", [1, 2, 3, 33, 70])
@pytest.mark.parametrize("depth_step,num_depths", DEPTHS)
def test_rarefy_host_equals_the_numpy_restatement_bit_for_bit(tree_name, num_samples, depth_step, num_depths):
    _, best, first, bl = cells_case(tree_name, num_samples, depth_step, num_depths)
    got, want = cohort_mod.rarefy_host(best, first, bl, depth_step, num_depths), numpy_rarefy(best, first, bl, depth_step, num_depths)
    assert got.shape == (num_samples, num_depths, 2) and same_bits(got, want), np.argwhere(got.view(U64) != want.view(U64))[:10]
    reads = best.sum(axis=1, dtype=U64).astype(np.int64)
    written = np.minimum(reads // depth_step, num_depths)
    for s in range(num_samples):
        assert (got[s, :written[s]] >= 0.0).all() and (got[s, written[s]:] == -1.0).all(), s
    assert written[0] == num_depths                                    # a whole curve
    if num_samples >= 33:                                              # one ends exactly at a k_j, one is 1 read, one none, many end early
        assert reads[1] == depth_step * written[1] and reads[2] == 1 and reads[3] == 0 and not (got[3] != -1.0).any()
        assert (written[4:] < num_depths).sum() >= 10 or num_depths == 1


# ---- independent of the rule: every subset, and exact binomials ----------------------------------------------------------
def exact_curve(best_row, first, branch_length, depths, chance=None):
    """The expected unrooted and rooted PD of k reads of one sample in exact fractions, for every k of `depths`.  Without
    `chance`: by enumerating all C(n, k) subsets of the reads.  With it: chance(m, k) = C(n - m, k) / C(n, k)."""
    n_branches = len(first)
    half = [Fraction(float(x)) / 2 for x in branch_length]
    reads = [b for b in range(n_branches) for _ in range(int(best_row[b]))]      # every read: its branch
    n = len(reads)
    in_clade = lambda read, b: int(first[b]) <= read <= b
    out = {}
    for k in depths:
        unrooted = rooted = Fraction(0)
        if chance is None:
            count = 0
            for subset in itertools.combinations(reads, k):
                count += 1
                for b in range(n_branches):
                    for far in (sum(in_clade(r, b) and r != b for r in subset), sum(in_clade(r, b) for r in subset)):
                        rooted += half[b] * (far > 0)
                        unrooted += half[b] * (0 < far < k)
            assert count == math.comb(n, k)
            out[k] = (unrooted / count, rooted / count)
        else:
            for b in range(n_branches):
                clade = sum(int(best_row[x]) for x in range(int(first[b]), b + 1))
                for far in (clade - int(best_row[b]), clade):
                    rooted += half[b] * (1 - chance(far, k))
                    unrooted += half[b] * (1 - chance(far, k) - chance(n - far, k))
            out[k] = (unrooted, rooted)
    return out


def curve_bound(k, n_branches, branch_length):
    return Fraction(8 * k + 2 * n_branches + 8, 2 ** 53) * sum(Fraction(float(x)) for x in branch_length)


def test_the_curve_is_the_average_over_every_subset_of_the_reads():
    """The bound, with u = 2^-53.  Q(m, k) is a product of k factors (n - m - i) / (n - i): the conversions are exact, and a
    step rounds three times (the reciprocal, the two products), so the computed Q is the exact one times at most (1 + u)^3k,
    and Q <= 1: an error of 3ku (and (3ku)^2 / 2 beyond, below ku * 2^-30 for k <= 2^20).  ru = 1 - miss rounds once, values
    in [0, 1]: 3ku + u.  uu = ru - all: (3ku + u) + 3ku + u = (6k + 2)u; replacing a negative uu by 0 moves it towards the
    exact value, which is >= 0.  The two halves of a branch are added, a sum <= 2 that rounds once: 2 (6k + 2)u + 2u; times
    half[b] = bl[b] / 2 (exact), a product <= bl[b] that rounds once: bl[b] ((6k + 2)u + u + u) = bl[b] (6k + 4)u.  Summed
    over the branches: (6k + 4)u * sum(bl).  The blocked sum makes fewer than N + N / 256 + 1 <= 2N additions of
    non-negative terms, each rounding a partial sum that is at most the total <= sum(bl) (1 + 2^-20): 2Nu * sum(bl).  In
    all (6k + 2N + 4)u * sum(bl); the issue's (8k + 2N + 8)u * sum(bl) leaves (2k + 4)u for the second-order terms."""
    rng = np.random.default_rng(11)
    for parent, bl in ((BALANCED, np.array([0.5, 0.25, 1.0, 0.75, 0.125, 2.0, 0.0625])), tree_case("tree15")):
        first = numpy_first(parent)
        n_branches = len(parent)
        for n in (1, 2, 5, 8):
            best = np.zeros((1, n_branches), U64)
            for b in rng.integers(0, n_branches, size=n):
                best[0, b] += U64(1)
            got = cohort_mod.rarefy_host(best, first, bl, 1, n)
            assert same_bits(got, numpy_rarefy(best, first, bl, 1, n))
            want = exact_curve(best[0], first, bl, range(1, n + 1))
            for k in range(1, n + 1):
                for idx in (0, 1):
                    assert abs(Fraction(float(got[0, k - 1, idx])) - want[k][idx]) <= curve_bound(k, n_branches, bl), (n, k, idx)
            assert want[1][0] == 0 and want[n][1] >= want[n][0]


def test_the_curve_agrees_with_exact_binomial_fractions_at_depth():
    parent, bl = tree_case("tree15")
    first = numpy_first(parent)
    rng = np.random.default_rng(12)
    for n in (4096, 100_000):
        best = rng.multinomial(n, rng.dirichlet(np.full(len(parent), 0.5))).astype(U64)[None, :]
        best[0, 3] += best[0, 7]
        best[0, 7] = 0                                                             # an empty leaf among them
        got = cohort_mod.rarefy_host(best, first, bl, 1024, 4)
        denominators = {k: math.comb(n, k) for k in (1024, 2048, 3072, 4096)}
        chance = lambda m, k: Fraction(math.comb(n - m, k), denominators[k])
        want = exact_curve(best[0], first, bl, denominators, chance)
        for j, k in enumerate(denominators):
            for idx in (0, 1):
                assert abs(Fraction(float(got[0, j, idx])) - want[k][idx]) <= curve_bound(k, len(parent), bl), (n, k, idx)


# ---- a case by hand --------------------------------------------------------------------------------------------------
def test_one_sample_on_the_balanced_tree_by_hand():
    # ((0,1)2,(3,4)5)6, every length 1, so half = 0.5.  3 reads on leaf 0 and 1 on leaf 3: T = n = 4.  (below, clade) per
    # branch: b0 (0, 3), b1 (0, 0), b2 (3, 3), b3 (0, 1), b4 (0, 0), b5 (1, 1), b6 (4, 4): six half branches with mass on
    # both sides (x = 3 three times, x = 1 three times) and the two of the root branch with all of it below.
    # pd: 0.5 * (1 + 0 + 2 + 1 + 0 + 2 + 0) = 3, the path between the two placements: half of b0, b2, b5, half of b3.
    # rooted_pd: the root branch too, 0.5 * 2 more = 4.
    # D = x / 4 is 0.75 or 0.25 on the six: w = 0.25, 2w = 0.5, so bwpd_one = 0.5 * 6 * 0.5 = 1.5,
    # bwpd_half = 0.5 * 6 * sqrt(0.5) = 2.1213..., quadratic = 0.5 * 6 * (0.75 * 0.25) = 0.5625.
    # The curve: Q(m, k) = C(4 - m, k) / C(4, k).  k = 1: a single read spans nothing, 0; rooted 0.5 + 1 + 1 = 2.5 from either
    # leaf.  k = 2: three of the six pairs hold the read of leaf 3: 3 * 3 / 6 = 1.5; rooted: 0.5 * (3 * 1 + 3 * 0.5 + 2) = 3.25.
    # k = 3: three of the four triples hold it: 2.25; rooted 0.5 * (3 + 3 * 0.75 + 2) = 3.625.  k = 4: all reads, pd and rooted_pd.
    first = numpy_first(BALANCED)
    bl = np.ones(7)
    cells = np.zeros((1, 7), U64)
    cells[0, 0], cells[0, 3] = 3, 1
    alpha = cohort_mod.alpha_host(cells, first, bl)
    assert same_records(alpha, numpy_alpha(cells, first, bl))
    root = math.sqrt(0.5)
    half_terms = [0.5 * root, 0.0, 0.5 * (root + root), 0.5 * root, 0.0, 0.5 * (root + root), 0.0]
    bwpd_half = 0.0
    for t in half_terms:
        bwpd_half = bwpd_half + t
    assert tuple(alpha[0].tolist()) == (3.0, 4.0, bwpd_half, 1.5, 0.5625) and abs(bwpd_half - 3 * root) < 1e-15
    curve = cohort_mod.rarefy_host(cells, first, bl, 1, 5)
    assert same_bits(curve, numpy_rarefy(cells, first, bl, 1, 5))
    hand = [(0.0, 2.5), (1.5, 3.25), (2.25, 3.625), (3.0, 4.0)]
    # every Q here is a dyadic fraction or a third; (8k + 2N + 8) * 2^-53 * sum(bl) is the test's bound above
    assert np.abs(curve[0, :4] - np.array(hand)).max() <= (8 * 4 + 2 * 7 + 8) * 2.0 ** -53 * 7
    assert same_bits(curve[0, 0], hand[0]) and same_bits(curve[0, 3], hand[3]) and same_bits(curve[0, 4], (-1.0, -1.0))


# ---- properties ----------------------------------------------------------------------------------------------------------
def test_properties():
    for tree_name, num_samples in (("tree15", 33), ("tree2999", 3)):
        parent, bl = tree_case(tree_name)
        first = numpy_first(parent)
        n_branches = len(parent)
        rng = np.random.default_rng(70 + num_samples)
        # with mass := best the curve at k = n_s is alpha's pd and rooted_pd: every Q of an inner side is exactly 0 there
        # and of an empty side exactly 1
        counts = rng.integers(1, 120, size=num_samples)
        best = np.stack([rng.multinomial(c, rng.dirichlet(np.full(n_branches, 0.2))) for c in counts]).astype(U64)
        best[1] = 0
        best[1, n_branches // 2] = 9                                              # all reads on one branch
        counts[1] = 9
        alpha = cohort_mod.alpha_host(best, first, bl)
        curve = cohort_mod.rarefy_host(best, first, bl, 1, 128)
        for s in range(num_samples):
            assert same_bits(curve[s, counts[s] - 1], (alpha["pd"][s], alpha["rooted_pd"][s])), s
            assert (curve[s, counts[s]:] == -1.0).all()
            assert (np.diff(curve[s, :counts[s], 1]) >= -1e-12).all()              # more reads, no less expected diversity
        assert not curve[1, :9, 0].view(U64).any() and alpha["pd"][1] == 0.0       # exactly +0.0 at every depth
        assert (curve[1, :9, 1] == curve[1, 0, 1]).all() and curve[1, 0, 1] > 0
        mass = random_cells(rng, num_samples, n_branches, empty=1, bits=42)
        a = cohort_mod.alpha_host(mass, first, bl)
        used = a["pd"] != -1.0
        assert (a["bwpd_one"][used] <= a["bwpd_half"][used]).all() and (a["bwpd_half"][used] <= a["pd"][used]).all()
        assert (a["pd"][used] <= a["rooted_pd"][used]).all() and (a["quadratic"][used] <= a["bwpd_one"][used]).all()
        assert same_records(cohort_mod.alpha_host(mass * U64(2), first, bl), a)    # D = x / T: the same bits


# ---- forged cells ------------------------------------------------------------------------------------------------------
def forged_diversity_cohorts():
    """name -> (mass, best, parent, branch_length)"""
    parent, bl = tree_case("tree15")
    n = len(parent)
    rng = np.random.default_rng(45)
    x = random_cells(rng, 3, n, bits=42)
    few = draw_best(rng, 3, n, 7, 40)
    top = U64(1) << U64(63)
    wrapped = x.copy()
    wrapped[0, 2], wrapped[0, 9] = top, top + U64(5)                               # T_0 wraps to a small number
    wrapped[1, :] = U64(0xFFFFFFFFFFFFFFFF)
    wrapped_best = few.copy()
    wrapped_best[0, 2], wrapped_best[0, 9] = top, top                              # n_0 wraps back to the few reads
    wrapped_best[1, 4] = U64(0xFFFFFFFFFFFFFFFD)                                          # n_1 wraps below the reads of a clade
    huge = few.copy()
    huge[0, 5] = U64(1) << U64(53)                                                 # n_0 >= 2^53: not rarefiable
    huge[1, 5] = (U64(1) << U64(53)) - U64(1) - huge[1].sum(dtype=U64) + huge[1, 5]   # n_1 = 2^53 - 1: rarefiable
    one_parent, one_bl = tree_case("one")
    return {
        "sums that wrap": (wrapped, wrapped_best, parent, bl),
        "reads at and above 2^53": (x, huge, parent, bl),
        "an empty sample": (np.stack([x[0], np.zeros(n, U64), x[2]]), np.stack([few[0], np.zeros(n, U64), few[2]]), parent, bl),
        "all empty": (np.zeros((2, n), U64), np.zeros((2, n), U64), parent, bl),
        "zero-length branches": (x, few, parent, np.zeros(n)),
        "a single branch": (random_cells(rng, 4, 1, bits=42) + U64(1), np.array([[300], [1], [0], [7]], U64), one_parent, np.array([0.25])),
    }


@pytest.mark.parametrize("name", sorted(forged_diversity_cohorts()))
def test_forged_cells(name):
    mass, best, parent, bl = forged_diversity_cohorts()[name]
    first = numpy_first(parent)
    alpha = cohort_mod.alpha_host(mass, first, bl)
    assert same_records(alpha, numpy_alpha(mass, first, bl)), name
    curves = {}
    for step, depths in DEPTHS:
        curves[step, depths] = cohort_mod.rarefy_host(best, first, bl, step, depths)
        assert same_bits(curves[step, depths], numpy_rarefy(best, first, bl, step, depths)), (name, step, depths)
    curve = curves[7, 40]
    if name == "reads at and above 2^53":
        assert (curve[0] == -1.0).all() and (curve[1] >= 0.0).all() and int(best[1].sum(dtype=U64)) == (1 << 53) - 1
    elif name == "an empty sample":
        assert (curve[1] == -1.0).all() and all(alpha[f][1] == -1.0 for f in FIELDS) and (curve[0] >= 0).all()
    elif name == "all empty":
        assert (curve == -1.0).all() and all((alpha[f] == -1.0).all() for f in FIELDS)
    elif name == "zero-length branches":
        assert not curve[0].view(U64).any() and all(not alpha[f].view(U64).any() for f in FIELDS)
    elif name == "a single branch":      # the one branch holds everything below its middle and nothing beside it
        rooted = 0.5 * bl[0]
        assert same_bits(alpha["pd"], np.zeros(4)) and same_bits(alpha["rooted_pd"], np.full(4, rooted))
        assert same_bits(curve[0, :, 0], np.zeros(40)) and same_bits(curve[0, :, 1], np.full(40, rooted))
        assert same_bits(curve[3, 0], (0.0, rooted)) and (curve[3, 1:] == -1.0).all() and (curve[1:3] == -1.0).all()
    else:
        assert 0 < int(best[0].sum(dtype=U64)) < 1 << 20 and int(mass[0].sum(dtype=U64)) < 1 << 50      # both wrapped back
        assert (curve[0, 0] >= 0).all()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_diversity_symbols_exist_and_refuse_what_the_header_says():
    lib = capi.load()
    names = ("epik_amd_cohort_alpha_device", "epik_amd_cohort_alpha", "epik_amd_cohort_alpha_host",
             "epik_amd_cohort_rarefy_device", "epik_amd_cohort_rarefy", "epik_amd_cohort_rarefy_host")
    for name in names:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == _header_symbols() and capi.ABI_VERSION == 3
    assert capi.ALPHA.itemsize == 40 and [capi.ALPHA.fields[k][1] for k in FIELDS] == [0, 8, 16, 24, 32]
    assert (capi.DIVERSITY_BLOCK, capi.RAREFY_MAX_DEPTHS, capi.RAREFY_MAX_DEPTH) == (256, 256, 1 << 20)
    err = lambda: lib.epik_amd_last_error().decode()
    out = np.zeros(2, dtype=capi.ALPHA)
    curve = np.zeros((2, 256, 2))
    assert lib.epik_amd_cohort_alpha_device(None, None, None, None, None) == capi.ERR_INVALID and "null cohort" in err()
    assert lib.epik_amd_cohort_alpha(None, None, None, out.ctypes.data) == capi.ERR_INVALID and "null cohort" in err()
    assert lib.epik_amd_cohort_rarefy_device(None, None, None, 1, 1, None, None) == capi.ERR_INVALID and "null cohort" in err()
    assert lib.epik_amd_cohort_rarefy(None, None, None, 1, 1, curve.ctypes.data) == capi.ERR_INVALID and "null cohort" in err()
    first = cohort_mod.first_of([2, 2, -1])
    cells = np.ones((2, 3), U64)
    bl = np.ones(3)
    ptr = lambda x: x.ctypes.data if x is not None else None
    alpha_args = lambda m=cells, s=2, n=3, f=first, l=bl, o=out: (ptr(m), s, n, ptr(f), ptr(l), ptr(o))
    rarefy_args = lambda m=cells, s=2, n=3, f=first, l=bl, step=1, depths=3, o=curve: (ptr(m), s, n, ptr(f), ptr(l), step, depths, ptr(o))
    assert lib.epik_amd_cohort_alpha_host(*alpha_args()) == capi.OK and lib.epik_amd_cohort_rarefy_host(*rarefy_args()) == capi.OK
    assert lib.epik_amd_cohort_rarefy_host(*rarefy_args(step=4096, depths=256)) == capi.OK
    assert lib.epik_amd_cohort_rarefy_host(*rarefy_args(step=1 << 20, depths=1)) == capi.OK
    for host, args in ((lib.epik_amd_cohort_alpha_host, alpha_args), (lib.epik_amd_cohort_rarefy_host, rarefy_args)):
        assert host(*args(s=0)) == capi.ERR_INVALID and "num_samples is 0" in err()
        assert host(*args(n=0)) == capi.ERR_INVALID and "at least one branch" in err()
        for missing in ("m", "f", "l", "o"):
            assert host(*args(**{missing: None})) == capi.ERR_INVALID and "null argument" in err(), missing
        assert host(*args(f=np.array([0, 2, 0], dtype=np.uint32))) == capi.ERR_INVALID and "branch 1" in err() and "first" in err()
        for bad in (-1.0, np.inf, np.nan):
            assert host(*args(l=np.array([1.0, 1.0, bad]))) == capi.ERR_INVALID and "branch 2" in err() and "length" in err()
    for bad in (0, (1 << 20) + 1, 0xFFFFFFFF):
        assert lib.epik_amd_cohort_rarefy_host(*rarefy_args(step=bad, depths=1)) == capi.ERR_INVALID and "depth_step" in err()
    for bad in (0, 257, 0xFFFFFFFF):
        assert lib.epik_amd_cohort_rarefy_host(*rarefy_args(depths=bad)) == capi.ERR_INVALID and "num_depths" in err() and "[1, 256]" in err()
    assert lib.epik_amd_cohort_rarefy_host(*rarefy_args(step=4097, depths=256)) == capi.ERR_INVALID
    assert "num_depths * depth_step" in err() and "2^20" in err()
    for step, depths in ((0, 4), (1, 0), (1, 257), (8192, 129)):
        with pytest.raises(capi.EpikAmdError):
            cohort_mod.rarefy_host(cells, first, bl, step, depths)
    with pytest.raises(ValueError):
        cohort_mod.alpha_host(cells, first[:2], bl)
    with pytest.raises(ValueError):
        cohort_mod.rarefy_host(cells, first, bl[:2], 1, 1)


# ---- the drivers and the launcher ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_drivers_refuse_the_flags_without_cohort_and_name_them(host_bins, tmp_path, binary):
    base = [os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "none.list"), "-o", str(tmp_path)]
    for extra, flag, needs in ((["--cohort-alpha"], "--cohort-alpha", "--cohort "),
                               (["--cohort-rarefy", "64"], "--cohort-rarefy", "--cohort "),
                               (["--cohort-rarefy", "64", "--cohort-rarefy-step", "4"], "--cohort-rarefy", "--cohort "),
                               (["--cohort", "--cohort-rarefy-step", "4"], "--cohort-rarefy-step", "--cohort-rarefy "),
                               (["--cohort", "--cohort-alpha", "--cohort-rarefy-step", "4"], "--cohort-rarefy-step", "--cohort-rarefy "),
                               (["--cohort", "--cohort-rarefy", "0"], "--cohort-rarefy ", "[1, 1048576]"),
                               (["--cohort", "--cohort-rarefy", "1048577"], "--cohort-rarefy ", "[1, 1048576]"),
                               (["--cohort", "--cohort-rarefy", "x"], "--cohort-rarefy ", "[1, 1048576]"),
                               (["--cohort", "--cohort-rarefy=-3"], "--cohort-rarefy ", "[1, 1048576]"),
                               (["--cohort", "--cohort-rarefy", "64", "--cohort-rarefy-step", "0"], "--cohort-rarefy-step", "[1, 1048576]"),
                               (["--cohort", "--cohort-rarefy", "64", "--cohort-rarefy-step", "2x"], "--cohort-rarefy-step", "[1, 1048576]"),
                               (["--cohort", "--cohort-rarefy", "64", "--cohort-rarefy-step", "65"], "--cohort-rarefy-step", "[1, 256]"),
                               (["--cohort", "--cohort-rarefy", "1000", "--cohort-rarefy-step", "3"], "--cohort-rarefy-step", "[1, 256]")):
        run = subprocess.run(base + extra, capture_output=True, text=True)
        assert run.returncode == 255, run.stdout + run.stderr
        assert run.stderr.startswith("Error:") and flag in run.stderr and needs in run.stderr, (extra, run.stderr)
        assert "Loading database" not in run.stdout and "HIP device" not in run.stderr and not list(tmp_path.iterdir())
    out = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort-alpha " in out.stdout and "--cohort-rarefy arg" in out.stdout
    assert "--cohort-rarefy-step arg" in out.stdout and "cohort_alpha_<list>.tsv" in out.stdout and "cohort_rarefy_<list>.tsv" in out.stdout


def test_launcher_passes_the_flags_only_when_given():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw)
    assert "--cohort-alpha" not in " ".join(default) and "--cohort-rarefy" not in " ".join(default)
    assert epik.driver_command(**kw, cohort_alpha=False, cohort_rarefy=None, cohort_rarefy_step=None) == default
    assert "--cohort-alpha" not in " ".join(epik.driver_command(**kw, cohort=True))
    assert epik.driver_command(**kw, cohort=True, cohort_alpha=True)[:-1] == default[:-1] + ["--cohort", "--cohort-alpha"]
    assert epik.driver_command(**kw, cohort=True, cohort_rarefy=64)[:-1] == default[:-1] + ["--cohort", "--cohort-rarefy", "64"]
    assert epik.driver_command(**kw, cohort=True, cohort_alpha=True, cohort_rarefy=64, cohort_rarefy_step=4)[:-1] == \
        default[:-1] + ["--cohort", "--cohort-alpha", "--cohort-rarefy", "64", "--cohort-rarefy-step", "4"]
    assert epik.driver_command(**kw, cohort=True, cohort_squash=True, cohort_epca=True, cohort_kmeans=2, cohort_alpha=True,
                               cohort_rarefy=1 << 20)[:-1] == \
        default[:-1] + ["--cohort", "--cohort-squash", "--cohort-epca", "--cohort-kmeans", "2", "--cohort-alpha", "--cohort-rarefy", "1048576"]
    for bad in (dict(cohort_alpha=True), dict(cohort_rarefy=64), dict(cohort=True, cohort_rarefy_step=4),
                dict(cohort=True, cohort_rarefy=64, cohort_rarefy_step=65), dict(cohort=True, cohort_rarefy=1000, cohort_rarefy_step=3)):
        with pytest.raises(click.UsageError):
            epik.driver_command(**kw, **bad)
    me = os.path.join(ROOT, "epik.py")
    out = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort-alpha" in out.stdout and "--cohort-rarefy-step" in out.stdout
    for flags in (["--cohort-alpha"], ["--cohort-rarefy", "64"]):
        run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, *flags, me], capture_output=True, text=True)
        assert run.returncode == 2 and "--cohort" in run.stderr and flags[0] in run.stderr, (run.stdout, run.stderr)
    for bad in (["--cohort-rarefy", "0"], ["--cohort-rarefy", "1048577"], ["--cohort-rarefy", "64", "--cohort-rarefy-step", "0"],
                ["--cohort-rarefy", "64", "--cohort-rarefy-step", "65"]):
        run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, "--cohort", *bad, me], capture_output=True, text=True)
        assert run.returncode == 2 and bad[-2] in run.stderr, (run.stdout, run.stderr)


def test_the_two_files_read_back_and_keep_names(tmp_path):
    names = ["a", "skin 3", "it's", "none", "z.9_-"]
    parent, bl = tree_case("tree15")
    first = numpy_first(parent)
    rng = np.random.default_rng(8)
    mass = random_cells(rng, 5, len(parent), bits=42)
    mass[3] = 0
    best = draw_best(rng, 5, len(parent), 4, 16)                 # reads: 101, 32, 1, 0, 22
    alpha = cohort_mod.alpha_host(mass, first, bl)
    text = cohort_mod.format_alpha_tsv(names, alpha)
    lines = text.split("\n")
    assert lines[:3] == ["# epik_amd alpha v1  samples=5 used=4", "# unused\tnone", "name\tpd\trooted_pd\tbwpd_0.5\tbwpd_1\tquadratic_entropy"]
    assert lines[3] == "a" + "".join("\t%.17g" % alpha[f][0] for f in FIELDS)
    assert [ln.split("\t")[0] for ln in lines[3:7]] == ["a", "skin 3", "it's", "z.9_-"] and len(lines) == 8 and lines[-1] == ""
    path = tmp_path / "cohort_alpha_x.tsv"
    path.write_bytes(text.encode())
    back_names, back, info = cohort_mod.read_alpha_tsv(str(path))
    assert back_names == ["a", "skin 3", "it's", "z.9_-"] and info == {"samples": 5, "used": 4, "unused": ["none"]}
    assert same_records(back, alpha[[0, 1, 2, 4]])
    curve = cohort_mod.rarefy_host(best, first, bl, 4, 16)
    reads = cohort_mod.reads_of(best)
    assert list(reads) == [101, 32, 1, 0, 22]
    text = cohort_mod.format_rarefy_tsv(names, reads, 4, curve)
    lines = text.split("\n")
    assert lines[:3] == ["# epik_amd rarefy v1  samples=5 used=4 step=4 depths=16", "# unused\tnone", "name\tk\treads\tpd\trooted_pd"]
    assert lines[3] == "a\t4\t101\t%.17g\t%.17g" % (curve[0, 0, 0], curve[0, 0, 1])
    assert len(lines) == 3 + 16 + 8 + 0 + 5 + 1          # a sample with one read is used and has no depth to show
    rarefy_path = tmp_path / "cohort_rarefy_x.tsv"
    rarefy_path.write_bytes(text.encode())
    rows, info = cohort_mod.read_rarefy_tsv(str(rarefy_path))
    assert info == {"samples": 5, "used": 4, "step": 4, "depths": 16, "unused": ["none"]}
    assert [r[:3] for r in rows[16:24]] == [("skin 3", 4 * (j + 1), 32) for j in range(8)]
    assert same_bits([r[3:] for r in rows[16:24]], curve[1, :8]) and rows[-1][:3] == ("z.9_-", 20, 22)
    path.write_text("# something else\n")
    with pytest.raises(ValueError):
        cohort_mod.read_alpha_tsv(str(path))
    with pytest.raises(ValueError):
        cohort_mod.read_rarefy_tsv(str(path))
    with pytest.raises(ValueError):
        cohort_mod.format_alpha_tsv(names[:4], alpha)
    with pytest.raises(ValueError):
        cohort_mod.format_rarefy_tsv(names[:4], reads, 4, curve)
    # nothing used: the first line, the unused samples, the column names alone
    zero = np.zeros((2, len(first)), U64)
    assert cohort_mod.format_alpha_tsv(["x y", "q"], cohort_mod.alpha_host(zero, first, bl)) == (
        "# epik_amd alpha v1  samples=2 used=0\n# unused\tx y\n# unused\tq\nname\tpd\trooted_pd\tbwpd_0.5\tbwpd_1\tquadratic_entropy\n")
    assert cohort_mod.format_rarefy_tsv(["x y", "q"], [0, 1 << 53], 2, cohort_mod.rarefy_host(zero, first, bl, 2, 3)) == (
        "# epik_amd rarefy v1  samples=2 used=0 step=2 depths=3\n# unused\tx y\n# unused\tq\nname\tk\treads\tpd\trooted_pd\n")


# ---- the host code stand-alone -----------------------------------------------------------------------------------------
def _cells_input(path, cells, first, bl):
    with open(path, "wb") as fh:
        fh.write(np.array(cells.shape, dtype="<u8").tobytes() + np.ascontiguousarray(cells, U64).tobytes() +
                 np.ascontiguousarray(first, np.uint32).tobytes() + np.ascontiguousarray(bl, np.float64).tobytes())


@pytest.mark.parametrize("sanitized", [False, True])
def test_host_test_binary_alpha_and_rarefy_are_the_library_s(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    cases = [(tree_case("tree15"), 7), (tree_case("tree2999"), 3)]
    cases += [((parent, bl), len(mass)) for name, (mass, _, parent, bl) in forged_diversity_cohorts().items()]
    forged = [None, None] + list(forged_diversity_cohorts().values())
    for i, ((parent, bl), num_samples) in enumerate(cases):
        first = numpy_first(parent)
        rng = np.random.default_rng(9 + i)
        mass = forged[i][0] if forged[i] else random_cells(rng, num_samples, len(parent), empty=1, bits=42)
        best = forged[i][1] if forged[i] else draw_best(rng, num_samples, len(parent), 7, 40)
        _cells_input(tmp_path / "mass.bin", mass, first, bl)
        _cells_input(tmp_path / "best.bin", best, first, bl)
        run = subprocess.run([binary, "alpha", str(tmp_path / "out.bin"), str(tmp_path / "mass.bin")], capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (i, run.stderr)
        assert (tmp_path / "out.bin").read_bytes() == cohort_mod.alpha_host(mass, first, bl).tobytes(), i
        for step, depths in ((7, 40), (1, 256)):
            run = subprocess.run([binary, "rarefy", str(tmp_path / "out.bin"), str(tmp_path / "best.bin"), str(step), str(depths)],
                                 capture_output=True, text=True)
            assert run.returncode == 0 and not run.stderr, (i, run.stderr)
            assert (tmp_path / "out.bin").read_bytes() == cohort_mod.rarefy_host(best, first, bl, step, depths).tobytes(), (i, step)
    for step, depths, word in (("0", "4", "depth_step"), ("1", "257", "num_depths"), ("4097", "256", "2^20")):
        run = subprocess.run([binary, "rarefy", str(tmp_path / "o.bin"), str(tmp_path / "best.bin"), step, depths], capture_output=True, text=True)
        assert run.returncode == 1 and word in run.stderr
