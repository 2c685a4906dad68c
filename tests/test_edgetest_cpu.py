"""The edge test (which branches differ between the groups of a factor column: per-branch ANOVA and Kruskal-Wallis by
permutation, max-statistic adjusted) without a GPU: the host mirror (epik_amd_cohort_edgetest_host) against values worked out
by hand and against the rule restated in numpy, bit for bit on the records, on every eta of every labelling and on the maxima;
sanity on the same cases; the exhaustive share; the labellings shared with PERMANOVA; the capped factor reader; the drivers,
the launcher, the formatters and the stand-alone test binary.
"""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, synth
from test_cohort_cpu import host_bins, numpy_first, random_cells, same_bits  # noqa: F401 (host_bins: a fixture)
from test_permanova_cpu import MISSING, NA, numpy_labellings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
FAMILY_DOUBLES = ("eta2", "stat", "p", "p_adj")
FAMILY_COUNTS = ("at_least", "max_at_least")


# ---- the rule restated --------------------------------------------------------------------------------------------------------
def numpy_vectors(mass, first):
    """xm[S][N], xi[S][N] of the correlation rule (rows of samples without mass mean nothing) and inner[N]."""
    mass = np.asarray(mass, dtype=U64)
    s, n = mass.shape
    first = np.asarray(first, dtype=np.int64)
    prefix = np.zeros((s, n + 1), dtype=U64)
    np.cumsum(mass, axis=1, dtype=U64, out=prefix[:, 1:])
    total = prefix[:, n]
    clade = prefix[:, 1:] - prefix[:, first]
    below = clade - mass
    with np.errstate(invalid="ignore", divide="ignore"):
        t = total.astype(np.float64)[:, None]
        xm = mass.astype(np.float64) / t
        xi = (below.astype(np.float64) / t + clade.astype(np.float64) / t) - 1.0
    return xm, xi, first < np.arange(n), total


def numpy_midranks(x):
    """Midranks down the columns of x[L][K] by the two counts."""
    less = np.zeros(x.shape, dtype=np.int64)
    equal = np.zeros(x.shape, dtype=np.int64)
    for i in range(x.shape[0]):
        less += x[i][None, :] < x
        equal += x[i][None, :] == x
    return less.astype(np.float64) + 0.5 * (equal + 1).astype(np.float64)


def column_groups(labels_c, total):
    used, lam, sizes, group_of = [], [], [], {}
    for s, v in enumerate(labels_c):
        if int(total[s]) == 0 or int(v) == MISSING:
            continue
        if int(v) not in group_of:
            group_of[int(v)] = len(sizes)
            sizes.append(0)
        used.append(s), lam.append(group_of[int(v)])
        sizes[group_of[int(v)]] += 1
    return np.array(used, dtype=np.int64), np.array(lam, dtype=np.int64), sizes


def numpy_eta(d, mu, sizes):
    """eta's numerator A(mu) for d[4][L][N] and mu[P + 1][L]: one loop over the positions that adds d[i] into the accumulator
    of mu_i of every labelling; nothing is summed by np.sum.  Returns A [P + 1][4][N] and the sums S_g [P + 1][G][4][N]."""
    rows = np.arange(mu.shape[0])
    acc = np.zeros((mu.shape[0], len(sizes)) + d[:, 0, :].shape)
    for i in range(mu.shape[1]):
        acc[rows, mu[:, i], :] += d[:, i, :]
    among = np.zeros((mu.shape[0],) + d[:, 0, :].shape)
    for g, n_g in enumerate(sizes):
        among = among + (acc[:, g] * acc[:, g]) / float(n_g)
    return among, acc


def numpy_edgetest(mass, first, labels, permutations, seed, labellings=numpy_labellings):
    mass, labels = np.asarray(mass, dtype=U64), np.asarray(labels)
    s, n = mass.shape
    m, row = labels.shape[1], permutations + 1
    xm, xi, inner, total = numpy_vectors(mass, first)
    records = np.zeros((m, n), dtype=capi.EDGETEST)
    for f in FAMILY_DOUBLES:
        records["family"][f] = NA
    records["top_mass"] = records["top_imbalance"] = MISSING
    stat, most = np.full((m, 4, n, row), NA), np.full((m, 4, row), NA)
    for c in range(m):
        used, lam, sizes = column_groups(labels[:, c], total)
        L, G = len(used), len(sizes)
        records["used"][c], records["groups"][c] = L, G
        if G < 2 or L - G < 1:
            continue
        mu = labellings(lam, seed, permutations)
        x = np.stack([xm[used], numpy_midranks(xm[used]), xi[used], numpy_midranks(xi[used])])      # [4][L][N]
        acc = np.zeros((4, n))
        for i in range(L):
            acc = acc + x[:, i, :]
        d = x - (acc / float(L))[:, None, :]
        sxx = np.zeros((4, n))
        for i in range(L):
            sxx = sxx + d[:, i, :] * d[:, i, :]
        defined = (sxx > 0.0) & (inner[None, :] | (np.arange(4) < 2)[:, None])                       # [4][N]
        among, sums = numpy_eta(d, mu, sizes)
        with np.errstate(invalid="ignore", divide="ignore"):
            eta = among / sxx[None]                                                                  # [P + 1][4][N]
            ssw = sxx - among[0]
            f_stat = (among[0] / float(G - 1)) / (ssw / float(L - G))
            means = sums[0] / np.array(sizes, dtype=np.float64)[:, None, None]                       # [G][4][N]
        eta2 = eta[0]
        for f in range(4):
            if not defined[f].any():
                continue
            live = defined[f]
            mmax = eta[:, f, live].max(axis=1)                                                       # [P + 1]
            most[c, f] = mmax
            stat[c, f, live, :] = eta[:, f, live].T
            fam = records["family"][c, :, f]
            fam["eta2"][live] = eta2[f, live]
            fam["stat"][live] = np.where(ssw[f, live] > 0.0, f_stat[f, live], NA) if f % 2 == 0 else float(L - 1) * eta2[f, live]
            at_least = (eta[1:, f, :] >= eta2[f][None, :]).sum(axis=0)
            max_at_least = (mmax[1:, None] >= eta2[f][None, :]).sum(axis=0)
            fam["at_least"][live], fam["max_at_least"][live] = at_least[live], max_at_least[live]
            fam["p"][live] = (1 + at_least[live]).astype(np.float64) / float(permutations + 1)
            fam["p_adj"][live] = (1 + max_at_least[live]).astype(np.float64) / float(permutations + 1)
            records["family"][c, :, f] = fam
            if f % 2 == 0:
                top = np.argmax(means[:, f, :], axis=0)                                              # (the lowest g of a tie)
                name = "top_mass" if f == 0 else "top_imbalance"
                records[name][c] = np.where(live, top, MISSING)
    return cohort_mod.Edgetest(records, stat, most)


def only_na_or_numbers(result):
    """No arithmetic NaN reaches an output: a NaN is the NA pattern."""
    arrays = [result.records["family"][f] for f in FAMILY_DOUBLES] + [v for v in (result.stat, result.max) if v is not None]
    for v in arrays:
        v = np.ascontiguousarray(v)
        assert (v.view(U64)[np.isnan(v)] == U64(capi.NA_BITS)).all()
        assert not np.isinf(v).any()


def same_edgetest(got, want, what=""):
    for f in ("used", "groups", "top_mass", "top_imbalance"):
        assert np.array_equal(got.records[f], want.records[f]), (what, f, np.argwhere(got.records[f] != want.records[f])[:8])
    for f in FAMILY_COUNTS:
        a, b = got.records["family"][f], want.records["family"][f]
        assert np.array_equal(a, b), (what, f, np.argwhere(a != b)[:8])
    for f in FAMILY_DOUBLES:
        a, b = np.ascontiguousarray(got.records["family"][f]), np.ascontiguousarray(want.records["family"][f])
        assert same_bits(a, b), (what, f, np.argwhere(a.view(U64) != b.view(U64))[:8])
    for name in ("stat", "max"):
        a, b = getattr(got, name), getattr(want, name)
        if a is not None and b is not None:
            assert same_bits(a, b), (what, name, np.argwhere(a.view(U64) != b.view(U64))[:8])
    only_na_or_numbers(got)
    return True


TREES = {}


def edge_tree(num_branches):
    """(parent, first) of a random tree of 7 or 999 branches, or the cherry of 3."""
    if num_branches not in TREES:
        parent = np.array([2, 2, -1]) if num_branches == 3 else np.asarray(synth.make_tree((num_branches + 1) // 2, seed=30).parent)
        assert len(parent) == num_branches
        TREES[num_branches] = (np.asarray(parent, dtype=np.int64), numpy_first(parent))
    return TREES[num_branches]


def sparser(rng, mass):
    """`mass` with nine cells in ten zeroed."""
    out = mass.copy()
    out[rng.random(out.shape) < 0.9] = 0
    return out


def factor_labels(rng, num_samples):
    """labels [S][4]: two groups; three unbalanced groups with a fifth missing; seven groups under scattered ids below 32;
    one single group (undefined)."""
    s = num_samples
    cols = [rng.integers(0, 2, size=s), np.where(rng.random(s) < 0.2, MISSING, rng.choice(3, size=s, p=[0.6, 0.3, 0.1])),
            np.array([31, 20, 3, 7, 0, 30, 12])[np.minimum(rng.geometric(0.35, size=s) - 1, 6)], np.full(s, 17)]
    return np.ascontiguousarray(np.array(cols, dtype=np.uint32).T)


# ---- 1. by hand -------------------------------------------------------------------------------------------------------------
HAND_PARENT = np.array([2, 2, 4, 4, -1])
HAND_MASS = np.array([[4, 2, 0, 2, 0], [2, 4, 0, 2, 0], [1, 1, 2, 4, 0], [1, 1, 0, 6, 0]], dtype=U64)


def test_three_leaves_four_samples_by_hand():
    """Leaves 0, 1 under the inner branch 2; leaf 3; root 4.  Every sample has mass 8; the groups are a a b b.
    Branch 0, mass: x = 1/2 1/4 1/8 1/8, mx = 1/4, d = 1/4 0 -1/8 -1/8, sxx = 3/32; S_a = 1/4, S_b = -1/4, A = 1/32 + 1/32 = 1/16;
      eta2 = (1/16) / (3/32); ssw = 1/32; F = (1/16) / ((1/32) / 2) = 4.  Its ranks 4 3 1.5 1.5: d = 1.5 0.5 -1 -1, sxx = 4.5,
      S = 2, -2, A = 4, eta2 = 4 / 4.5, H = 3 * eta2.  The larger mean is a's.
    Branch 3, mass: x = 1/4 1/4 1/2 3/4, mx = 7/16, d = -3/16 -3/16 1/16 5/16, sxx = 44/256; S = -3/8, 3/8; A = 9/64;
      ssw = 44/256 - 36/256 = 1/32; F = (9/64) / (1/64) = 9.  The larger mean is b's.
    Branch 2, mass: x = 0 0 1/4 0, mx = 1/16, sxx = 3/64, S = -1/8, 1/8, A = 1/64, eta2 = (1/64) / (3/64), ssw = 1/32, F = 1.
      Its ranks 2 2 4 2: d = -1/2 -1/2 3/2 -1/2, sxx = 3, S = -1, 1, A = 1: eta2 = 1/3, H = 3 * (1/3).
      Imbalance (B + C - 1): 1/2 1/2 -1/4 -1/2, mx = 1/16, d = 7/16 7/16 -5/16 -9/16, sxx = 204/256; S = 7/8, -7/8; A = 49/64;
      ssw = 1/32; F = (49/64) / (1/64) = 49; its ranks 3.5 3.5 2 1: sxx = 4.5, S = 2, -2: eta2 = 4 / 4.5.
    Branch 4 (the root): no mass in any sample and the imbalance 1 in every sample: no family is defined.  The leaves have
    no imbalance.  With P = 1 a p is 1/2 or 1: 1 iff the one relabelling's eta reaches eta2."""
    first = numpy_first(HAND_PARENT)
    labels = np.array([[5, 5, 2, 2]], dtype=np.uint32).T.copy()
    got = cohort_mod.edgetest_host(HAND_MASS, first, labels, permutations=1, seed=3)
    r = got.records[0]
    fam = r["family"]
    assert list(r["used"]) == [4] * 5 and list(r["groups"]) == [2] * 5
    assert same_bits(fam["eta2"][0], [(1 / 16) / (3 / 32), 4 / 4.5, NA, NA]) and same_bits(fam["stat"][0], [4.0, 3.0 * (4 / 4.5), NA, NA])
    assert same_bits(fam["eta2"][3][:2], [(9 / 64) / (44 / 256), 4 / 4.5]) and same_bits(fam["stat"][3][0], 9.0)
    assert same_bits(fam["eta2"][2], [(1 / 64) / (3 / 64), 1.0 / 3.0, (49 / 64) / (204 / 256), 4 / 4.5])
    assert same_bits(fam["stat"][2][[0, 2, 3]], [1.0, 49.0, 3.0 * (4 / 4.5)])
    assert same_bits(fam["stat"][2][1], 3.0 * (1.0 / 3.0))
    assert np.isnan(fam["eta2"][4]).all() and np.isnan(fam["p"][4]).all() and not fam["at_least"][4].any()
    assert list(r["top_mass"]) == [0, 0, 1, 1, MISSING] and list(r["top_imbalance"]) == [MISSING, MISSING, 0, MISSING, MISSING]
    defined = ~np.isnan(fam["eta2"])
    assert defined.sum() == 2 + 2 + 4 + 2
    reached = got.stat[0].transpose(1, 0, 2)[..., 1] >= fam["eta2"]                    # [N][4]
    assert same_bits(fam["p"][defined], np.where(reached[defined], 1.0, 0.5))
    assert set(np.unique(fam["p_adj"][defined])) <= {0.5, 1.0} and (fam["p_adj"][defined] >= fam["p"][defined]).all()
    assert same_bits(got.stat[0, :, :, 0].T[defined], fam["eta2"][defined])
    same_edgetest(got, numpy_edgetest(HAND_MASS, first, labels, 1, 3))
    # both of the other splits of 2 + 2 are below on branch 0's mass: with enough relabellings p tends to 1/3
    more = cohort_mod.edgetest_host(HAND_MASS, first, labels, permutations=300, seed=3)
    assert 0.2 < more.records["family"]["p"][0, 0, 0] < 0.5


# ---- 2. the host mirror against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("num_samples", [3, 4, 33, 65, 130])
@pytest.mark.parametrize("num_branches", [7, 999])
def test_host_equals_the_numpy_restatement_bit_for_bit(num_branches, num_samples):
    parent, first = edge_tree(num_branches)
    rng = np.random.default_rng(7000 + 10 * num_branches + num_samples)
    dense = random_cells(rng, num_samples, num_branches, empty=1, bits=42)
    some_defined = False
    for kind, mass in (("random_cells", dense), ("nine in ten zeroed", sparser(rng, dense))):
        labels = factor_labels(rng, num_samples)
        for permutations in (1, 63, 64, 65):
            seed = int(rng.integers(0, 1 << 63)) * 2 + 1
            got = cohort_mod.edgetest_host(mass, first, labels, permutations, seed)
            want = numpy_edgetest(mass, first, labels, permutations, seed)
            same_edgetest(got, want, (num_branches, num_samples, kind, permutations))
            fam = got.records["family"]
            both = ~np.isnan(fam["p"])
            assert np.array_equal(both, ~np.isnan(fam["p_adj"])) and np.array_equal(both, ~np.isnan(fam["eta2"]))
            assert (fam["p_adj"][both] >= fam["p"][both]).all() and (fam["max_at_least"] >= fam["at_least"]).all()
            assert np.isnan(fam["eta2"][3]).all() and (got.records["groups"][3] <= 1).all()              # one group: undefined
            inner = first < np.arange(num_branches)
            assert np.isnan(fam["eta2"][:, ~inner, 2:]).all()                                            # no imbalance of a leaf
            assert ((fam["eta2"][both] >= 0.0) & (fam["eta2"][both] <= 1.0 + 1e-12)).all()
            assert ((got.records["top_mass"] == MISSING) == np.isnan(fam["eta2"][..., 0])).all()
            some_defined = some_defined or both[0].any()
            lean = cohort_mod.edgetest_host(mass, first, labels, permutations, seed, with_stat=False, with_max=False)
            assert lean.stat is None and lean.max is None and lean.records.tobytes() == got.records.tobytes()
    assert some_defined == (num_samples >= 4)


# ---- 3. sanity -------------------------------------------------------------------------------------------------------------------
def test_one_defined_branch_identical_samples_and_disjoint_constant_shares():
    # the cherry: only the root is inner, so the imbalance families have one defined branch: p_adj is p, bit for bit
    parent, first = edge_tree(3)
    rng = np.random.default_rng(11)
    mass = random_cells(rng, 12, 3, bits=20) + U64(1)
    labels = np.array([[0, 1, 2] * 4], dtype=np.uint32).T.copy()
    got = cohort_mod.edgetest_host(mass, first, labels, 200, 5)
    fam = got.records["family"][0]
    assert not np.isnan(fam["eta2"][2, 2:]).any() and np.isnan(fam["eta2"][:2, 2:]).all()
    assert same_bits(fam["p_adj"][2, 2:], fam["p"][2, 2:]) and np.array_equal(fam["max_at_least"][2, 2:], fam["at_least"][2, 2:])
    assert same_bits(got.max[0, 2:], got.stat[0, 2:, 2, :])
    same_edgetest(got, numpy_edgetest(mass, first, labels, 200, 5))
    # identical samples: nothing varies, no family is defined; used and groups are still written.  (The masses sum to 16, so
    # every share and every sum of eight of them is exact: the rule's sxx > 0.0 is a comparison of computed doubles, and a
    # mean that rounds leaves deviations of an ulp, which the rule counts as variation.)
    parent, first = edge_tree(7)
    mass = np.tile(np.array([[1, 2, 1, 4, 0, 3, 5]], dtype=U64), (8, 1))
    labels = np.array([[0, 1] * 4], dtype=np.uint32).T.copy()
    got = cohort_mod.edgetest_host(mass, first, labels, 20, 1)
    assert np.isnan(got.records["family"]["eta2"]).all() and not got.records["family"]["at_least"].any()
    assert (got.records["used"] == 8).all() and (got.records["groups"] == 2).all() and (got.records["top_mass"] == MISSING).all()
    assert np.isnan(got.stat).all() and np.isnan(got.max).all()
    only_na_or_numbers(got)
    # two groups with disjoint constant shares on branch 0 (1/4 against 1/2): eta2 is 1 and F is NA (ssw = 0)
    first = numpy_first(HAND_PARENT)
    mass = np.array([[2, 1, 0, 5, 0], [2, 3, 0, 3, 0], [4, 1, 2, 1, 0], [4, 0, 0, 4, 0]], dtype=U64)
    labels = np.array([[0, 0, 1, 1]], dtype=np.uint32).T.copy()
    got = cohort_mod.edgetest_host(mass, first, labels, 50, 9)
    fam = got.records["family"][0, 0]
    assert same_bits(fam["eta2"][:2], [1.0, 1.0]) and np.isnan(fam["stat"][0]) and same_bits(fam["stat"][1], 3.0)
    assert not np.isnan(fam["p"][0]) and got.records["top_mass"][0, 0] == 1
    same_edgetest(got, numpy_edgetest(mass, first, labels, 50, 9))


def test_the_share_of_relabellings_follows_the_exact_share_of_all_720_orders():
    """L = 6 in groups of 3 + 3 and P = 20 000: the share of relabellings with eta >= eta2 lies within 0.02 of the share q
    over all 720 orders (were the draws independent and uniform, 0.02 would be more than five standard deviations,
    5 sqrt(q (1 - q) / P) <= 0.0177).  The seed is fixed: the check is deterministic."""
    parent, first = edge_tree(7)
    rng = np.random.default_rng(21)
    mass = random_cells(rng, 6, 7, bits=30) + U64(1)
    labels = np.array([[0, 1, 1, 0, 1, 0]], dtype=np.uint32).T.copy()
    lam = labels[:, 0].astype(np.int64)
    every = np.array([lam] + [lam[list(sigma)] for sigma in itertools.permutations(range(6))])
    exact = numpy_edgetest(mass, first, labels, 720, 0, labellings=lambda *_: every)
    permutations = 20000
    got = cohort_mod.edgetest_host(mass, first, labels, permutations, 1, with_stat=False)
    fam, want = got.records["family"][0], exact.records["family"][0]
    defined = ~np.isnan(fam["eta2"])
    assert defined.sum() >= 12 and same_bits(fam["eta2"], want["eta2"])
    q = want["at_least"][defined] / 720.0
    share = fam["at_least"][defined] / float(permutations)
    print("q", q, "share", share)
    assert (q > 0.0).all() and (np.abs(share - q) <= 0.02).all()
    q_adj = want["max_at_least"][defined] / 720.0
    assert (np.abs(fam["max_at_least"][defined] / float(permutations) - q_adj) <= 0.02).all()


def test_the_labellings_are_permanova_s():
    """The same seed and column under both rules: PERMANOVA's SSW of every permutation and the edge test's eta of one branch
    are both functions of the same labellings, numpy_labellings (test_permanova_cpu): another seed gives other values."""
    from test_permanova_cpu import numpy_permanova
    parent, first = edge_tree(7)
    rng = np.random.default_rng(31)
    mass = random_cells(rng, 9, 7, empty=4, bits=30)
    labels = np.array([[0, 1, 2, 0, MISSING, 1, 2, 0, 1]], dtype=np.uint32).T.copy()
    bl = np.ones(7)
    permutations, seed = 40, 77
    used, lam, sizes = column_groups(labels[:, 0], mass.sum(axis=1, dtype=U64))
    mu = numpy_labellings(lam, seed, permutations)
    got = cohort_mod.edgetest_host(mass, first, labels, permutations, seed)
    want = numpy_edgetest(mass, first, labels, permutations, seed, labellings=lambda *_: mu)
    branch = int(np.flatnonzero(~np.isnan(got.records["family"]["eta2"][0, :, 0]))[0])
    assert same_bits(got.stat[0, 0, branch], want.stat[0, 0, branch]) and len(set(got.stat[0, 0, branch])) > 3
    other = cohort_mod.edgetest_host(mass, first, labels, permutations, seed + 1)
    assert not same_bits(other.stat[0, 0, branch, 1:], got.stat[0, 0, branch, 1:])
    assert same_bits(other.stat[0, 0, branch, 0], got.stat[0, 0, branch, 0])
    perm = cohort_mod.permanova_host(mass, first, bl, labels, permutations, seed)
    kr = cohort_mod.kr_host(mass, first, bl)
    restated = numpy_permanova(kr, cohort_mod.totals_of(mass), labels, permutations, seed, False)
    assert same_bits(perm.ssw, restated.ssw)


# ---- 4. the C ABI ---------------------------------------------------------------------------------------------------------------
def test_edgetest_symbols_exist_and_refuse_what_the_header_says():
    lib = capi.load()
    for name in ("epik_amd_cohort_edgetest_device", "epik_amd_cohort_edgetest", "epik_amd_cohort_edgetest_host"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert capi.ABI_VERSION == 3 and capi.EDGETEST.itemsize == 208 and capi.EDGETEST_FAMILY.itemsize == 48
    assert [capi.EDGETEST.fields[k][1] for k in capi.EDGETEST.names] == [0, 4, 8, 200, 204]
    assert capi.EDGETEST_MAX_GROUPS == 32
    err = lambda: lib.epik_amd_last_error().decode()
    labels = np.zeros((4, 1), np.uint32)
    out = np.zeros(3, dtype=capi.EDGETEST)
    assert lib.epik_amd_cohort_edgetest_device(None, None, labels.ctypes.data, 1, 9, 1, None, None, None, None) == capi.ERR_INVALID
    assert "null cohort" in err()
    assert lib.epik_amd_cohort_edgetest(None, None, labels.ctypes.data, 1, 9, 1, out.ctypes.data, None, None) == capi.ERR_INVALID
    assert "null cohort" in err()
    first = cohort_mod.first_of([2, 2, -1])
    cells = np.ones((4, 3), U64)
    ptr = lambda x: x.ctypes.data if x is not None else None
    args = lambda m=cells, s=4, n=3, f=first, l=labels, c=1, p=9, seed=1, o=out: (ptr(m), s, n, ptr(f), ptr(l), c, p, seed, ptr(o), None, None)
    host = lib.epik_amd_cohort_edgetest_host
    assert host(*args()) == capi.OK and host(*args(seed=(1 << 64) - 1)) == capi.OK
    assert host(*args(s=0)) == capi.ERR_INVALID and "num_samples is 0" in err()
    assert host(*args(n=0)) == capi.ERR_INVALID and "at least one branch" in err()
    for missing in ("m", "f", "l", "o"):
        assert host(*args(**{missing: None})) == capi.ERR_INVALID and "null argument" in err(), missing
    assert host(*args(f=np.array([0, 2, 0], dtype=np.uint32))) == capi.ERR_INVALID and "branch 1" in err()
    for bad in (0, 65, 0xFFFFFFFF):
        assert host(*args(c=bad)) == capi.ERR_INVALID and "num_columns" in err() and "[1, 64]" in err()
    for bad in (0, 1_000_000, 0xFFFFFFFF):
        assert host(*args(p=bad)) == capi.ERR_INVALID and "num_permutations" in err() and "[1, 999999]" in err()
    for bad in (32, 255, 0xFFFFFFFE):
        wrong = labels.copy()
        wrong[2, 0] = bad
        assert host(*args(l=wrong)) == capi.ERR_INVALID and "sample 2" in err() and "column 0" in err() and "32" in err()
    fine = labels.copy()
    fine[2, 0] = 31
    assert host(*args(l=fine)) == capi.OK
    with pytest.raises(ValueError):
        cohort_mod.edgetest_host(cells, first, np.zeros((3, 1), np.uint32))
    with pytest.raises(capi.EpikAmdError):
        cohort_mod.edgetest_host(cells, first, np.zeros((4, 0), np.uint32))
    with pytest.raises(capi.EpikAmdError):
        cohort_mod.edgetest_host(cells, first, labels, permutations=0)


# ---- 5. the factor file ---------------------------------------------------------------------------------------------------------
def test_the_factor_file_s_cap_is_an_argument(tmp_path):
    path = tmp_path / "factors.tsv"
    wide = [f"s{i}" for i in range(33)]
    path.write_text("sample\tone\tmany\nstranger\tq\tanother\n" + "".join(f"s{i}\tk\tv{i}\n" for i in range(33)))
    with pytest.raises(ValueError) as e:
        cohort_mod.read_factors(str(path), wide, most=capi.EDGETEST_MAX_GROUPS)
    assert all(w in str(e.value) for w in ("line 35", "column many", "'v32'", "label number 33", "more than 32")), str(e.value)
    assert "pairwise" not in str(e.value)
    columns, labels, label_names, skipped = cohort_mod.read_factors(str(path), wide[:32], most=capi.EDGETEST_MAX_GROUPS)
    assert columns == ["one", "many"] and skipped == 2 and len(label_names[1]) == 32 and labels[:, 1].tolist() == list(range(32))
    # without the new argument: exactly as before (256, or 32 and its words with pairwise)
    assert len(cohort_mod.read_factors(str(path), wide)[2][1]) == 33
    with pytest.raises(ValueError) as e:
        cohort_mod.read_factors(str(path), wide, True)
    assert "more than 32 (the most of --cohort-permanova-pairwise)" in str(e.value) and "line 35" in str(e.value)
    again = cohort_mod.read_factors(str(path), wide[:32], False, None)
    assert again[0] == columns and np.array_equal(again[1], labels) and again[2] == label_names


# ---- 6. the output file -----------------------------------------------------------------------------------------------------------
def _cells_input(path, cells, first):
    with open(path, "wb") as fh:
        fh.write(np.array(cells.shape, dtype="<u8").tobytes() + np.ascontiguousarray(cells, U64).tobytes() +
                 np.ascontiguousarray(first, np.uint32).tobytes() + np.ones(cells.shape[1]).tobytes())


FILE_NAMES = ["a", "skin 3", "it's", "none", "z.9_-", "q", "r", "s", "t"]
FILE_FACTORS = ("sample\tstate\tsite\tlone\n"
                "q\tsick\tgut\tx\n" "a\thealthy\tskin\tx\n" "skin 3\tsick\tskin\tx\n" "it's\thealthy\tgut\tx\n" "none\tsick\tmouth\tx\n"
                "z.9_-\thealthy\tNA\tx\n" "r\tsick\tgut\tx\n" "s\thealthy\tmouth of 2\tx\n" "t\tsick\tgut\tx\n" "other\t1\t2\t3\n")


def test_the_file_reads_back_and_the_python_and_the_c_formatters_agree(host_bins, tmp_path):
    parent, first = edge_tree(7)
    rng = np.random.default_rng(8)
    mass = random_cells(rng, 9, 7, bits=42)
    mass[3] = 0
    mass[:, 5] = 0                                                              # a branch without mass: no line of its own as a leaf
    (tmp_path / "factors.tsv").write_text(FILE_FACTORS)
    columns, labels, label_names, skipped = cohort_mod.read_factors(str(tmp_path / "factors.tsv"), FILE_NAMES, most=32)
    assert skipped == 1 and columns == ["state", "site", "lone"]
    result = cohort_mod.edgetest_host(mass, first, labels, 99, 7, with_stat=False, with_max=False)
    totals = cohort_mod.totals_of(mass)
    text = cohort_mod.format_edgetest_tsv(FILE_NAMES, totals, columns, label_names, labels, 99, 7, result.records)
    lines = text.split("\n")
    assert lines[:5] == ["# epik_amd edgetest v1  samples=9 used=8 columns=3 permutations=99 seed=7",
                         "# unused\tnone", "# column\t0\tstate\t8\t2", "# column\t1\tsite\t7\t3", "# column\t2\tlone\t8\t1"]
    assert lines[5:7] == ["# group\t0\t0\thealthy\t4", "# group\t0\t1\tsick\t4"]
    assert [ln.split("\t")[3:] for ln in lines[7:10]] == [["skin", "2"], ["gut", "4"], ["mouth of 2", "1"]]
    assert lines[10] == "# group\t2\t0\tx\t8" and lines[11] == cohort_mod.EDGETEST_HEADER
    assert cohort_mod.EDGETEST_HEADER.split("\t")[:10] == ["edge_num", "column", "mass_eta2", "mass_f", "mass_p", "mass_p_adj", "mass_top",
                                                          "mass_h", "mass_kw_p", "mass_kw_p_adj"]
    fam = result.records["family"]
    defined = ~np.isnan(fam["eta2"]).all(axis=2)                                # [M][N]
    assert not defined[2].any() and defined[0].sum() >= 5 and len(lines) == 12 + defined.sum() + 1 and lines[-1] == ""
    b = int(np.flatnonzero(defined[0])[0])
    r = result.records[0, b]
    top = label_names[0][cohort_mod.groups_of(labels, totals)[0][0][int(r["top_mass"])]]
    start = f"{b}\tstate\t%.17g\t%.17g\t%.17g\t%.17g\t{top}\t%.17g\t%.17g\t%.17g\t" % (
        r["family"][0]["eta2"], r["family"][0]["stat"], r["family"][0]["p"], r["family"][0]["p_adj"], r["family"][1]["stat"],
        r["family"][1]["p"], r["family"][1]["p_adj"])
    assert lines[12].startswith(start), (lines[12], start)
    if first[b] == b:
        assert lines[12].endswith("\tNA" * 8)
    path = tmp_path / "cohort_edgetest_x.tsv"
    path.write_text(text)
    back_columns, rows, groups, info = cohort_mod.read_edgetest_tsv(str(path))
    assert back_columns == columns and info["unused"] == ["none"] and info["permutations"] == 99 and info["seed"] == 7
    assert info["column_used"] == [8, 7, 8] and info["column_groups"] == [2, 3, 1] and groups[2] == (1, 0, "skin", 2)
    assert len(rows) == defined.sum() and rows[0]["edge_num"] == b and rows[0]["column"] == "state" and rows[0]["mass_top"] == top
    assert same_bits(rows[0]["mass_eta2"], r["family"][0]["eta2"]) and same_bits(rows[0]["mass_kw_p_adj"], r["family"][1]["p_adj"])
    assert [(row["column"], row["edge_num"]) for row in rows] == [(columns[c], int(e)) for c, e in np.argwhere(defined)]
    # the C++ reader and formatter over the C++ mirror: the same bytes
    _cells_input(tmp_path / "mass.bin", mass, first)
    (tmp_path / "names.txt").write_text("".join(name + "\n" for name in FILE_NAMES))
    run = subprocess.run([os.path.join(host_bins, "cohort_test"), "edgetest-tsv", str(tmp_path / "cpp.tsv"), str(tmp_path / "mass.bin"),
                          str(tmp_path / "names.txt"), str(tmp_path / "factors.tsv"), "99", "7"], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr
    assert "3 columns, 1 lines of samples that are not in the list skipped" in run.stdout
    assert (tmp_path / "cpp.tsv").read_bytes() == text.encode()
    path.write_text("# something else\n")
    with pytest.raises(ValueError):
        cohort_mod.read_edgetest_tsv(str(path))
    with pytest.raises(ValueError):
        cohort_mod.format_edgetest_tsv(FILE_NAMES[:4], totals, columns, label_names, labels, 99, 7, result.records)


# ---- 7. the launcher and the drivers ------------------------------------------------------------------------------------------
DEPENDENTS = (["--cohort-edge-test-permutations", "99"], ["--cohort-edge-test-seed", "5"])


@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_drivers_refuse_the_flags_and_read_the_factors_before_the_database(host_bins, tmp_path, binary):
    out = tmp_path / "out"
    out.mkdir()
    base = [os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "none.list"), "-o", str(out)]

    def refused(extra, *words):
        run = subprocess.run(base + extra, capture_output=True, text=True)
        assert run.returncode == 255 and run.stderr.startswith("Error:"), (extra, run.stdout + run.stderr)
        assert all(w in run.stderr for w in words), (extra, run.stderr)
        assert "Loading database" not in run.stdout and "HIP device" not in run.stderr and not list(out.iterdir())
        return run

    refused(["--cohort-edge-test", "f.tsv"], "--cohort-edge-test", "--cohort ")
    refused(["--cohort-edge-test", "f.tsv", "--cohort-alpha"], "--cohort ")
    for dependent in DEPENDENTS:
        refused(dependent, dependent[0], "needs --cohort-edge-test")
        refused(["--cohort"] + dependent, dependent[0], "needs --cohort-edge-test")
        refused(["--cohort", "--cohort-permanova", "f.tsv"] + dependent, dependent[0], "needs --cohort-edge-test")
    shown = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert shown.returncode == 0 and "cohort_edgetest_<list>.tsv" in shown.stdout
    for flag in ("--cohort-edge-test arg", "--cohort-edge-test-permutations arg", "--cohort-edge-test-seed arg"):
        assert flag in shown.stdout, flag
    for name in "abc":
        (tmp_path / f"{name}.fasta").write_text(">r\nACGT\n")
    (tmp_path / "samples.list").write_text("a\ta.fasta\nb\tb.fasta\nc\tc.fasta\n")
    base[4] = str(tmp_path / "samples.list")
    factors = str(tmp_path / "factors.tsv")
    (tmp_path / "factors.tsv").write_text("sample\tstate\na\tx\nb\ty\nc\tx\n")
    for value in ("0", "1000000", "many", "12x"):
        refused(["--cohort", "--cohort-edge-test", factors, "--cohort-edge-test-permutations", value], "--cohort-edge-test-permutations",
                "[1, 999999]")
    for value in ("18446744073709551616", "seed", "7x"):
        refused(["--cohort", "--cohort-edge-test", factors, "--cohort-edge-test-seed", value], "--cohort-edge-test-seed", "uint64")
    head = "sample\tstate\tsite\n"
    for text, words in ((head + "a\tx\ty\nb\tx\nc\tx\ty\n", ("line 3", "2 fields, not 3")),
                        (head + "a\tx\ty\nb\tx\ty\na\tz\tw\nc\tx\ty\n", ("line 4", "'a'", "twice")),
                        (head + "a\tx\ty\nb\tx\ty\n", ("no line", "'c'")),
                        ("sample\tstate\tstate\n", ("line 1", "'state'", "twice")),
                        (None, ("cannot open",))):
        if text is not None:
            (tmp_path / "factors.tsv").write_text(text)
        else:
            os.remove(tmp_path / "factors.tsv")
        refused(["--cohort", "--cohort-edge-test", factors], "--cohort-edge-test", *words)
    # the cap, named by line and column: 32 labels; the same file is fine for --cohort-permanova
    names = [f"s{i}" for i in range(33)]
    (tmp_path / "wide.list").write_text("".join(f"{n}\ta.fasta\n" for n in names))
    (tmp_path / "factors.tsv").write_text("sample\tmany\n" + "".join(f"{n}\tv{i}\n" for i, n in enumerate(names)))
    base[4] = str(tmp_path / "wide.list")
    refused(["--cohort", "--cohort-edge-test", factors], "--cohort-edge-test", "line 34", "column many", "'v32'", "more than 32")
    refused(["--cohort", "--cohort-permanova", factors, "--cohort-edge-test", factors], "--cohort-edge-test", "line 34")
    # a good file passes on to the device and the database (there is none), beside PERMANOVA of the same file
    (tmp_path / "factors.tsv").write_text("sample\tmany\n" + "".join(f"{n}\tv{i % 32}\n" for i, n in enumerate(names)))
    run = subprocess.run(base + ["--cohort", "--cohort-edge-test", factors, "--cohort-edge-test-seed", "18446744073709551615",
                                 "--cohort-edge-test-permutations", "999999", "--cohort-permanova", factors], capture_output=True, text=True)
    assert run.returncode == 255 and "--cohort-edge-test" not in run.stderr and "factors.tsv" not in run.stderr, run.stderr
    assert "Cohort edge-test factors: 1 columns, 0 lines of samples that are not in the list skipped" in run.stdout
    assert "Cohort factors: 1 columns" in run.stdout


def test_launcher_passes_the_flags_only_when_given():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw)
    assert "edge-test" not in " ".join(default) and "edge-test" not in " ".join(epik.driver_command(**kw, cohort=True))
    assert epik.driver_command(**kw, cohort_edge_test=None, cohort_edge_test_permutations=None, cohort_edge_test_seed=None) == default
    assert epik.driver_command(**kw, cohort=True, cohort_edge_test="f.tsv")[:-1] == default[:-1] + ["--cohort", "--cohort-edge-test", "f.tsv"]
    assert epik.driver_command(**kw, cohort=True, cohort_alpha=True, cohort_permanova="f.tsv", cohort_edge_test="f.tsv",
                               cohort_edge_test_permutations=9999, cohort_edge_test_seed=(1 << 64) - 1, taxonomy="t.tsv",
                               strand="both")[:-1] == \
        default[:-1] + ["--strand", "both", "--cohort", "--cohort-alpha", "--cohort-permanova", "f.tsv", "--cohort-edge-test", "f.tsv",
                        "--cohort-edge-test-permutations", "9999", "--cohort-edge-test-seed", "18446744073709551615",
                        "--taxonomy", "t.tsv"]
    for bad in (dict(cohort_edge_test="f.tsv"), dict(cohort=True, cohort_edge_test_permutations=9), dict(cohort=True, cohort_edge_test_seed=9),
                dict(cohort=True, cohort_permanova="f.tsv", cohort_edge_test_seed=9)):
        with pytest.raises(click.UsageError):
            epik.driver_command(**kw, **bad)
    me = os.path.join(ROOT, "epik.py")
    out = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("--cohort-edge-test ", "--cohort-edge-test-permutations", "--cohort-edge-test-seed"):
        assert flag in out.stdout, flag
    for flags, word in ((["--cohort-edge-test", me], "--cohort"), (["--cohort", "--cohort-edge-test-seed", "3"], "--cohort-edge-test"),
                        (["--cohort", "--cohort-edge-test", me, "--cohort-edge-test-permutations", "0"], "999999"),
                        (["--cohort", "--cohort-edge-test", me, "--cohort-edge-test-permutations", "1000000"], "999999"),
                        (["--cohort", "--cohort-edge-test", me, "--cohort-edge-test-seed", "-1"], "18446744073709551615")):
        run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, *flags, me], capture_output=True, text=True)
        assert run.returncode == 2 and word in run.stderr, (flags, run.stdout, run.stderr)


# ---- 8. the host code stand-alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitized", [False, True])
def test_host_test_binary_edgetest_is_the_library_s(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    for num_branches, num_samples, permutations in ((7, 3, 1), (7, 5, 64), (999, 33, 9), (7, 65, 65)):
        parent, first = edge_tree(num_branches)
        rng = np.random.default_rng(900 + num_samples)
        mass = random_cells(rng, num_samples, num_branches, empty=1, bits=42)
        labels = factor_labels(rng, num_samples)
        _cells_input(tmp_path / "mass.bin", mass, first)
        (tmp_path / "labels.bin").write_bytes(labels.tobytes())
        run = subprocess.run([binary, "edgetest", str(tmp_path / "out.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "labels.bin"),
                              str(permutations), "12345678901234567890"], capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (num_samples, run.stderr)
        want = cohort_mod.edgetest_host(mass, first, labels, permutations, 12345678901234567890)
        assert (tmp_path / "out.bin").read_bytes() == want.records.tobytes() + want.stat.tobytes() + want.max.tobytes(), num_samples
    bad = labels.copy()
    bad[1, 0] = 32
    (tmp_path / "labels.bin").write_bytes(bad.tobytes())
    run = subprocess.run([binary, "edgetest", str(tmp_path / "o.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "labels.bin"), "9", "1"],
                         capture_output=True, text=True)
    assert run.returncode == 1 and "sample 1" in run.stderr and "32" in run.stderr
    (tmp_path / "labels.bin").write_bytes(b"\0" * 6)
    run = subprocess.run([binary, "edgetest", str(tmp_path / "o.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "labels.bin"), "9", "1"],
                         capture_output=True, text=True)
    assert run.returncode == 1 and "uint32 [S][M]" in run.stderr
    # the factor file through the stand-alone reader: an error names its line
    (tmp_path / "names.txt").write_text("".join(f"n{i}\n" for i in range(mass.shape[0])))
    (tmp_path / "factors.tsv").write_text("sample\tstate\n" + "".join(f"n{i}\tx\n" for i in range(mass.shape[0])) + "n3\ty\n")
    run = subprocess.run([binary, "edgetest-tsv", str(tmp_path / "o.tsv"), str(tmp_path / "mass.bin"), str(tmp_path / "names.txt"),
                          str(tmp_path / "factors.tsv"), "9", "1"], capture_output=True, text=True)
    assert run.returncode == 1 and f"line {mass.shape[0] + 2}" in run.stderr and "'n3'" in run.stderr and "twice" in run.stderr
    assert "--cohort-edge-test" in run.stderr
