"""PERMDISP of a cohort's samples over their KR distances, no device: the rule of include/epik_amd.h restated here in numpy
(the labellings are test_permanova_cpu's) against epik_amd_cohort_permdisp_host and _permdisp_kr_host bit for bit -- every
record, every stat[p], the group means and z --, the star and the plane by hand, the edge cases (a group of one, one group,
all singletons, residuals all zero), a p-value counted by hand, PERMANOVA's labellings under the same seed, the file from
Python and from C++, the flags' refusals and the stand-alone host binary (plain and under ASan + UBSan).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod
from test_cohort_cpu import host_bins, numpy_kr, same_bits  # noqa: F401 (host_bins: a fixture)
from test_pcoa_cpu import STAR_KR, pcoa_cells, pcoa_tree, plane_points
from test_permanova_cpu import FILE_FACTORS, FILE_NAMES, _cells_input, cohort_input, numpy_labellings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
MISSING = capi.PERMDISP_MISSING
NA = float(np.uint64(capi.NA_BITS).view(np.float64))
DOUBLES = ("eta2", "f", "p")
SLOTS = 1 + capi.PERMDISP_PAIR_SLOTS


# ---- the rule restated ------------------------------------------------------------------------------------------------------
def numpy_column(kr, idx, lam, sizes):
    """(z, r, clip, mean) by position of a column: every chain in the rule's order, j ascending, then i, then g."""
    n = len(idx)
    sizes = np.asarray(sizes, dtype=np.float64)
    k = kr[np.ix_(idx, idx)].T                                                  # A2[i][j] is the square of KR[u_j][u_i]
    a2 = k * k
    t, every = np.zeros(n), np.zeros(n)
    for j in range(n):
        same = lam == lam[j]
        every = np.where(same, every + a2[:, j], every)
        t = np.where(same & (np.arange(n) < j), t + a2[:, j], t)
    w = np.zeros(len(sizes))
    for i in range(n):
        w[lam[i]] = w[lam[i]] + t[i]
    centre = (w / sizes) / sizes
    z2 = every / sizes[lam] - centre[lam] if n else np.zeros(0)
    z = np.where(z2 > 0.0, np.sqrt(np.where(z2 > 0.0, z2, 0.0)), 0.0)
    mean = np.zeros(len(sizes))
    for i in range(n):
        mean[lam[i]] = mean[lam[i]] + z[i]
    mean = mean / sizes
    return z, (z - mean[lam] if n else z), z2 < 0.0, mean


def numpy_sums(x, mu, sizes):
    """(sxx, A(mu) [Q]) of the edge-test rule for the vector x and the labellings mu[Q][n]."""
    acc = np.float64(0.0)
    for v in x:
        acc = acc + v
    d = x - acc / np.float64(len(x))
    sxx = np.float64(0.0)
    for v in d:
        sxx = sxx + v * v
    q = mu.shape[0]
    s = np.zeros((q, len(sizes)))
    for i in range(len(x)):
        s[np.arange(q), mu[:, i]] = s[np.arange(q), mu[:, i]] + d[i]
    among = np.zeros(q)
    for g in range(len(sizes)):
        among = among + (s[:, g] * s[:, g]) / np.float64(sizes[g])
    return sxx, among


def numpy_test(z, r, clip, pos, lam, sizes, permutations, seed):
    """One test of the rule: (record, stat [P + 1] or None)."""
    record = np.zeros((), dtype=capi.PERMDISP)
    for f in DOUBLES:
        record[f] = NA
    n, groups = len(pos), len(sizes)
    record["used"], record["groups"], record["clipped"] = n, groups, int(clip[pos].sum()) if n else 0
    if groups < 2 or n - groups < 1:
        return record, None
    sxx, among = numpy_sums(z[pos], lam[None, :], sizes)
    if not sxx > 0.0:
        return record, None
    record["eta2"] = among[0] / sxx
    ssw = sxx - among[0]
    if ssw > 0.0:
        record["f"] = (among[0] / float(groups - 1)) / (ssw / float(n - groups))
    stat = np.full(permutations + 1, record["eta2"])
    sxx_r, among_r = numpy_sums(r[pos], numpy_labellings(lam, seed, permutations), sizes)
    if sxx_r > 0.0:
        stat[1:] = (among_r / sxx_r)[1:]
        record["at_least"] = int((stat[1:] >= stat[0]).sum())
    else:
        record["at_least"] = permutations
    record["p"] = float(1 + int(record["at_least"])) / float(permutations + 1)
    return record, stat


def numpy_permdisp(kr, totals, labels, permutations, seed, pairwise):
    """`cohort_mod.Permdisp` by the rule."""
    labels = np.asarray(labels)
    s, m = labels.shape
    slots = SLOTS if pairwise else 1
    records = np.zeros((m, slots), dtype=capi.PERMDISP)
    for f in DOUBLES:
        records[f] = NA
    stat = np.full((m, slots, permutations + 1), NA)
    group_mean = np.full((m, capi.PERMDISP_MAX_GROUPS), NA)
    zs = np.full((m, s), NA)
    for c in range(m):
        idx, lam, number = [], [], {}
        for i in range(s):
            if int(totals[i]) == 0 or labels[i, c] == MISSING:
                continue
            idx.append(i)
            lam.append(number.setdefault(int(labels[i, c]), len(number)))
        idx, lam = np.array(idx, dtype=np.int64), np.array(lam, dtype=np.int64)
        sizes = [int((lam == g).sum()) for g in range(len(number))]
        z, r, clip, mean = numpy_column(kr, idx, lam, sizes)
        zs[c, idx], group_mean[c, :len(sizes)] = z, mean
        records[c, 0], values = numpy_test(z, r, clip, np.arange(len(idx)), lam, sizes, permutations, seed)
        if values is not None:
            stat[c, 0] = values
        if pairwise:
            for h in range(1, len(sizes)):
                for g in range(h):
                    keep = np.flatnonzero((lam == g) | (lam == h))
                    slot = cohort_mod.pair_slot(g, h)
                    records[c, slot], values = numpy_test(z, r, clip, keep, (lam[keep] == h).astype(np.int64), [sizes[g], sizes[h]],
                                                          permutations, seed)
                    if values is not None:
                        stat[c, slot] = values
    return cohort_mod.Permdisp(records, stat, group_mean, zs)


def same_permdisp(got, want, what=""):
    for f in ("used", "groups", "clipped", "pad", "at_least"):
        assert np.array_equal(got.records[f], want.records[f]), (what, f, np.argwhere(got.records[f] != want.records[f])[:8])
    for f in DOUBLES:
        assert same_bits(got.records[f], want.records[f]), (what, f, np.argwhere(got.records[f].view(U64) != want.records[f].view(U64))[:8])
    if want.stat is not None and got.stat is not None:
        assert same_bits(got.stat, want.stat), (what, "stat", np.argwhere(got.stat.view(U64) != want.stat.view(U64))[:8])
    assert same_bits(got.group_mean, want.group_mean), (what, "group_mean")
    assert same_bits(got.z, want.z), (what, "z", np.argwhere(got.z.view(U64) != want.z.view(U64))[:8])
    for v in (got.records["eta2"], got.records["f"], got.records["p"], got.stat, got.group_mean, got.z):
        if v is not None:                                                       # no arithmetic NaN: a NaN is the NA pattern
            assert (v.view(U64)[np.isnan(v)] == U64(capi.NA_BITS)).all(), what
    return True


def disp_labels(rng, num_samples, pairwise):
    """labels [S][M], every label below 32: 2 groups; 3 unbalanced groups with a fifth missing; 4 groups; up to 7 groups under
    scattered ids, some of one sample; and, without pairwise, every sample its own group up to 32 (undefined) and one group."""
    s = num_samples
    cols = [rng.integers(0, 2, size=s), np.where(rng.random(s) < 0.2, MISSING, rng.choice(3, size=s, p=[0.6, 0.3, 0.1])),
            rng.integers(0, 4, size=s), np.array([31, 20, 3, 7, 0, 30, 12])[np.minimum(rng.geometric(0.35, size=s) - 1, 6)]]
    if not pairwise:
        cols += [np.arange(s) % 32, np.full(s, 17)]
    return np.ascontiguousarray(np.array(cols, dtype=np.uint32).T)


RESTATED = {}


def restated(num_used, num_branches, permutations, pairwise):
    """(mass, first, bl, kr, totals, labels, seed, numpy_permdisp) of a case, computed once."""
    key = (num_used, num_branches, permutations, pairwise)
    if key not in RESTATED:
        first, bl = pcoa_tree(num_branches)
        mass = pcoa_cells(num_used, num_branches)
        rng = np.random.default_rng(77 + 13 * num_used + num_branches + permutations)
        labels = disp_labels(rng, mass.shape[0], pairwise)
        seed = int(rng.integers(0, 1 << 63)) * 2 + 1
        kr = numpy_kr(mass, first, bl)
        totals = mass.sum(axis=1, dtype=U64)
        RESTATED[key] = (mass, first, bl, kr, totals, labels, seed, numpy_permdisp(kr, totals, labels, permutations, seed, pairwise))
    return RESTATED[key]


@pytest.mark.parametrize("num_branches", [7, 999])
@pytest.mark.parametrize("num_used", [0, 1, 2, 3, 33, 64, 65])
def test_permdisp_host_equals_the_numpy_restatement_bit_for_bit(num_used, num_branches):
    defined = 0
    for permutations, pairwise in ((1, False), (64, True), (65, False)):
        mass, first, bl, kr, totals, labels, seed, want = restated(num_used, num_branches, permutations, pairwise)
        what = (num_used, num_branches, permutations, pairwise)
        same_permdisp(cohort_mod.permdisp_host(mass, first, bl, labels, permutations, seed, pairwise), want, what)
        same_permdisp(cohort_mod.permdisp_kr_host(kr, totals, labels, permutations, seed, pairwise), want, what)
        r = want.records
        assert (r["used"][:, 0] <= num_used).all() and r["used"][0, 0] == num_used
        assert same_bits(want.stat[:, :, 0], r["eta2"])                                   # slot 0 holds eta2
        if not pairwise:                                                        # all singletons (up to 32), and one group
            assert r["groups"][4, 0] == min(num_used, 32) and r["groups"][5, 0] == min(num_used, 1) and np.isnan(r["p"][5, 0])
            if num_used <= 32:
                assert np.isnan(r["p"][4, 0]) and not want.z[4][totals > 0].view(U64).any()   # a group of one: z is +0.0
        defined += int((~np.isnan(r["p"])).sum())
    if num_used >= 33:
        assert defined >= 12


# ---- the star and the plane, by hand ---------------------------------------------------------------------------------------
def test_the_star_clips_its_centre():
    """Four samples in one group: A2 is 4 between leaves and 1 to the centre.  W = 3 * 4 + 3 * 1 = 15, c = 15 / 16 = 0.9375;
    m_leaf = (4 + 4 + 1) / 4 = 2.25, z2_leaf = 1.3125; m_centre = 3 / 4, z2_centre = 0.75 - 0.9375 < 0: clipped, z = 0.  All
    exact in binary.  A second group of two samples at distance 3: W = 9, c = 9 / 4, m = 9 / 2, z2 = 2.25, z = 1.5."""
    kr = np.zeros((6, 6))
    kr[:4, :4] = STAR_KR
    kr[4, 5] = kr[5, 4] = 3.0
    kr[:4, 4:] = kr[4:, :4] = 7.0                                               # (between the groups: never read)
    labels = np.array([[0, 0, 0, 0, 1, 1]], dtype=np.uint32).T.copy()
    got = cohort_mod.permdisp_kr_host(kr, np.ones(6, U64), labels, 99, 1)
    leaf = np.sqrt(1.3125)
    assert same_bits(got.z[0], [leaf, leaf, leaf, 0.0, 1.5, 1.5])
    r = got.records[0, 0]
    assert r["clipped"] == 1 and r["used"] == 6 and r["groups"] == 2 and r["pad"] == 0
    assert same_bits(got.group_mean[0, :2], [((leaf + leaf) + leaf + 0.0) / 4.0, 1.5])
    assert (got.group_mean[0, 2:].view(U64) == U64(capi.NA_BITS)).all()
    assert not np.isnan(r["eta2"]) and 0.0 <= r["eta2"] <= 1.0 and not np.isnan(r["p"])
    same_permdisp(got, numpy_permdisp(kr, np.ones(6, U64), labels, 99, 1, False))
    # the four alone: one group, no test, but z, the mean and clipped are written
    alone = cohort_mod.permdisp_kr_host(STAR_KR, np.ones(4, U64), np.zeros((4, 1), np.uint32), 9, 1)
    assert same_bits(alone.z[0], [leaf, leaf, leaf, 0.0]) and alone.records["clipped"][0, 0] == 1
    assert np.isnan(alone.records["p"][0, 0]) and alone.records["at_least"][0, 0] == 0 and np.isnan(alone.stat).all()


# The largest |z - numpy's Euclidean distance to the group centroid| of the host mirror on the 12 points, measured on the CPU:
# 1.776e-15 (z is between 1 and 10 there: a few ulp); the largest relative deviation of eta2 and F from numpy's one-way ANOVA
# of the same z: 6.890e-16.  The tolerances are 16 times those, the margin for another numpy, as for the principal coordinates.
PLANE_Z_MEASURED = 1.78e-15
PLANE_Z_TOLERANCE = 16 * PLANE_Z_MEASURED
PLANE_ANOVA_MEASURED = 6.89e-16
PLANE_ANOVA_TOLERANCE = 16 * PLANE_ANOVA_MEASURED


def test_twelve_points_in_the_plane_are_as_far_from_their_centroid_as_euclid_says():
    xy = plane_points()
    dist = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(axis=2))
    labels = np.array([[0, 1, 2] * 4, [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1]], dtype=np.uint32).T.copy()
    got = cohort_mod.permdisp_kr_host(dist, np.ones(12, U64), labels, 199, 3, True)
    same_permdisp(got, numpy_permdisp(dist, np.ones(12, U64), labels, 199, 3, True))
    assert not got.records["clipped"].any()
    deviation = 0.0
    for c in range(2):
        for g in np.unique(labels[:, c]):
            members = labels[:, c] == g
            want = np.sqrt(((xy[members] - xy[members].mean(axis=0)) ** 2).sum(axis=1))
            deviation = max(deviation, float(np.abs(got.z[c][members] - want).max()))
    print(f"plane: z of the host mirror is within {deviation:.3e} of numpy's distance to the centroid")
    assert deviation <= PLANE_Z_TOLERANCE
    # eta2 and F of the observed distances are the one-way ANOVA of z, relative to numpy's own sums
    relative = 0.0
    for c in range(2):
        z, lab = got.z[c], labels[:, c]
        groups = np.unique(lab)
        among = sum(((z[lab == g].mean() - z.mean()) ** 2) * (lab == g).sum() for g in groups)
        within = sum(((z[lab == g] - z[lab == g].mean()) ** 2).sum() for g in groups)
        f = (among / (len(groups) - 1)) / (within / (12 - len(groups)))
        eta2 = among / (among + within)
        relative = max(relative, abs(got.records["f"][c, 0] - f) / f, abs(got.records["eta2"][c, 0] - eta2) / eta2)
    print(f"plane: eta2 and F of the host mirror are within {relative:.3e} of numpy's, relative")
    assert relative <= PLANE_ANOVA_TOLERANCE


# ---- the edge cases --------------------------------------------------------------------------------------------------------
def test_a_group_of_one_residuals_all_zero_and_undefined_columns():
    x = np.array([0.0, 2.0, 10.0, 14.0, 30.0])
    kr = np.abs(x[:, None] - x[None, :])
    totals = np.ones(5, U64)
    # groups {0, 2}, {10, 14} and {30}: z = 1 1 2 2 0 (exact), the means 1 2 0, the residuals all +0.0: nothing to permute
    labels = np.array([[0, 0, 1, 1, 2], [4, 4, 4, 4, 4], [0, 1, 2, 3, 5], [MISSING] * 5], dtype=np.uint32).T.copy()
    got = cohort_mod.permdisp_kr_host(kr, totals, labels, 50, 9, True)
    same_permdisp(got, numpy_permdisp(kr, totals, labels, 50, 9, True))
    assert same_bits(got.z[0], [1.0, 1.0, 2.0, 2.0, 0.0]) and same_bits(got.group_mean[0, :3], [1.0, 2.0, 0.0])
    r = got.records[0, 0]
    assert r["used"] == 5 and r["groups"] == 3 and r["at_least"] == 50 and same_bits(r["p"], 1.0) and np.isnan(r["f"])   # ssw = 0
    assert same_bits(r["eta2"], 1.0) and same_bits(got.stat[0, 0], np.full(51, 1.0))     # every permuted statistic is a tie
    pair = got.records[0, cohort_mod.pair_slot(0, 1)]
    assert pair["used"] == 4 and pair["groups"] == 2 and pair["at_least"] == 50 and same_bits(pair["p"], 1.0)
    lone = got.records[0, cohort_mod.pair_slot(0, 2)]                            # 2 + 1 samples: defined, z = 1 1 0
    assert lone["used"] == 3 and not np.isnan(lone["eta2"])
    # one group; all singletons; no label: NA records, used and groups written, z and the means all the same
    for c, (used, groups) in ((1, (5, 1)), (2, (5, 5)), (3, (0, 0))):
        r = got.records[c, 0]
        assert (r["used"], r["groups"], r["at_least"], r["clipped"]) == (used, groups, 0, 0)
        assert all(np.float64(r[f]).view(U64) == U64(capi.NA_BITS) for f in DOUBLES) and np.isnan(got.stat[c]).all()
    assert same_bits(got.z[2], np.zeros(5)) and same_bits(got.group_mean[2, :5], np.zeros(5)) and np.isnan(got.z[3]).all()
    assert not np.isnan(got.z[1]).any() and not np.isnan(got.group_mean[1, 0]) and np.isnan(got.group_mean[1, 1:]).all()
    assert (got.records["used"][:, cohort_mod.pair_slot(3, 4) + 1:] == 0).all()


def test_the_p_value_counted_by_hand_and_the_labellings_of_permanova():
    """Points 0 2 4 6 | 10 16 on a line, groups a a a a b b.  Group a: W = 4 + 16 + 36 + 4 + 16 + 4 = 80, c = 80 / 16 = 5,
    m = 14 6 6 14, z = 3 1 1 3; group b: W = 36, c = 9, m = 18, z = 3 3.  Means 2 and 3, residuals 1 -1 -1 1 0 0: all exact.
    The count is made here from the restated labellings, which are PERMANOVA's for the same seed."""
    x = np.array([0.0, 2.0, 4.0, 6.0, 10.0, 16.0])
    kr = np.abs(x[:, None] - x[None, :])
    labels = np.array([[0, 0, 0, 0, 1, 1]], dtype=np.uint32).T.copy()
    permutations, seed = 40, 5
    totals = np.ones(6, U64)
    got = cohort_mod.permdisp_kr_host(kr, totals, labels, permutations, seed)
    assert same_bits(got.z[0], [3.0, 1.0, 1.0, 3.0, 3.0, 3.0]) and same_bits(got.group_mean[0, :2], [2.0, 3.0])
    # observed: mx = 14 / 6; the residuals have mean 0, so d = r and sxx_r = 4; S_a = sum of r over a, S_b likewise
    r = np.array([1.0, -1.0, -1.0, 1.0, 0.0, 0.0])
    lam = labels[:, 0].astype(np.int64)
    labellings = numpy_labellings(lam, seed, permutations)
    etas = np.array([(r[mu == 0].sum() ** 2 / 4.0 + r[mu == 1].sum() ** 2 / 2.0) / 4.0 for mu in labellings])   # (exact: small integers)
    assert same_bits(got.stat[0, 0, 1:], etas[1:])
    count = int((etas[1:] >= got.records["eta2"][0, 0]).sum())
    assert got.records["at_least"][0, 0] == count and same_bits(got.records["p"][0, 0], (1 + count) / 41.0) and 0 < count < 40
    # the same seed sees PERMANOVA's labellings: the same mu^p explains the SSW of permutation p there
    anova = cohort_mod.permanova_kr_host(kr, totals, labels, permutations, seed)
    a2 = kr * kr
    for p in (1, 2, 17, 40):
        mu = labellings[p]
        ssw = sum(a2[np.ix_(mu == g, mu == g)].sum() / 2.0 / (mu == g).sum() for g in (0, 1))   # (exact: small integers over 4 and 2)
        assert same_bits(anova.ssw[0, 0, p], ssw), p
    other = cohort_mod.permdisp_kr_host(kr, totals, labels, permutations, seed + 1)
    assert not same_bits(other.stat[0, 0, 1:], got.stat[0, 0, 1:])


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_permdisp_symbols_exist_and_refuse_what_the_header_says():
    lib = capi.load()
    for name in ("epik_amd_cohort_permdisp_device", "epik_amd_cohort_permdisp", "epik_amd_cohort_permdisp_host",
                 "epik_amd_cohort_permdisp_kr_host"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert capi.ABI_VERSION == 3 and capi.PERMDISP.itemsize == 48
    assert [capi.PERMDISP.fields[k][1] for k in capi.PERMDISP.names] == [0, 4, 8, 12, 16, 24, 32, 40]
    err = lambda: lib.epik_amd_last_error().decode()
    labels = np.zeros((4, 1), np.uint32)
    out, mean, z = np.zeros(497, dtype=capi.PERMDISP), np.zeros(32), np.zeros(4)
    ptr = lambda x: x.ctypes.data if x is not None else None
    assert lib.epik_amd_cohort_permdisp_device(None, None, ptr(labels), 1, 9, 1, 0, None, None, None, None, None) == capi.ERR_INVALID
    assert "null cohort" in err()
    assert lib.epik_amd_cohort_permdisp(None, None, None, ptr(labels), 1, 9, 1, 0, ptr(out), None, ptr(mean), ptr(z)) == capi.ERR_INVALID
    assert "null cohort" in err()
    first = cohort_mod.first_of([2, 2, -1])
    cells, bl = np.ones((4, 3), U64), np.ones(3)
    args = lambda m=cells, s=4, n=3, f=first, b=bl, l=labels, c=1, p=9, seed=1, pw=0, o=out, g=mean, zz=z: \
        (ptr(m), s, n, ptr(f), ptr(b), ptr(l), c, p, seed, pw, ptr(o), None, ptr(g), ptr(zz))
    host = lib.epik_amd_cohort_permdisp_host
    assert host(*args()) == capi.OK and host(*args(pw=1)) == capi.OK and host(*args(seed=(1 << 64) - 1)) == capi.OK
    assert host(*args(s=0)) == capi.ERR_INVALID and "num_samples is 0" in err()
    assert host(*args(n=0)) == capi.ERR_INVALID and "at least one branch" in err()
    for missing in ("m", "f", "b", "l", "o", "g", "zz"):
        assert host(*args(**{missing: None})) == capi.ERR_INVALID and "null argument" in err(), missing
    for bad in (0, 65, 0xFFFFFFFF):
        assert host(*args(c=bad)) == capi.ERR_INVALID and "num_columns" in err() and "[1, 64]" in err()
    for bad in (0, 1_000_000, 0xFFFFFFFF):
        assert host(*args(p=bad)) == capi.ERR_INVALID and "num_permutations" in err() and "[1, 999999]" in err()
    for bad in (32, 0xFFFFFFFE):
        wrong = labels.copy()
        wrong[2, 0] = bad
        assert host(*args(l=wrong)) == capi.ERR_INVALID and "sample 2" in err() and "column 0" in err() and "32" in err()
    kr, totals = np.zeros((4, 4)), np.ones(4, U64)
    kr_host = lib.epik_amd_cohort_permdisp_kr_host
    assert kr_host(ptr(kr), ptr(totals), 4, ptr(labels), 1, 9, 1, 0, ptr(out), None, ptr(mean), ptr(z)) == capi.OK
    assert kr_host(None, ptr(totals), 4, ptr(labels), 1, 9, 1, 0, ptr(out), None, ptr(mean), ptr(z)) == capi.ERR_INVALID
    assert "null argument" in err()
    assert kr_host(ptr(kr), ptr(totals), 0, ptr(labels), 1, 9, 1, 0, ptr(out), None, ptr(mean), ptr(z)) == capi.ERR_INVALID
    with pytest.raises(ValueError):
        cohort_mod.permdisp_host(cells, first, bl, np.zeros((3, 1), np.uint32))
    with pytest.raises(capi.EpikAmdError):
        cohort_mod.permdisp_host(cells, first, bl, labels, permutations=0)


# ---- the output file -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairwise", [False, True])
def test_the_python_and_the_c_formatters_agree(host_bins, tmp_path, pairwise):
    mass, first, bl, _ = cohort_input("tree15", 9, seed=8)
    mass[2] = mass[4] // U64(2) + U64(1)                                       # (cohort_input leaves sample 2 empty)
    mass[3] = 0
    (tmp_path / "factors.tsv").write_text(FILE_FACTORS)
    columns, labels, label_names, skipped = cohort_mod.read_factors(str(tmp_path / "factors.tsv"), FILE_NAMES, most=32)
    assert skipped == 1 and columns == ["state", "site", "lone"]
    result = cohort_mod.permdisp_host(mass, first, bl, labels, 99, 7, pairwise, with_stat=False)
    totals = cohort_mod.totals_of(mass)
    text = cohort_mod.format_permdisp_tsv(FILE_NAMES, totals, columns, label_names, labels, 99, 7, pairwise, result.records,
                                          result.group_mean, result.z)
    lines = text.split("\n")
    r = result.records
    assert lines[:5] == [f"# epik_amd permdisp v1  samples=9 used=8 columns=3 permutations=99 seed=7 pairwise={int(pairwise)}",
                         "# unused\tnone", "# column\t0\tstate\t8\t2", "# column\t1\tsite\t7\t3", "# column\t2\tlone\t8\t1"]
    assert lines[5] == "# group\t0\t0\thealthy\t4\t%.17g" % result.group_mean[0, 0] and lines[6].startswith("# group\t0\t1\tsick\t4\t")
    assert lines[10] == "# group\t2\t0\tx\t8\t%.17g" % result.group_mean[2, 0] and lines[11] == cohort_mod.PERMDISP_HEADER
    assert lines[12] == "state\t*\t*\t8\t2\t%d\t%.17g\t%.17g\t%d\t%.17g" % (r["clipped"][0, 0], r["eta2"][0, 0], r["f"][0, 0],
                                                                        r["at_least"][0, 0], r["p"][0, 0])
    at = lines.index("# distances")
    assert at == (19 if pairwise else 15) and lines[at - 1] == "lone\t*\t*\t8\t1\t%d\tNA\tNA\t0\tNA" % r["clipped"][2, 0]
    assert lines[at + 1] == "column\tname\tlabel\tdistance" and lines[at + 2] == "state\ta\thealthy\t%.17g" % result.z[0, 0]
    assert len(lines) == at + 2 + 8 + 7 + 8 + 1 and lines[-2] == "lone\tt\tx\t%.17g" % result.z[2, 8]
    _cells_input(tmp_path / "mass.bin", mass, first, bl)
    (tmp_path / "names.txt").write_text("".join(name + "\n" for name in FILE_NAMES))
    run = subprocess.run([os.path.join(host_bins, "cohort_test"), "permdisp-tsv", str(tmp_path / "cpp.tsv"), str(tmp_path / "mass.bin"),
                          str(tmp_path / "names.txt"), str(tmp_path / "factors.tsv"), "99", "7", str(int(pairwise))],
                         capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr
    assert (tmp_path / "cpp.tsv").read_bytes() == text.encode()
    with pytest.raises(ValueError):
        cohort_mod.format_permdisp_tsv(FILE_NAMES, totals, columns, label_names, labels, 99, 7, not pairwise, result.records,
                                       result.group_mean, result.z)


# ---- the launcher and the drivers ------------------------------------------------------------------------------------------
DEPENDENTS = (["--cohort-permdisp-permutations", "99"], ["--cohort-permdisp-seed", "5"], ["--cohort-permdisp-pairwise"])


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

    refused(["--cohort-permdisp", "f.tsv"], "--cohort-permdisp", "--cohort ")
    for dependent in DEPENDENTS:
        refused(dependent, dependent[0], "needs --cohort-permdisp")
        refused(["--cohort"] + dependent, dependent[0], "needs --cohort-permdisp")
        refused(["--cohort", "--cohort-permanova", "f.tsv"] + dependent, dependent[0], "needs --cohort-permdisp")
    shown = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert shown.returncode == 0 and "cohort_permdisp_<list>.tsv" in shown.stdout
    for flag in ("--cohort-permdisp arg", "--cohort-permdisp-permutations arg", "--cohort-permdisp-seed arg", "--cohort-permdisp-pairwise "):
        assert flag in shown.stdout, flag
    for name in "abc":
        (tmp_path / f"{name}.fasta").write_text(">r\nACGT\n")
    (tmp_path / "samples.list").write_text("a\ta.fasta\nb\tb.fasta\nc\tc.fasta\n")
    base[4] = str(tmp_path / "samples.list")
    factors = str(tmp_path / "factors.tsv")
    (tmp_path / "factors.tsv").write_text("sample\tstate\na\tx\nb\ty\nc\tx\n")
    for value in ("0", "1000000", "many", "12x"):
        refused(["--cohort", "--cohort-permdisp", factors, "--cohort-permdisp-permutations", value], "--cohort-permdisp-permutations",
                "[1, 999999]")
    for value in ("18446744073709551616", "seed", "7x"):
        refused(["--cohort", "--cohort-permdisp", factors, "--cohort-permdisp-seed", value], "--cohort-permdisp-seed", "uint64")
    (tmp_path / "factors.tsv").write_text("sample\tstate\tsite\na\tx\ty\nb\tx\nc\tx\ty\n")
    refused(["--cohort", "--cohort-permdisp", factors], "--cohort-permdisp", "line 3", "2 fields, not 3")
    names = [f"s{i}" for i in range(33)]                                        # the cap of 32 labels, pairwise or not
    (tmp_path / "wide.list").write_text("".join(f"{n}\ta.fasta\n" for n in names))
    (tmp_path / "factors.tsv").write_text("sample\tmany\n" + "".join(f"{n}\tv{i}\n" for i, n in enumerate(names)))
    base[4] = str(tmp_path / "wide.list")
    refused(["--cohort", "--cohort-permdisp", factors], "--cohort-permdisp", "line 34", "column many", "'v32'", "more than 32")
    # a good file, the same one for all three tests, passes on to the device and the database (there is none)
    (tmp_path / "factors.tsv").write_text("sample\tmany\n" + "".join(f"{n}\tv{i % 3}\n" for i, n in enumerate(names)))
    run = subprocess.run(base + ["--cohort", "--cohort-permdisp", factors, "--cohort-permanova", factors, "--cohort-edge-test", factors,
                                 "--cohort-pcoa", "--cohort-permdisp-seed", "18446744073709551615", "--cohort-permdisp-pairwise"],
                         capture_output=True, text=True)
    assert run.returncode == 255 and "--cohort-permdisp" not in run.stderr and "factors.tsv" not in run.stderr, run.stderr
    assert "Cohort PERMDISP factors: 1 columns, 0 lines of samples that are not in the list skipped" in run.stdout


def test_launcher_passes_the_flags_only_when_given():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw)
    assert "permdisp" not in " ".join(default) and "permdisp" not in " ".join(epik.driver_command(**kw, cohort=True))
    assert epik.driver_command(**kw, cohort_permdisp=None, cohort_permdisp_permutations=None, cohort_permdisp_seed=None,
                               cohort_permdisp_pairwise=False) == default
    assert epik.driver_command(**kw, cohort=True, cohort_permdisp="f.tsv")[:-1] == default[:-1] + ["--cohort", "--cohort-permdisp", "f.tsv"]
    assert epik.driver_command(**kw, cohort=True, cohort_permanova="f.tsv", cohort_permdisp="f.tsv", cohort_permdisp_permutations=9999,
                               cohort_permdisp_seed=(1 << 64) - 1, cohort_permdisp_pairwise=True, cohort_pcoa=True, taxonomy="t.tsv",
                               strand="both")[:-1] == \
        default[:-1] + ["--strand", "both", "--cohort", "--cohort-permanova", "f.tsv", "--cohort-permdisp", "f.tsv",
                        "--cohort-permdisp-permutations", "9999", "--cohort-permdisp-seed", "18446744073709551615",
                        "--cohort-permdisp-pairwise", "--cohort-pcoa", "--taxonomy", "t.tsv"]
    for bad in (dict(cohort_permdisp="f.tsv"), dict(cohort=True, cohort_permdisp_permutations=9), dict(cohort=True, cohort_permdisp_seed=9),
                dict(cohort=True, cohort_permdisp_pairwise=True), dict(cohort=True, cohort_permanova="f.tsv", cohort_permdisp_pairwise=True)):
        with pytest.raises(click.UsageError):
            epik.driver_command(**kw, **bad)
    me = os.path.join(ROOT, "epik.py")
    out = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("--cohort-permdisp ", "--cohort-permdisp-permutations", "--cohort-permdisp-seed", "--cohort-permdisp-pairwise"):
        assert flag in out.stdout, flag
    for flags, word in ((["--cohort-permdisp", me], "--cohort"), (["--cohort", "--cohort-permdisp-pairwise"], "--cohort-permdisp"),
                        (["--cohort", "--cohort-permdisp", me, "--cohort-permdisp-permutations", "0"], "999999")):
        run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, *flags, me], capture_output=True, text=True)
        assert run.returncode == 2 and word in run.stderr, (flags, run.stdout, run.stderr)


# ---- the host code stand-alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitized", [False, True])
def test_host_test_binary_permdisp_is_the_library_s(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    for num_samples, permutations, pairwise in ((2, 1, True), (5, 64, True), (33, 65, False), (65, 20, True)):
        mass, first, bl, rng = cohort_input("tree15", num_samples, seed=9)
        labels = disp_labels(rng, num_samples, pairwise)
        _cells_input(tmp_path / "mass.bin", mass, first, bl)
        (tmp_path / "labels.bin").write_bytes(labels.tobytes())
        run = subprocess.run([binary, "permdisp", str(tmp_path / "out.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "labels.bin"),
                              str(permutations), "12345678901234567890", str(int(pairwise))], capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (num_samples, run.stderr)
        want = cohort_mod.permdisp_host(mass, first, bl, labels, permutations, 12345678901234567890, pairwise)
        assert (tmp_path / "out.bin").read_bytes() == \
            want.records.tobytes() + want.stat.tobytes() + want.group_mean.tobytes() + want.z.tobytes(), num_samples
    bad = labels.copy()
    bad[1, 0] = 32
    (tmp_path / "labels.bin").write_bytes(bad.tobytes())
    run = subprocess.run([binary, "permdisp", str(tmp_path / "o.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "labels.bin"), "9", "1", "0"],
                         capture_output=True, text=True)
    assert run.returncode == 1 and "sample 1" in run.stderr and "32" in run.stderr
    (tmp_path / "names.txt").write_text("".join(f"n{i}\n" for i in range(mass.shape[0])))
    (tmp_path / "factors.tsv").write_text("sample\tstate\n" + "".join(f"n{i}\t{'xy'[i % 2]}\n" for i in range(mass.shape[0])))
    run = subprocess.run([binary, "permdisp-tsv", str(tmp_path / "o.tsv"), str(tmp_path / "mass.bin"), str(tmp_path / "names.txt"),
                          str(tmp_path / "factors.tsv"), "9", "1", "1"], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr and (tmp_path / "o.tsv").read_text().startswith("# epik_amd permdisp v1  samples=65")
