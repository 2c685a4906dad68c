"""PERMANOVA of a cohort's samples over their KR distances on the host (epik_amd/host/cohort.cpp: permanova_records), without
a GPU: a case derived by hand; the rule restated in numpy (keys in uint64 arithmetic, a stable argsort for the ranks, chains in
Python's order) against the host mirror bit for bit, every SSW of every permutation and every field; the generator; the
factor file's reader; the output file from Python and from C++; the flags' refusals; the stand-alone host binary.
"""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod
from test_cohort_cpu import host_bins, numpy_first, numpy_kr, random_cells, same_bits, tree_case  # noqa: F401 (host_bins: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
MISSING = capi.PERMANOVA_MISSING
NA = float(np.uint64(capi.NA_BITS).view(np.float64))
DOUBLES = ("ss_total", "ss_within", "f", "r2", "p")


# ---- the rule restated ------------------------------------------------------------------------------------------------------
def numpy_keys(seed, permutations, n):
    """key_p(i) for p = 0 .. P (row 0 is not used by the rule) and i < n: uint64 arithmetic that wraps."""
    with np.errstate(over="ignore"):
        counter = (np.arange(permutations + 1, dtype=U64)[:, None] << U64(32)) | np.arange(n, dtype=U64)[None, :]
        z = U64(seed) + counter * U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def numpy_labellings(lam, seed, permutations):
    """mu^p for p = 0 .. P, [P + 1][n]: a stable argsort of the keys is the order of (key, position); the position at slot r
    has rank r and takes lambda_r."""
    lam = np.asarray(lam)
    order = np.argsort(numpy_keys(seed, permutations, len(lam)), axis=1, kind="stable")
    mu = np.empty((permutations + 1, len(lam)), dtype=np.int64)
    np.put_along_axis(mu, order, np.broadcast_to(lam, mu.shape), axis=1)
    mu[0] = lam
    return mu


def numpy_ssw(A, mu, sizes):
    """SSW of every labelling mu[Q][n] over the block A[n][n]: (ssw [Q], W_g / n_g [Q][G]).  The labellings side by side;
    every chain in the rule's order: j ascending, then i ascending, then g ascending."""
    mu = np.asarray(mu)
    q, n = mu.shape
    t = np.zeros((q, n))
    for j in range(n):
        rows = np.arange(n) < j                                             # t_i takes A[i][j] for j > i ...
        same = (mu == mu[:, j:j + 1]) & rows[None, :]                       # ... where mu_j == mu_i
        t = np.where(same, t + A[:, j][None, :], t)
    w = np.zeros((q, len(sizes)))
    for i in range(n):
        w[np.arange(q), mu[:, i]] = w[np.arange(q), mu[:, i]] + t[:, i]
    terms = w / np.asarray(sizes, dtype=np.float64)[None, :]
    ssw = np.zeros(q)
    for g in range(len(sizes)):
        ssw = ssw + terms[:, g]
    return ssw, terms


def numpy_test(kr, idx, lam, sizes, permutations, seed):
    """One test of the rule: (record, ssw [P + 1] or None, W_g / n_g or None)."""
    record = np.zeros((), dtype=capi.PERMANOVA)
    for f in DOUBLES:
        record[f] = NA
    n, groups = len(idx), len(sizes)
    record["used"], record["groups"] = n, groups
    if groups < 2 or n - groups < 1:
        return record, None, None
    d = kr[np.ix_(idx, idx)]
    A = d * d
    total = numpy_ssw(A, np.zeros((1, n), dtype=np.int64), [1])[0][0] / float(n)
    ssw, terms = numpy_ssw(A, numpy_labellings(lam, seed, permutations), sizes)
    among = total - ssw[0]
    record["ss_total"], record["ss_within"] = total, ssw[0]
    if total != 0.0:
        record["r2"] = among / total
        if ssw[0] != 0.0:
            record["f"] = (among / float(groups - 1)) / (ssw[0] / float(n - groups))
    record["at_most"] = int((ssw[1:] <= ssw[0]).sum())
    record["p"] = float(1 + int(record["at_most"])) / float(permutations + 1)
    return record, ssw, terms[0]


def numpy_permanova(kr, totals, labels, permutations, seed, pairwise):
    """`cohort_mod.Permanova` by the rule."""
    labels = np.asarray(labels)
    s, m = labels.shape
    slots = 1 + (capi.PERMANOVA_PAIR_SLOTS if pairwise else 0)
    records = np.zeros((m, slots), dtype=capi.PERMANOVA)
    for f in DOUBLES:
        records[f] = NA
    ssw = np.full((m, slots, permutations + 1), NA)
    group_ss = np.full((m, capi.PERMANOVA_MAX_GROUPS), NA)
    for c in range(m):
        idx, lam, number = [], [], {}
        for i in range(s):
            if int(totals[i]) == 0 or labels[i, c] == MISSING:
                continue
            idx.append(i)
            lam.append(number.setdefault(int(labels[i, c]), len(number)))
        idx, lam = np.array(idx, dtype=np.int64), np.array(lam, dtype=np.int64)
        sizes = [int((lam == g).sum()) for g in range(len(number))]
        records[c, 0], values, terms = numpy_test(kr, idx, lam, sizes, permutations, seed)
        if values is not None:
            ssw[c, 0], group_ss[c, :len(sizes)] = values, terms
        if pairwise:
            for h in range(1, len(sizes)):
                for g in range(h):
                    keep = (lam == g) | (lam == h)
                    slot = 1 + h * (h - 1) // 2 + g
                    records[c, slot], values, _ = numpy_test(kr, idx[keep], (lam[keep] == h).astype(np.int64), [sizes[g], sizes[h]],
                                                             permutations, seed)
                    if values is not None:
                        ssw[c, slot] = values
    return cohort_mod.Permanova(records, ssw, group_ss)


def same_permanova(got, want, what=""):
    for f in ("used", "groups", "at_most"):
        assert np.array_equal(got.records[f], want.records[f]), (what, f, np.argwhere(got.records[f] != want.records[f])[:8])
    for f in DOUBLES:
        assert same_bits(got.records[f], want.records[f]), (what, f, np.argwhere(got.records[f].view(U64) != want.records[f].view(U64))[:8])
    if want.ssw is not None and got.ssw is not None:
        assert same_bits(got.ssw, want.ssw), (what, "ssw", np.argwhere(got.ssw.view(U64) != want.ssw.view(U64))[:8])
    assert same_bits(got.group_ss, want.group_ss), (what, "group_ss")
    only_na_or_numbers(got)
    return True


def only_na_or_numbers(result):
    """No arithmetic NaN reaches an output: a NaN is the NA pattern."""
    for f in DOUBLES:
        v = result.records[f]
        assert (v.view(U64)[np.isnan(v)] == U64(capi.NA_BITS)).all(), f
    for v in (result.ssw, result.group_ss):
        if v is not None:
            assert (v.view(U64)[np.isnan(v)] == U64(capi.NA_BITS)).all()


def factor_columns(rng, mass, pairwise):
    """labels [S][M]: two balanced groups; three unbalanced ones with a fifth missing; one group (undefined); every sample
    its own group (undefined; left out with pairwise beyond 32 samples); no label at all; up to seven groups, some of one
    sample, under ids that are not 0 .. G - 1; and two groups whose ids come in descending order."""
    s = mass.shape[0]
    cols = [np.arange(s) % 2, rng.choice(3, size=s, p=[0.6, 0.3, 0.1]), np.full(s, 5)]
    cols[1] = np.where(rng.random(s) < 0.2, MISSING, cols[1])
    if not pairwise or s <= capi.PERMANOVA_MAX_PAIR_GROUPS:
        cols.append(np.arange(s)[::-1] % 256 if s <= 256 else np.arange(s) % 256)
    cols.append(np.full(s, MISSING))
    cols.append(np.array([255, 200, 3, 77, 0, 31, 128])[np.minimum(rng.geometric(0.35, size=s) - 1, 6)])
    cols.append(np.where(np.arange(s) < (s + 2) // 3, 9, 4))
    return np.ascontiguousarray(np.array(cols, dtype=np.uint32).T)


def cohort_input(tree_name, num_samples, seed=5):
    parent, bl = tree_case(tree_name)
    first = numpy_first(parent)
    rng = np.random.default_rng(seed * 1000 + num_samples)
    mass = random_cells(rng, num_samples, len(parent), empty=2, bits=42)
    return mass, first, bl, rng


# ---- 1. by hand -------------------------------------------------------------------------------------------------------------
def test_four_points_on_a_line_by_hand():
    """Points 0, 1, 10, 11 with labels a a b b.  The squared distances: 1, 100, 121, 81, 100, 1; their sum 404, over L = 4:
    ss_total = 101.  Within a: 1 / 2, within b: 1 / 2: ss_within = 1, ss_among = 100, f = (100 / 1) / (1 / 2) = 200,
    r2 = 100 / 101.  The two other ways to split 2 + 2: {0, 10}{1, 11}: 100 / 2 + 100 / 2 = 100; {0, 11}{1, 10}: 121 / 2 + 81 / 2
    = 101."""
    x = np.array([0.0, 1.0, 10.0, 11.0])
    kr = np.abs(x[:, None] - x[None, :])
    labels = np.array([[0, 0, 1, 1], [7, 3, 7, 3], [1, 0, 0, 1]], dtype=np.uint32).T.copy()
    got = cohort_mod.permanova_kr_host(kr, np.ones(4, U64), labels, permutations=200, seed=1)
    r = got.records[:, 0]
    assert list(r["used"]) == [4, 4, 4] and list(r["groups"]) == [2, 2, 2]
    assert same_bits(r["ss_total"], [101.0] * 3) and same_bits(r["ss_within"], [1.0, 100.0, 101.0])
    assert same_bits(r["f"][0], 200.0) and same_bits(r["r2"][0], 100.0 / 101.0)
    assert same_bits(r["f"][2], 0.0) and same_bits(r["r2"][2], 0.0)
    assert same_bits(got.group_ss[:, :2], [[0.5, 0.5], [50.0, 50.0], [60.5, 40.5]])
    assert set(np.unique(got.ssw[:, 0, :])) == {1.0, 100.0, 101.0}              # every permutation is one of the three splits
    assert same_bits(got.ssw[:, 0, 0], r["ss_within"])
    for c in range(3):
        assert r["at_most"][c] == (got.ssw[c, 0, 1:] <= got.ssw[c, 0, 0]).sum()
        assert same_bits(r["p"][c], (1 + int(r["at_most"][c])) / 201.0)
    assert r["at_most"][2] == 200 and r["p"][2] == 1.0 and 0 < r["at_most"][0] < 200
    same_permanova(got, numpy_permanova(kr, np.ones(4, U64), labels, 200, 1, False))
    # a sample without mass or without a label is not a position: the same test of the other four
    wide = np.full((6, 6), -1.0)
    wide[np.ix_([0, 2, 3, 5], [0, 2, 3, 5])] = kr
    more = np.array([[0, 1, 0, 1, MISSING, 1]], dtype=np.uint32).T.copy()
    again = cohort_mod.permanova_kr_host(wide, np.array([3, 0, 1, 1, 9, 2], U64), more, permutations=200, seed=1)
    assert again.records[0, 0] == got.records[0, 0] and same_bits(again.ssw[0, 0], got.ssw[0, 0])


# ---- 2. the host mirror against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("num_samples", [2, 4, 5, 33, 65, 130])
def test_host_equals_the_numpy_restatement_bit_for_bit(num_samples):
    mass, first, bl, rng = cohort_input("tree15", num_samples)
    if num_samples >= 5:
        mass[num_samples - 1] = mass[0]                                        # two samples at distance 0
    kr = numpy_kr(mass, first, bl)
    totals = cohort_mod.totals_of(mass)
    for permutations in (1, 64, 65, 200):
        for pairwise in (False, True):
            labels = factor_columns(rng, mass, pairwise)
            seed = int(rng.integers(0, 1 << 63)) * 2 + 1
            got = cohort_mod.permanova_host(mass, first, bl, labels, permutations, seed, pairwise)
            want = numpy_permanova(kr, totals, labels, permutations, seed, pairwise)
            same_permanova(got, want, (num_samples, permutations, pairwise))
            same_permanova(cohort_mod.permanova_kr_host(kr, totals, labels, permutations, seed, pairwise), want)
            r = got.records
            assert r["groups"][2, 0] == min(1, r["used"][2, 0]) and np.isnan(r["p"][2, 0]) and r["at_most"][2, 0] == 0   # G = 1
            none = labels.shape[1] - 3                                         # the column without a label
            assert r["used"][none, 0] == 0 and r["groups"][none, 0] == 0 and np.isnan(r["ss_total"][none, 0])
            if labels.shape[1] == 7:                                           # G = L
                assert r["groups"][3, 0] == r["used"][3, 0] == (totals != 0).sum() and np.isnan(r["f"][3, 0])
            if pairwise:
                # the slots: pair (g, h) at 1 + h (h - 1) / 2 + g; a slot without a pair has used = 0
                for c in range(labels.shape[1]):
                    groups = int(r["groups"][c, 0])
                    sizes = cohort_mod.groups_of(labels, totals)[c][1]
                    for h in range(1, 32):
                        for g in range(h):
                            slot = cohort_mod.pair_slot(g, h)
                            assert slot == 1 + h * (h - 1) // 2 + g
                            if h < groups:
                                assert r["used"][c, slot] == sizes[g] + sizes[h] and r["groups"][c, slot] == 2
                                assert np.isnan(r["p"][c, slot]) == (sizes[g] + sizes[h] < 3)
                            else:
                                assert r["used"][c, slot] == 0 and r["groups"][c, slot] == 0 and np.isnan(r["p"][c, slot])
    if num_samples >= 33:
        assert not np.isnan(got.records["f"][[0, 1, -2, -1], 0]).any()


def test_identical_samples_and_identical_groups():
    mass, first, bl, _ = cohort_input("tree15", 8)
    mass[:] = mass[0]
    labels = np.array([[0, 1] * 4], dtype=np.uint32).T.copy()
    got = cohort_mod.permanova_host(mass, first, bl, labels, 64, 3, True)
    r = got.records[0]
    for slot in (0, 1):                                                        # ss_total = 0: f and r2 undefined, p = 1
        assert same_bits(r["ss_total"][slot], 0.0) and same_bits(r["ss_within"][slot], 0.0) and r["at_most"][slot] == 64
        assert np.isnan(r["f"][slot]) and np.isnan(r["r2"][slot]) and same_bits(r["p"][slot], 1.0)
    same_permanova(got, numpy_permanova(numpy_kr(mass, first, bl), cohort_mod.totals_of(mass), labels, 64, 3, True))
    # two groups of the same two samples each: d^2 / 2 + d^2 / 2 within, (4 d^2) / 4 in all; the sum of four equal terms
    # rounds at 3 d^2 at the most, so ss_among is 0 within two roundings of ss_total
    mass, first, bl, _ = cohort_input("tree15", 4, seed=6)
    mass[2], mass[3] = mass[0], mass[1]
    labels = np.array([[0, 0, 1, 1]], dtype=np.uint32).T.copy()
    got = cohort_mod.permanova_host(mass, first, bl, labels, 65, 3)
    r = got.records[0, 0]
    assert r["ss_total"] > 0 and abs(r["ss_total"] - r["ss_within"]) <= 2 * np.spacing(r["ss_total"]) and r["p"] > 0.5
    same_permanova(got, numpy_permanova(numpy_kr(mass, first, bl), cohort_mod.totals_of(mass), labels, 65, 3, False))
    # within-group distances all 0: SSW_0 = 0, f undefined, r2 = 1
    labels = np.array([[0, 1, 0, 1]], dtype=np.uint32).T.copy()
    r = cohort_mod.permanova_host(mass, first, bl, labels, 65, 3).records[0, 0]
    assert same_bits(r["ss_within"], 0.0) and np.isnan(r["f"]) and same_bits(r["r2"], 1.0) and 0 < r["p"] < 1


# ---- 3. the generator -----------------------------------------------------------------------------------------------------------
def test_the_keys_rank_into_permutations_that_differ_by_p_and_by_seed():
    for n in (1, 2, 6, 65, 300):
        keys = numpy_keys(12345, 50, n)
        assert len(np.unique(keys)) == keys.size                               # no tie within or between permutations
        assert not np.array_equal(keys, numpy_keys(12346, 50, n))
        lam = np.arange(n)                                                     # mu_i = rank_p(i)
        mu = numpy_labellings(lam, 12345, 50)
        assert (np.sort(mu, axis=1) == lam[None, :]).all() and (mu[0] == lam).all()
        if n >= 65:                                                            # (6! = 720 orders may well repeat among 51)
            assert len({tuple(row) for row in mu}) == 51
        if n >= 6:
            assert not np.array_equal(mu[1:], numpy_labellings(lam, 99, 50)[1:])
        for p in (1, 50):                                                      # the rank is the count of smaller (key, position)
            counted = [sum((keys[p, j], j) < (keys[p, i], i) for j in range(n)) for i in range(n)]
            assert list(mu[p]) == counted
    # the counter: p in the high word, the position in the low one; seed 0 and counter 0 give the finaliser's fixed point 0,
    # counter 1 the first output of splitmix64 seeded with 0
    assert numpy_keys(0, 0, 2)[0, 0] == 0 and numpy_keys(0, 0, 2)[0, 1] == 0xE220A8397B1DCDAF
    assert numpy_keys(5, 3, 2)[3, 1] == numpy_keys(5 + ((3 << 32) | 1) * 0x9E3779B97F4A7C15 % (1 << 64), 0, 1)[0, 0]


def test_the_share_of_permutations_follows_the_exact_share_of_all_720_labellings():
    """L = 6, groups 3 + 3: q is the share of the 720 labellings lambda o sigma with SSW <= SSW_0.  at_most of P = 9 999
    permutations is a sum of P draws; were they independent and uniform its share would lie within 5 sqrt(q (1 - q) / P) of
    q but for one run in two million.  The seed is fixed: the check is deterministic."""
    mass, first, bl, _ = cohort_input("tree15", 6, seed=11)
    mass[mass.sum(axis=1) == 0] = 1
    labels = np.array([[0, 1, 1, 0, 1, 0]], dtype=np.uint32).T.copy()
    kr = numpy_kr(mass, first, bl)
    A = kr * kr
    lam = labels[:, 0].astype(np.int64)
    every = np.array([lam[list(sigma)] for sigma in itertools.permutations(range(6))])
    ssw, _ = numpy_ssw(A, np.vstack([lam[None, :], every]), [3, 3])
    q = float((ssw[1:] <= ssw[0]).mean())
    assert 0.0 < q < 1.0 and len(every) == 720
    permutations = 9999
    got = cohort_mod.permanova_host(mass, first, bl, labels, permutations, 1, with_ssw=False)
    share = int(got.records["at_most"][0, 0]) / permutations
    print("q", q, "share", share, "bound", 5 * np.sqrt(q * (1 - q) / permutations))
    assert abs(share - q) <= 5 * np.sqrt(q * (1 - q) / permutations)
    assert same_bits(got.records["p"][0, 0], (1 + int(got.records["at_most"][0, 0])) / 10000.0)


# ---- 4. the C ABI ---------------------------------------------------------------------------------------------------------------
def test_permanova_symbols_exist_and_refuse_what_the_header_says():
    lib = capi.load()
    for name in ("epik_amd_cohort_permanova_device", "epik_amd_cohort_permanova", "epik_amd_cohort_permanova_host",
                 "epik_amd_cohort_permanova_kr_host"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert capi.ABI_VERSION == 3 and capi.PERMANOVA.itemsize == 56
    assert [capi.PERMANOVA.fields[k][1] for k in capi.PERMANOVA.names] == [0, 4, 8, 16, 24, 32, 40, 48]
    assert capi.PERMANOVA_PAIR_SLOTS == 32 * 31 // 2 == cohort_mod.pair_slot(30, 31)
    err = lambda: lib.epik_amd_last_error().decode()
    labels = np.zeros((4, 1), np.uint32)
    out = np.zeros(497, dtype=capi.PERMANOVA)
    assert lib.epik_amd_cohort_permanova_device(None, None, labels.ctypes.data, 1, 9, 1, 0, None, None, None, None) == capi.ERR_INVALID
    assert "null cohort" in err()
    assert lib.epik_amd_cohort_permanova(None, None, None, labels.ctypes.data, 1, 9, 1, 0, out.ctypes.data, None, None) == capi.ERR_INVALID
    assert "null cohort" in err()
    first = cohort_mod.first_of([2, 2, -1])
    cells, bl = np.ones((4, 3), U64), np.ones(3)
    ptr = lambda x: x.ctypes.data if x is not None else None
    args = lambda m=cells, s=4, n=3, f=first, b=bl, l=labels, c=1, p=9, seed=1, pw=0, o=out: \
        (ptr(m), s, n, ptr(f), ptr(b), ptr(l), c, p, seed, pw, ptr(o), None, None)
    host = lib.epik_amd_cohort_permanova_host
    assert host(*args()) == capi.OK and host(*args(pw=1)) == capi.OK and host(*args(seed=(1 << 64) - 1)) == capi.OK
    assert host(*args(s=0)) == capi.ERR_INVALID and "num_samples is 0" in err()
    assert host(*args(n=0)) == capi.ERR_INVALID and "at least one branch" in err()
    for missing in ("m", "f", "b", "l", "o"):
        assert host(*args(**{missing: None})) == capi.ERR_INVALID and "null argument" in err(), missing
    assert host(*args(f=np.array([0, 2, 0], dtype=np.uint32))) == capi.ERR_INVALID and "branch 1" in err()
    for bad in (0, 65, 0xFFFFFFFF):
        assert host(*args(c=bad)) == capi.ERR_INVALID and "num_columns" in err() and "[1, 64]" in err()
    for bad in (0, 1_000_000, 0xFFFFFFFF):
        assert host(*args(p=bad)) == capi.ERR_INVALID and "num_permutations" in err() and "[1, 999999]" in err()
    for bad in (256, 0xFFFFFFFE):
        wrong = labels.copy()
        wrong[2, 0] = bad
        assert host(*args(l=wrong)) == capi.ERR_INVALID and "sample 2" in err() and "column 0" in err() and "256" in err()
    many, more_cells = np.arange(33, dtype=np.uint32)[:, None].copy(), np.ones((33, 3), U64)
    big = (ptr(more_cells), 33, 3, ptr(first), ptr(bl), ptr(many), 1, 9, 1)
    assert host(*big, 0, ptr(out), None, None) == capi.OK
    assert host(*big, 1, ptr(out), None, None) == capi.ERR_INVALID and "33 distinct labels" in err() and "32" in err()
    kr = np.zeros((4, 4))
    totals = np.ones(4, U64)
    kr_host = lib.epik_amd_cohort_permanova_kr_host
    assert kr_host(ptr(kr), ptr(totals), 4, ptr(labels), 1, 9, 1, 0, ptr(out), None, None) == capi.OK
    assert kr_host(None, ptr(totals), 4, ptr(labels), 1, 9, 1, 0, ptr(out), None, None) == capi.ERR_INVALID and "null argument" in err()
    assert kr_host(ptr(kr), ptr(totals), 0, ptr(labels), 1, 9, 1, 0, ptr(out), None, None) == capi.ERR_INVALID
    with pytest.raises(ValueError):
        cohort_mod.permanova_host(cells, first, bl, np.zeros((3, 1), np.uint32))
    with pytest.raises(capi.EpikAmdError):
        cohort_mod.permanova_host(cells, first, bl, np.zeros((4, 0), np.uint32))
    with pytest.raises(capi.EpikAmdError):
        cohort_mod.permanova_host(cells, first, bl, labels, permutations=0)


# ---- 5. the factor file ---------------------------------------------------------------------------------------------------------
GOOD_FACTORS = ("# a comment\n\nsample\tstate\tsite of body\n"
                "b\tsick\tgut\n"
                "stranger\tx\ty\n"
                "a\thealthy\tNA\n"
                "\n# another\n"
                "c\tsick\t\n"
                "d\tit's 7 %\tgut\n")


def test_the_factor_file(tmp_path):
    path = tmp_path / "factors.tsv"
    path.write_text(GOOD_FACTORS)
    names = ["a", "b", "c", "d"]
    columns, labels, label_names, skipped = cohort_mod.read_factors(str(path), names)
    assert columns == ["state", "site of body"] and skipped == 1 and labels.dtype == np.uint32
    assert label_names == [["sick", "healthy", "it's 7 %"], ["gut"]]            # numbered by first appearance in the file
    assert labels.tolist() == [[1, MISSING], [0, 0], [0, MISSING], [2, 0]]
    path.write_bytes(GOOD_FACTORS.replace("\n", "\r\n").encode())
    again = cohort_mod.read_factors(str(path), names)
    assert again[0] == columns and np.array_equal(again[1], labels) and again[2] == label_names and again[3] == 1
    head = "sample\tstate\tsite\n"
    many = "sample" + "".join(f"\tc{i}" for i in range(65)) + "\n"
    rows = "a\tx\ty\nb\tx\ty\nc\tx\ty\nd\tx\ty\n"
    for text, words in ((head + "a\tx\ty\nb\tx\nc\tx\ty\nd\tx\ty\n", ("line 3", "2 fields, not 3")),
                        (head + "a\tx\ty\nb\tx\ty\tz\nc\tx\ty\n", ("line 3", "4 fields, not 3")),
                        (head + "a\tx\ty\nb\tx\ty\n\na\tz\tw\nc\tx\ty\n", ("line 5", "'a'", "twice")),
                        (head + "a\tx\ty\nb\tx\ty\nc\tx\ty\n", ("no line", "'d'")),
                        ("name\tstate\n" + rows, ("line 1", "'sample'")),
                        ("sample\n", ("line 1", "0 columns")),
                        (many, ("line 1", "65 columns")),
                        ("sample\tstate\tstate\n", ("line 1", "'state'", "twice")),
                        ("sample\tstate\t\n", ("line 1", "column 2", "empty")),
                        ("# nothing\n\n", ("no header",))):
        path.write_text(text)
        with pytest.raises(ValueError) as e:
            cohort_mod.read_factors(str(path), names)
        assert all(w in str(e.value) for w in words), (text, str(e.value))
    # the caps: 256 distinct labels a column among the list's samples, 32 with pairwise; a stranger's label does not count
    for most, pairwise in ((256, False), (32, True)):
        wide = [f"s{i}" for i in range(most + 1)]
        text = "sample\tone\tmany\nstranger\tq\tanother\n" + "".join(f"s{i}\tk\tv{i}\n" for i in range(most + 1))
        path.write_text(text)
        with pytest.raises(ValueError) as e:
            cohort_mod.read_factors(str(path), wide, pairwise)
        assert all(w in str(e.value) for w in (f"line {most + 3}", "column many", f"'v{most}'", f"more than {most}")), str(e.value)
        columns, labels, label_names, skipped = cohort_mod.read_factors(str(path), wide[:most], pairwise)
        assert skipped == 2 and len(label_names[1]) == most and labels[:, 1].tolist() == list(range(most))
    assert len(cohort_mod.read_factors(str(path), wide)[2][1]) == 33            # without pairwise 33 labels are fine


# ---- 6. the output file -----------------------------------------------------------------------------------------------------------
def _cells_input(path, cells, first, bl):
    with open(path, "wb") as fh:
        fh.write(np.array(cells.shape, dtype="<u8").tobytes() + np.ascontiguousarray(cells, U64).tobytes() +
                 np.ascontiguousarray(first, np.uint32).tobytes() + np.ascontiguousarray(bl, np.float64).tobytes())


FILE_NAMES = ["a", "skin 3", "it's", "none", "z.9_-", "q", "r", "s", "t"]
FILE_FACTORS = ("sample\tstate\tsite\tlone\n"
                "q\tsick\tgut\tx\n" "a\thealthy\tskin\tx\n" "skin 3\tsick\tskin\tx\n" "it's\thealthy\tgut\tx\n" "none\tsick\tmouth\tx\n"
                "z.9_-\thealthy\tNA\tx\n" "r\tsick\tgut\tx\n" "s\thealthy\tmouth of 2\tx\n" "t\tsick\tgut\tx\n" "other\t1\t2\t3\n")


@pytest.mark.parametrize("pairwise", [False, True])
def test_the_file_reads_back_and_the_python_and_the_c_formatters_agree(host_bins, tmp_path, pairwise):
    mass, first, bl, _ = cohort_input("tree15", 9, seed=8)
    mass[2] = mass[4] // U64(2) + U64(1)                                       # (cohort_input leaves sample 2 empty)
    mass[3] = 0
    (tmp_path / "factors.tsv").write_text(FILE_FACTORS)
    columns, labels, label_names, skipped = cohort_mod.read_factors(str(tmp_path / "factors.tsv"), FILE_NAMES, pairwise)
    assert skipped == 1 and columns == ["state", "site", "lone"]
    result = cohort_mod.permanova_host(mass, first, bl, labels, 99, 7, pairwise, with_ssw=False)
    totals = cohort_mod.totals_of(mass)
    text = cohort_mod.format_permanova_tsv(FILE_NAMES, totals, columns, label_names, labels, 99, 7, pairwise, result.records,
                                           result.group_ss)
    lines = text.split("\n")
    r = result.records
    assert lines[:5] == [f"# epik_amd permanova v1  samples=9 used=8 columns=3 permutations=99 seed=7 pairwise={int(pairwise)}",
                         "# unused\tnone", "# column\t0\tstate\t8\t2", "# column\t1\tsite\t7\t3", "# column\t2\tlone\t8\t1"]
    # the groups in the rule's order (first appearance in the list, not in the file), with their sizes
    assert lines[5] == "# group\t0\t0\thealthy\t4\t%.17g" % result.group_ss[0, 0] and lines[6].startswith("# group\t0\t1\tsick\t4\t")
    assert [ln.split("\t")[3:5] for ln in lines[7:10]] == [["skin", "2"], ["gut", "4"], ["mouth of 2", "1"]]
    assert lines[10] == "# group\t2\t0\tx\t8\tNA" and lines[11] == cohort_mod.PERMANOVA_HEADER
    whole = "state\t*\t*\t8\t2\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%d\t%.17g" % (
        r["ss_total"][0, 0], r["ss_total"][0, 0] - r["ss_within"][0, 0], r["ss_within"][0, 0], r["f"][0, 0], r["r2"][0, 0],
        r["at_most"][0, 0], r["p"][0, 0])
    assert lines[12] == whole
    if pairwise:
        assert lines[13].startswith("state\thealthy\tsick\t8\t2\t") and lines[13].split("\t")[5:] == whole.split("\t")[5:]
        assert [ln.split("\t")[:5] for ln in lines[14:18]] == [["site", "*", "*", "7", "3"], ["site", "skin", "gut", "6", "2"],
                                                               ["site", "skin", "mouth of 2", "3", "2"],
                                                               ["site", "gut", "mouth of 2", "5", "2"]]
        assert lines[18] == "lone\t*\t*\t8\t1" + "\tNA" * 5 + "\t0\tNA" and len(lines) == 20
    else:
        assert lines[13].startswith("site\t*\t*\t7\t3\t") and lines[14] == "lone\t*\t*\t8\t1" + "\tNA" * 5 + "\t0\tNA" and len(lines) == 16
    path = tmp_path / "cohort_permanova_x.tsv"
    path.write_bytes(text.encode())
    back_columns, rows, groups, info = cohort_mod.read_permanova_tsv(str(path))
    assert back_columns == columns and info == {"samples": 9, "used": 8, "unused": ["none"], "permutations": 99, "seed": 7,
                                                "pairwise": pairwise, "column_used": [8, 7, 8], "column_groups": [2, 3, 1]}
    assert [(g[0], g[1], g[2], g[3]) for g in groups] == [(0, 0, "healthy", 4), (0, 1, "sick", 4), (1, 0, "skin", 2), (1, 1, "gut", 4),
                                                          (1, 2, "mouth of 2", 1), (2, 0, "x", 8)]
    assert same_bits([g[4] for g in groups[:5]], list(result.group_ss[0, :2]) + list(result.group_ss[1, :3]))
    assert rows[0][:3] == ("state", "*", "*") and rows[0][3] == r[0, 0] and same_bits(rows[0][4], r["ss_total"][0, 0] - r["ss_within"][0, 0])
    assert len(rows) == (7 if pairwise else 3) and np.isnan(rows[-1][4])
    if pairwise:
        assert rows[3][:3] == ("site", "skin", "gut") and rows[3][3].tobytes() == r[1, cohort_mod.pair_slot(0, 1)].tobytes()
    # the C++ reader and formatter over the C++ mirror: the same bytes
    _cells_input(tmp_path / "mass.bin", mass, first, bl)
    (tmp_path / "names.txt").write_text("".join(name + "\n" for name in FILE_NAMES))
    run = subprocess.run([os.path.join(host_bins, "cohort_test"), "permanova-tsv", str(tmp_path / "cpp.tsv"), str(tmp_path / "mass.bin"),
                          str(tmp_path / "names.txt"), str(tmp_path / "factors.tsv"), "99", "7", str(int(pairwise))],
                         capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr
    assert "3 columns, 1 lines of samples that are not in the list skipped" in run.stdout
    assert (tmp_path / "cpp.tsv").read_bytes() == text.encode()
    path.write_text("# something else\n")
    with pytest.raises(ValueError):
        cohort_mod.read_permanova_tsv(str(path))
    with pytest.raises(ValueError):
        cohort_mod.format_permanova_tsv(FILE_NAMES[:4], totals, columns, label_names, labels, 99, 7, pairwise, result.records, result.group_ss)
    with pytest.raises(ValueError):
        cohort_mod.format_permanova_tsv(FILE_NAMES, totals, columns, label_names, labels, 99, 7, not pairwise, result.records, result.group_ss)


# ---- 7. the launcher and the drivers ------------------------------------------------------------------------------------------
DEPENDENTS = (["--cohort-permanova-permutations", "99"], ["--cohort-permanova-seed", "5"], ["--cohort-permanova-pairwise"])


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

    refused(["--cohort-permanova", "f.tsv"], "--cohort-permanova", "--cohort ")
    refused(["--cohort-permanova", "f.tsv", "--cohort-permanova-pairwise", "--cohort-alpha"], "--cohort ")
    for dependent in DEPENDENTS:
        refused(dependent, dependent[0], "needs --cohort-permanova")
        refused(["--cohort"] + dependent, dependent[0], "needs --cohort-permanova")
    shown = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert shown.returncode == 0 and "cohort_permanova_<list>.tsv" in shown.stdout
    for flag in ("--cohort-permanova arg", "--cohort-permanova-permutations arg", "--cohort-permanova-seed arg", "--cohort-permanova-pairwise "):
        assert flag in shown.stdout, flag
    for name in "abc":
        (tmp_path / f"{name}.fasta").write_text(">r\nACGT\n")
    (tmp_path / "samples.list").write_text("a\ta.fasta\nb\tb.fasta\nc\tc.fasta\n")
    base[4] = str(tmp_path / "samples.list")
    factors = str(tmp_path / "factors.tsv")
    (tmp_path / "factors.tsv").write_text("sample\tstate\na\tx\nb\ty\nc\tx\n")
    for value in ("0", "1000000", "many", "12x"):
        refused(["--cohort", "--cohort-permanova", factors, "--cohort-permanova-permutations", value], "--cohort-permanova-permutations",
                "[1, 999999]")
    for value in ("18446744073709551616", "seed", "7x"):
        refused(["--cohort", "--cohort-permanova", factors, "--cohort-permanova-seed", value], "--cohort-permanova-seed", "uint64")
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
        refused(["--cohort", "--cohort-permanova", factors], "--cohort-permanova", *words)
    # the caps, named by line and column: 32 labels with pairwise
    names = [f"s{i}" for i in range(33)]
    (tmp_path / "wide.list").write_text("".join(f"{n}\ta.fasta\n" for n in names))
    (tmp_path / "factors.tsv").write_text("sample\tmany\n" + "".join(f"{n}\tv{i}\n" for i, n in enumerate(names)))
    base[4] = str(tmp_path / "wide.list")
    refused(["--cohort", "--cohort-permanova", factors, "--cohort-permanova-pairwise"], "line 34", "column many", "'v32'", "more than 32")
    # a good file passes on to the device and the database (there is none); the skipped lines are counted; the largest seed
    run = subprocess.run(base + ["--cohort", "--cohort-permanova", factors, "--cohort-permanova-seed", "18446744073709551615",
                                 "--cohort-permanova-permutations", "999999"], capture_output=True, text=True)
    assert run.returncode == 255 and "--cohort-permanova" not in run.stderr and "factors.tsv" not in run.stderr, run.stderr
    assert "Cohort factors: 1 columns, 0 lines of samples that are not in the list skipped" in run.stdout


def test_launcher_passes_the_flags_only_when_given():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw)
    assert "permanova" not in " ".join(default) and "permanova" not in " ".join(epik.driver_command(**kw, cohort=True))
    assert epik.driver_command(**kw, cohort_permanova=None, cohort_permanova_permutations=None, cohort_permanova_seed=None,
                               cohort_permanova_pairwise=False) == default
    assert epik.driver_command(**kw, cohort=True, cohort_permanova="f.tsv")[:-1] == default[:-1] + ["--cohort", "--cohort-permanova", "f.tsv"]
    assert epik.driver_command(**kw, cohort=True, cohort_alpha=True, cohort_dispersion=True, cohort_permanova="f.tsv",
                               cohort_permanova_permutations=9999, cohort_permanova_seed=(1 << 64) - 1, cohort_permanova_pairwise=True,
                               taxonomy="t.tsv", strand="both")[:-1] == \
        default[:-1] + ["--strand", "both", "--cohort", "--cohort-alpha", "--cohort-dispersion", "--cohort-permanova", "f.tsv",
                        "--cohort-permanova-permutations", "9999", "--cohort-permanova-seed", "18446744073709551615",
                        "--cohort-permanova-pairwise", "--taxonomy", "t.tsv"]
    for bad in (dict(cohort_permanova="f.tsv"), dict(cohort=True, cohort_permanova_permutations=9), dict(cohort=True, cohort_permanova_seed=9),
                dict(cohort=True, cohort_permanova_pairwise=True), dict(cohort_permanova_pairwise=True)):
        with pytest.raises(click.UsageError):
            epik.driver_command(**kw, **bad)
    me = os.path.join(ROOT, "epik.py")
    out = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("--cohort-permanova ", "--cohort-permanova-permutations", "--cohort-permanova-seed", "--cohort-permanova-pairwise"):
        assert flag in out.stdout, flag
    for flags, word in ((["--cohort-permanova", me], "--cohort"), (["--cohort", "--cohort-permanova-pairwise"], "--cohort-permanova"),
                        (["--cohort", "--cohort-permanova-seed", "3"], "--cohort-permanova"),
                        (["--cohort", "--cohort-permanova", me, "--cohort-permanova-permutations", "0"], "999999"),
                        (["--cohort", "--cohort-permanova", me, "--cohort-permanova-permutations", "1000000"], "999999"),
                        (["--cohort", "--cohort-permanova", me, "--cohort-permanova-seed", "-1"], "18446744073709551615")):
        run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, *flags, me], capture_output=True, text=True)
        assert run.returncode == 2 and word in run.stderr, (flags, run.stdout, run.stderr)


# ---- 8. the host code stand-alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitized", [False, True])
def test_host_test_binary_permanova_is_the_library_s(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    for num_samples, permutations, pairwise in ((2, 1, True), (5, 64, True), (33, 65, False), (65, 20, True)):
        mass, first, bl, rng = cohort_input("tree15", num_samples, seed=9)
        labels = factor_columns(rng, mass, pairwise)
        _cells_input(tmp_path / "mass.bin", mass, first, bl)
        (tmp_path / "labels.bin").write_bytes(labels.tobytes())
        run = subprocess.run([binary, "permanova", str(tmp_path / "out.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "labels.bin"),
                              str(permutations), "12345678901234567890", str(int(pairwise))], capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (num_samples, run.stderr)
        want = cohort_mod.permanova_host(mass, first, bl, labels, permutations, 12345678901234567890, pairwise)
        assert (tmp_path / "out.bin").read_bytes() == want.records.tobytes() + want.ssw.tobytes() + want.group_ss.tobytes(), num_samples
    bad = labels.copy()
    bad[1, 0] = 256
    (tmp_path / "labels.bin").write_bytes(bad.tobytes())
    run = subprocess.run([binary, "permanova", str(tmp_path / "o.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "labels.bin"), "9", "1", "0"],
                         capture_output=True, text=True)
    assert run.returncode == 1 and "sample 1" in run.stderr and "256" in run.stderr
    (tmp_path / "labels.bin").write_bytes(b"\0" * 6)
    run = subprocess.run([binary, "permanova", str(tmp_path / "o.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "labels.bin"), "9", "1", "0"],
                         capture_output=True, text=True)
    assert run.returncode == 1 and "uint32 [S][M]" in run.stderr
    # the factor file through the stand-alone reader: an error names its line
    (tmp_path / "names.txt").write_text("".join(f"n{i}\n" for i in range(mass.shape[0])))
    (tmp_path / "factors.tsv").write_text("sample\tstate\n" + "".join(f"n{i}\tx\n" for i in range(mass.shape[0])) + "n3\ty\n")
    run = subprocess.run([binary, "permanova-tsv", str(tmp_path / "o.tsv"), str(tmp_path / "mass.bin"), str(tmp_path / "names.txt"),
                          str(tmp_path / "factors.tsv"), "9", "1", "0"], capture_output=True, text=True)
    assert run.returncode == 1 and f"line {mass.shape[0] + 2}" in run.stderr and "'n3'" in run.stderr and "twice" in run.stderr
