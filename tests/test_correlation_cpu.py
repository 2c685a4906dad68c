"""Edge correlation with per-sample metadata and edge dispersion of a cohort's samples on the host:
epik_amd_cohort_correlation_host and epik_amd_cohort_dispersion_host against the rule of include/epik_amd.h restated in numpy,
bit for bit, NA bits included; the values against numpy.corrcoef; a case by hand; the properties; forged cells; the symbols
and the errors; the metadata file, the two output files, the launcher and the drivers; and the host code stand-alone.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod
from test_capi_cpu import _header_symbols
from test_cohort_cpu import host_bins, numpy_first, random_cells, same_bits, tree_case  # noqa: F401 (host_bins: a fixture)
from test_diversity_cpu import forged_diversity_cohorts
from test_epca_cpu import forged_epca_cohorts
from test_squash_cpu import BALANCED, numpy_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
NA = np.array([capi.NA_BITS], dtype=U64).view(np.float64)[0]
CORR_FIELDS = ("mass_pearson", "mass_spearman", "imbalance_pearson", "imbalance_spearman")
DISP_FIELDS = ("mass_mean", "mass_var", "mass_sd", "mass_cv", "mass_vmr", "imbalance_mean", "imbalance_var", "imbalance_sd")


# ---- the rule, restated ----------------------------------------------------------------------------------------------
def counted_midranks(v):
    """rank(x)_j = #{i: x_i < x_j} + 0.5 * (#{i: x_i == x_j} + 1) down every column of v[L][K], by counting."""
    v = np.asarray(v, dtype=np.float64)
    less = (v[None, :, :] < v[:, None, :]).sum(axis=1)          # [j][k]: the i with v[i] < v[j]
    equal = (v[None, :, :] == v[:, None, :]).sum(axis=1)
    return less.astype(np.float64) + 0.5 * (equal + 1).astype(np.float64)


def sequential(terms):
    """The sequential sum from +0.0 in ascending j of terms[L][K], a python loop: acc = acc + terms[j]."""
    acc = np.zeros(terms.shape[1])
    for j in range(terms.shape[0]):
        acc = acc + terms[j]
    return acc


def numpy_pearson(x, y):
    """P(x[:, k], y) of the rule for every column k of x[L][K], y[L]: NA unless L >= 3 and den > 0."""
    count, k = x.shape
    out = np.full(k, NA)
    if count < 3:
        return out
    y = np.asarray(y, dtype=np.float64)[:, None]
    mx, my = sequential(x) / float(count), sequential(y) / float(count)
    dx, dy = x - mx[None, :], y - my[None, :]
    sxx, syy, sxy = sequential(dx * dx), sequential(dy * dy), sequential(dx * dy)
    den = np.sqrt(sxx) * np.sqrt(syy)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = sxy / den
    r = np.where(r < -1.0, -1.0, r)
    r = np.where(r > 1.0, 1.0, r)
    return np.where(den > 0.0, r, out)


def branch_vectors(mass, first, rows):
    """xm[L][N], xi[L][N] over the samples `rows`, and the inner branches."""
    c, b, total = numpy_planes(mass, first)
    xm = np.asarray(mass, U64)[rows].astype(np.float64) / total[rows].astype(np.float64)[:, None]
    xi = (b[rows] + c[rows]) - 1.0
    return xm, xi, np.asarray(first, np.int64) < np.arange(len(first))


def numpy_correlation(mass, first, meta):
    """(capi.CORRELATION [M][N], used uint32 [M]) of the rule."""
    mass, meta = np.asarray(mass, U64), np.asarray(meta, np.float64)
    total = mass.sum(axis=1, dtype=U64)
    n, m = mass.shape[1], meta.shape[1]
    out = np.zeros((m, n), dtype=capi.CORRELATION)
    used = np.zeros(m, dtype=np.uint32)
    for c in range(m):
        rows = np.array([s for s in range(len(mass)) if total[s] != 0 and not np.isnan(meta[s, c])], dtype=np.int64)
        used[c] = len(rows)
        for f in CORR_FIELDS:
            out[f][c] = NA
        if len(rows) < 3:
            continue
        y = meta[rows, c]
        ry = counted_midranks(y[:, None])[:, 0]
        xm, xi, inner = branch_vectors(mass, first, rows)
        out["mass_pearson"][c] = numpy_pearson(xm, y)
        out["mass_spearman"][c] = numpy_pearson(counted_midranks(xm), ry)
        out["imbalance_pearson"][c] = np.where(inner, numpy_pearson(xi, y), NA)
        out["imbalance_spearman"][c] = np.where(inner, numpy_pearson(counted_midranks(xi), ry), NA)
    return out, used


def numpy_dispersion(mass, first):
    """capi.DISPERSION [N] of the rule."""
    mass = np.asarray(mass, U64)
    total = mass.sum(axis=1, dtype=U64)
    n = mass.shape[1]
    out = np.zeros(n, dtype=capi.DISPERSION)
    for f in DISP_FIELDS:
        out[f] = NA
    rows = np.flatnonzero(total != 0)
    count = len(rows)
    if count == 0:
        return out
    xm, xi, inner = branch_vectors(mass, first, rows)
    for kind, x, keep in (("mass", xm, np.ones(n, bool)), ("imbalance", xi, inner)):
        mean = sequential(x) / float(count)
        d = x - mean[None, :]
        var = sequential(d * d) / float(count)
        sd = np.sqrt(var)
        out[kind + "_mean"], out[kind + "_var"], out[kind + "_sd"] = np.where(keep, mean, NA), np.where(keep, var, NA), np.where(keep, sd, NA)
        if kind == "mass":
            with np.errstate(invalid="ignore", divide="ignore"):
                out["mass_cv"], out["mass_vmr"] = np.where(mean > 0.0, sd / mean, NA), np.where(mean > 0.0, var / mean, NA)
    return out


def same_records(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def is_na(x):
    return np.asarray(x, np.float64).view(U64) == U64(capi.NA_BITS)


def only_na_or_numbers(records):
    """No arithmetic NaN reached an output: every NaN is the NA pattern."""
    v = np.ascontiguousarray(records).view(np.float64)
    return bool((is_na(v) | ~np.isnan(v)).all())


def metadata(rng, mass):
    """[S][3]: a continuous column, one rounded to integers (ties), one with about a third missing."""
    s = len(mass)
    cont = rng.normal(size=s) * 3.0 + 7.0
    meta = np.stack([cont, np.round(rng.normal(size=s) * 1.5), np.where(rng.random(s) < 1 / 3, np.nan, rng.random(s))], axis=1)
    return meta


# Seven samples with one empty leave six with mass, and random_cells leaves a cell empty three times in ten: on the large tree
# most seeds leave some branch without mass in all six, which is constant and NA by the rule.
# test_no_mass_pearson_of_the_continuous_column_is_undefined needs inputs without such a branch, so the seed of a cohort is
# the first at which every branch has mass in some sample -- a property of the input alone, asserted there.
SEED_BASE = 5100
SEED_STEPS = {("tree2999", 7): 21}
SAMPLES = (1, 2, 3, 7, 33)
INPUTS = {}


def cohort_input(tree_name, num_samples):
    """(mass, first, meta, records, used, dispersion) of a random cohort with one empty sample: the host's results, computed once."""
    key = (tree_name, num_samples)
    if key not in INPUTS:
        parent, _ = tree_case(tree_name)
        first = numpy_first(parent)
        rng = np.random.default_rng(SEED_BASE + 100 * SEED_STEPS.get(key, 0) + num_samples)
        mass = random_cells(rng, num_samples, len(parent), empty=1, bits=42)
        meta = metadata(rng, mass)
        records, used = cohort_mod.correlation_host(mass, first, meta)
        INPUTS[key] = (mass, first, meta, records, used, cohort_mod.dispersion_host(mass, first))
    return INPUTS[key]


# ---- 1. the host mirror against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("tree_name", ["tree15", "tree2999"])
@pytest.mark.parametrize("num_samples", SAMPLES)
def test_host_equals_the_numpy_restatement_bit_for_bit(tree_name, num_samples):
    mass, first, meta, records, used, dispersion = cohort_input(tree_name, num_samples)
    want, want_used = numpy_correlation(mass, first, meta)
    assert np.array_equal(used, want_used) and used[0] == max(num_samples - 1, 1) and (used[2] <= used[0])
    for f in CORR_FIELDS:
        assert same_bits(records[f], want[f]), (f, np.argwhere(records[f].view(U64) != want[f].view(U64))[:10])
    assert same_records(records, want) and only_na_or_numbers(records)
    want = numpy_dispersion(mass, first)
    for f in DISP_FIELDS:
        assert same_bits(dispersion[f], want[f]), (f, np.argwhere(dispersion[f].view(U64) != want[f].view(U64))[:10])
    assert same_records(dispersion, want) and only_na_or_numbers(dispersion)
    inner = first < np.arange(len(first))
    assert is_na(records["imbalance_pearson"][:, ~inner]).all() and is_na(dispersion["imbalance_mean"][~inner]).all()
    assert not is_na(dispersion["imbalance_mean"][inner]).any() and not is_na(dispersion["mass_sd"]).any()
    if num_samples < 4:                                       # one sample is empty: fewer than three are used
        assert is_na(records.view(np.float64)).all()


# ---- 2. the values, independently ------------------------------------------------------------------------------------------
def argsort_midranks(x):
    """Midranks by a stable sort: the runs of equal values share the mean of their positions."""
    x = np.asarray(x, dtype=np.float64)
    order = np.argsort(x, kind="stable")
    ranks = np.zeros(len(x))
    i = 0
    while i < len(x):
        j = i
        while j + 1 < len(x) and x[order[j + 1]] == x[order[i]]:
            j += 1
        ranks[order[i:j + 1]] = (i + j) / 2.0 + 1.0
        i = j + 1
    return ranks


# the worst deviation of the host mirror from numpy.corrcoef measured on these inputs, in units of 2^-52: Pearson 1.5,
# Spearman 1.0; the bound is 8 times that, the margin of section 3.10
WORST_PEARSON, WORST_SPEARMAN = 1.5, 1.0


def test_the_values_agree_with_numpy_corrcoef_and_sorted_ranks():
    worst = {"pearson": 0.0, "spearman": 0.0}
    compared = 0
    for tree_name in ("tree15", "tree2999"):
        for num_samples in (7, 33):
            mass, first, meta, records, used, _ = cohort_input(tree_name, num_samples)
            total = mass.sum(axis=1, dtype=U64)
            step = 1 if tree_name == "tree15" else 37             # every branch of the small tree, a share of the large one's
            for c in range(meta.shape[1]):
                rows = np.flatnonzero((total != 0) & ~np.isnan(meta[:, c]))
                y = meta[rows, c]
                ry = argsort_midranks(y)
                assert np.array_equal(ry, counted_midranks(y[:, None])[:, 0])
                xm, xi, inner = branch_vectors(mass, first, rows)
                for kind, x in (("mass", xm), ("imbalance", xi)):
                    for b in range(0, len(first), step):
                        rx = argsort_midranks(x[:, b])
                        assert np.array_equal(rx, counted_midranks(x[:, b:b + 1])[:, 0]), (kind, b)   # the ranks: exactly
                        for name, u, v in (("pearson", x[:, b], y), ("spearman", rx, ry)):
                            got = records[f"{kind}_{name}"][c, b]
                            if is_na(got):
                                continue
                            want = np.corrcoef(u, v)[0, 1]
                            assert np.isfinite(want), (kind, name, c, b)
                            worst[name] = max(worst[name], abs(got - want) / 2.0 ** -52)
                            compared += 1
    print(f"worst deviation from numpy.corrcoef in units of 2^-52: {worst}, {compared} values")
    assert compared > 1000
    assert worst["pearson"] <= 8 * WORST_PEARSON and worst["spearman"] <= 8 * WORST_SPEARMAN, worst


# ---- 3. by hand ----------------------------------------------------------------------------------------------------------------
def test_a_case_by_hand_on_the_seven_branch_tree():
    first = numpy_first(BALANCED)                                # ((0,1)2,(3,4)5)6
    assert np.array_equal(argsort_midranks([1, 2, 2, 4]), [1.0, 2.5, 2.5, 4.0])
    assert np.array_equal(counted_midranks(np.array([[1.0], [2.0], [2.0], [4.0]]))[:, 0], [1.0, 2.5, 2.5, 4.0])
    assert np.array_equal(counted_midranks(np.array([[1.0], [1.0], [3.0], [3.0]]))[:, 0], [1.5, 1.5, 3.5, 3.5])
    assert np.array_equal(counted_midranks(np.array([[-0.0], [0.0], [3.0]]))[:, 0], [1.5, 1.5, 3.0])
    # every sample holds 8: a on leaf 0, 8 - a on leaf 3, a = 1, 1, 3, 3.  xm[0] = a / 8 has the mean 1/4, deviations
    # -+1/8, sxx = 1/16 and sqrt 1/4; its ranks 1.5, 1.5, 3.5, 3.5 have the mean 5/2, deviations -+1, sxx = 4 and sqrt 2.
    a = np.array([1, 1, 3, 3], U64)
    mass = np.zeros((4, 7), U64)
    mass[:, 0], mass[:, 3] = a, U64(8) - a
    # y0 = 10 a: dy = -+10, syy = 400, sqrt 20, sxy = 4 * (1/8) * 10 = 5 = den: r = 1.  y1 = -y0: r = -1.
    # y2 = 1, -1, -1, 1: the mean 0, sxy = -1/8 + 1/8 - 1/8 + 1/8 = 0: r = 0, and so with its ranks 3.5, 1.5, 1.5, 3.5.
    meta = np.array([[10.0, -10.0, 1.0], [10.0, -10.0, -1.0], [30.0, -30.0, -1.0], [30.0, -30.0, 1.0]])
    records, used = cohort_mod.correlation_host(mass, first, meta)
    assert list(used) == [4, 4, 4]
    for f in ("mass_pearson", "mass_spearman"):
        assert same_bits(records[f][:, 0], [1.0, -1.0, 0.0]), f          # leaf 0 rises with a
        assert same_bits(records[f][:, 3], [-1.0, 1.0, 0.0]), f          # leaf 3 falls
        assert is_na(records[f][:, [1, 2, 4, 5, 6]]).all(), f            # no mass in any sample: constant
    for f in ("imbalance_pearson", "imbalance_spearman"):
        # branch 2 has a / 8 below it and in its clade: xi = a / 4 - 1; branch 5 likewise 1 - a / 4; the root has all on both sides
        assert same_bits(records[f][:, 2], [1.0, -1.0, 0.0]) and same_bits(records[f][:, 5], [-1.0, 1.0, 0.0]), f
        assert is_na(records[f][:, [0, 1, 3, 4, 6]]).all(), f
    disp = cohort_mod.dispersion_host(mass, first)
    assert same_bits(disp["mass_mean"], [0.25, 0, 0, 0.75, 0, 0, 0]) and same_bits(disp["mass_var"], [1 / 64, 0, 0, 1 / 64, 0, 0, 0])
    assert same_bits(disp["mass_sd"], [0.125, 0, 0, 0.125, 0, 0, 0])
    assert same_bits(disp["mass_cv"][[0, 3]], [0.5, 0.125 / 0.75]) and same_bits(disp["mass_vmr"][[0, 3]], [1 / 16, (1 / 64) / 0.75])
    assert is_na(disp["mass_cv"][[1, 2, 4, 5, 6]]).all() and is_na(disp["mass_vmr"][[1, 2, 4, 5, 6]]).all()
    assert same_bits(disp["imbalance_mean"][[2, 5, 6]], [-0.5, 0.5, 1.0]) and same_bits(disp["imbalance_var"][[2, 5, 6]], [1 / 16, 1 / 16, 0])
    assert same_bits(disp["imbalance_sd"][[2, 5, 6]], [0.25, 0.25, 0.0]) and is_na(disp["imbalance_sd"][[0, 1, 3, 4]]).all()


# ---- 4. the properties -----------------------------------------------------------------------------------------------------
def test_properties_on_random_cohorts():
    for tree_name, num_samples in (("tree15", 7), ("tree15", 33), ("tree2999", 33)):
        mass, first, meta, records, used, _ = cohort_input(tree_name, num_samples)
        values = records.view(np.float64)
        defined = ~is_na(values)
        assert defined.any() and (values[defined] >= -1.0).all() and (values[defined] <= 1.0).all()
        # a column negated: every defined value negated bit for bit (a zero stays +0.0: the sums start from +0.0)
        negated, used_n = cohort_mod.correlation_host(mass, first, -meta)
        assert np.array_equal(used_n, used)
        got, want = negated.view(np.float64), np.where(defined & (values != 0.0), -values, values)
        assert same_bits(got, want), (tree_name, num_samples)
        # y -> 3 y + 1 on the integer column, exact and strictly increasing: Spearman's bits stay
        mapped = meta.copy()
        mapped[:, 1] = 3.0 * meta[:, 1] + 1.0
        again, _ = cohort_mod.correlation_host(mass, first, mapped)
        for f in ("mass_spearman", "imbalance_spearman"):
            assert same_bits(again[f], records[f]), f
        assert same_bits(again["mass_pearson"][[0, 2]], records["mass_pearson"][[0, 2]])
        # the columns permuted: the records permuted
        order = [2, 0, 1]
        permuted, used_p = cohort_mod.correlation_host(mass, first, meta[:, order])
        assert same_records(permuted, records[order]) and np.array_equal(used_p, used[order])
        # a constant column; a column with two values present; a column alone gives what it gives among others
        special = np.full((num_samples, 2), np.nan)
        special[:, 0] = 2.5
        special[:3, 1] = [0.5, 9.0, 4.0]                      # (sample 1 is the empty one: two of the three values are used)
        got, used_s = cohort_mod.correlation_host(mass, first, special)
        assert list(used_s) == [num_samples - 1, 2] and is_na(got.view(np.float64)).all()
        alone, used_a = cohort_mod.correlation_host(mass, first, meta[:, 2:3])
        assert same_records(alone[0], records[2]) and used_a[0] == used[2]
        # a leaf's imbalance
        inner = first < np.arange(len(first))
        assert is_na(records["imbalance_pearson"][:, ~inner]).all() and is_na(records["imbalance_spearman"][:, ~inner]).all()
        # a branch whose mass is the same in all samples (none: the sums are exact whatever the count)
        flat = mass.copy()
        flat[:, 3] = 0
        got, _ = cohort_mod.correlation_host(flat, first, meta)
        assert is_na(got["mass_pearson"][:, 3]).all() and is_na(got["mass_spearman"][:, 3]).all()
    # ... and the same share of the same total in every sample, a power of two: xm = 1/4 whatever the rest does
    first = numpy_first(BALANCED)
    mass = np.array([[4, 1, 0, 11, 0, 0, 0], [4, 5, 0, 7, 0, 0, 0], [4, 0, 3, 9, 0, 0, 0], [4, 2, 2, 2, 6, 0, 0]], U64)
    got, _ = cohort_mod.correlation_host(mass, first, np.array([[1.0], [2.0], [4.0], [3.0]]))
    assert is_na(got["mass_pearson"][0, 0]) and is_na(got["mass_spearman"][0, 0]) and not is_na(got["mass_pearson"][0, 1])


# ---- 5. forged cells ---------------------------------------------------------------------------------------------------
def forged_correlation_cohorts():
    """name -> (mass, parent): the forged cohorts of the epca and diversity tests, and one used sample among empty ones"""
    cases = {"epca: " + name: (mass, parent) for name, (mass, parent, _) in forged_epca_cohorts().items()}
    cases.update({"diversity: " + name: (mass, parent) for name, (mass, _, parent, _) in forged_diversity_cohorts().items()})
    parent, _ = tree_case("tree15")
    x = random_cells(np.random.default_rng(46), 1, len(parent), bits=42)[0]
    zero = np.zeros(len(parent), U64)
    cases["one used sample"] = (np.stack([zero, x, zero, zero]), parent)
    y = random_cells(np.random.default_rng(47), 5, len(parent), bits=42)
    cases["five identical"] = (np.stack([y[0]] * 5), parent)
    return cases


def forged_metadata(name, mass):
    return metadata(np.random.default_rng(len(name) + 13 * len(mass)), mass)


@pytest.mark.parametrize("name", sorted(forged_correlation_cohorts()))
def test_forged_cells(name):
    mass, parent = forged_correlation_cohorts()[name]
    first = numpy_first(parent)
    meta = forged_metadata(name, mass)
    lib = capi.load()
    s, n = mass.shape
    mass = np.ascontiguousarray(mass, U64)
    # into poisoned buffers: every cell is written
    out = np.full(3 * n * 4, -7.25).view(capi.CORRELATION)
    used = np.full(3, 0xA5A5A5A5, dtype=np.uint32)
    capi.check(lib.epik_amd_cohort_correlation_host(mass.ctypes.data, s, n, first.ctypes.data, meta.ctypes.data, 3, out.ctypes.data,
                                                    used.ctypes.data))
    want, want_used = numpy_correlation(mass, first, meta)
    assert same_records(out.reshape(3, n), want) and np.array_equal(used, want_used), name
    assert not (out.view(np.float64) == -7.25).any() and only_na_or_numbers(out)
    disp = np.full(n * 8, -7.25).view(capi.DISPERSION)
    capi.check(lib.epik_amd_cohort_dispersion_host(mass.ctypes.data, s, n, first.ctypes.data, disp.ctypes.data))
    assert same_records(disp, numpy_dispersion(mass, first)), name
    assert not (disp.view(np.float64) == -7.25).any() and only_na_or_numbers(disp)
    total = mass.sum(axis=1, dtype=U64)
    if not total.any():
        assert is_na(out.view(np.float64)).all() and is_na(disp.view(np.float64)).all() and not used.any()
    if name in ("one used sample", "epca: all identical", "epca: four identical on a leaf"):
        assert is_na(out.view(np.float64)).all()                          # fewer than three samples, or every x 0 or 1
    if name == "five identical":                                          # every rank is 3, whatever the mean of five equal masses rounds to
        assert is_na(out["mass_spearman"]).all() and is_na(out["imbalance_spearman"]).all()
    if name == "one used sample":
        assert same_bits(disp["mass_var"], np.zeros(n)) and not is_na(disp["mass_mean"]).any()


def test_no_mass_pearson_of_the_continuous_column_is_undefined():
    """A broken guard must not pass as "undefined": on the random cohorts of test 1 with seven samples or more every
    branch's mass_pearson with the continuous column is a number."""
    for tree_name in ("tree15", "tree2999"):
        for num_samples in (7, 33):
            mass, first, meta, records, used, _ = cohort_input(tree_name, num_samples)
            assert mass.any(axis=0).all(), "the seed must leave no branch without mass (see SEED_STEPS)"
            assert not is_na(records["mass_pearson"][0]).any(), (tree_name, num_samples, np.flatnonzero(is_na(records["mass_pearson"][0]))[:10])


# ---- 6. the C ABI, the files, the launcher, the drivers ---------------------------------------------------------------------
def test_correlation_symbols_exist_and_refuse_what_the_header_says():
    lib = capi.load()
    names = ("epik_amd_cohort_correlation_device", "epik_amd_cohort_correlation", "epik_amd_cohort_correlation_host",
             "epik_amd_cohort_dispersion_device", "epik_amd_cohort_dispersion", "epik_amd_cohort_dispersion_host")
    for name in names:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == _header_symbols() and capi.ABI_VERSION == 3
    assert capi.CORRELATION.itemsize == 32 and [capi.CORRELATION.fields[k][1] for k in CORR_FIELDS] == [0, 8, 16, 24]
    assert capi.DISPERSION.itemsize == 64 and [capi.DISPERSION.fields[k][1] for k in DISP_FIELDS] == list(range(0, 64, 8))
    assert capi.CORRELATION_MAX_COLUMNS == 64 and capi.NA_BITS == 0x7FF8000000000000 and np.isnan(NA)
    err = lambda: lib.epik_amd_last_error().decode()
    first = cohort_mod.first_of([2, 2, -1])
    cells = np.ones((4, 3), U64)
    meta = np.arange(8.0).reshape(4, 2)
    out, used, disp = np.zeros(6, dtype=capi.CORRELATION), np.zeros(2, np.uint32), np.zeros(3, dtype=capi.DISPERSION)
    assert lib.epik_amd_cohort_correlation_device(None, None, meta.ctypes.data, 2, None, None, None) == capi.ERR_INVALID and "null cohort" in err()
    assert lib.epik_amd_cohort_correlation(None, None, meta.ctypes.data, 2, out.ctypes.data, used.ctypes.data) == capi.ERR_INVALID
    assert "null cohort" in err()
    assert lib.epik_amd_cohort_dispersion_device(None, None, None, None) == capi.ERR_INVALID and "null cohort" in err()
    assert lib.epik_amd_cohort_dispersion(None, None, disp.ctypes.data) == capi.ERR_INVALID and "null cohort" in err()
    ptr = lambda x: x.ctypes.data if x is not None else None
    corr_args = lambda m=cells, s=4, n=3, f=first, y=meta, c=2, o=out, u=used: (ptr(m), s, n, ptr(f), ptr(y), c, ptr(o), ptr(u))
    disp_args = lambda m=cells, s=4, n=3, f=first, o=disp: (ptr(m), s, n, ptr(f), ptr(o))
    assert lib.epik_amd_cohort_correlation_host(*corr_args()) == capi.OK and lib.epik_amd_cohort_dispersion_host(*disp_args()) == capi.OK
    wide = np.zeros((4, 65))
    assert lib.epik_amd_cohort_correlation_host(*corr_args(y=wide, c=64, o=np.zeros(64 * 3, dtype=capi.CORRELATION), u=np.zeros(64, np.uint32))) == capi.OK
    for host, args, nulls in ((lib.epik_amd_cohort_correlation_host, corr_args, ("m", "f", "y", "o", "u")),
                              (lib.epik_amd_cohort_dispersion_host, disp_args, ("m", "f", "o"))):
        assert host(*args(s=0)) == capi.ERR_INVALID and "num_samples is 0" in err()
        assert host(*args(n=0)) == capi.ERR_INVALID and "at least one branch" in err()
        for missing in nulls:
            assert host(*args(**{missing: None})) == capi.ERR_INVALID and "null argument" in err(), missing
        assert host(*args(f=np.array([0, 2, 0], dtype=np.uint32))) == capi.ERR_INVALID and "branch 1" in err() and "first" in err()
    for bad in (0, 65, 0xFFFFFFFF):
        assert lib.epik_amd_cohort_correlation_host(*corr_args(y=wide, c=bad)) == capi.ERR_INVALID
        assert "num_columns" in err() and "[1, 64]" in err()
    for bad in (np.inf, -np.inf):
        y = meta.copy()
        y[2, 1] = bad
        assert lib.epik_amd_cohort_correlation_host(*corr_args(y=y)) == capi.ERR_INVALID
        assert "sample 2" in err() and "column 1" in err() and "infinite" in err()
    with pytest.raises(capi.EpikAmdError):
        cohort_mod.correlation_host(cells, first, np.zeros((4, 65)))
    with pytest.raises(capi.EpikAmdError):
        cohort_mod.correlation_host(cells, first, np.zeros((4, 0)))
    with pytest.raises(ValueError):
        cohort_mod.correlation_host(cells, first, np.zeros((3, 2)))
    with pytest.raises(ValueError):
        cohort_mod.dispersion_host(cells, first[:2])


GOOD_METADATA = ("# a comment\n\nsample\tpH\tdepth m\tcase\n"
                 "b\t7.25\t1e2\t1\n"
                 "stranger\t1\t2\t3\n"
                 "a\t-.5\tNA\t0\n"
                 "\n# another\n"
                 "c\t+6.\t\t1E-3\n")


def test_the_metadata_file(tmp_path):
    path = tmp_path / "meta.tsv"
    path.write_text(GOOD_METADATA)
    columns, values, skipped = cohort_mod.read_metadata(str(path), ["a", "b", "c"])
    assert columns == ["pH", "depth m", "case"] and skipped == 1 and values.shape == (3, 3)
    assert same_bits(values, [[-0.5, NA, 0.0], [7.25, 100.0, 1.0], [6.0, NA, 0.001]])
    path.write_bytes(GOOD_METADATA.replace("\n", "\r\n").encode())
    assert same_bits(cohort_mod.read_metadata(str(path), ["a", "b", "c"])[1], values)
    head = "sample\tpH\tdepth\n"
    many = "sample" + "".join(f"\tc{i}" for i in range(65)) + "\n"
    for text, words in ((head + "a\t1\t2\nb\t1\tx\nc\t1\t2\n", ("line 3", "column depth", "'x'")),
                        (head + "a\t1\t2\nb\tnan\t1\nc\t1\t2\n", ("line 3", "column pH", "'nan'")),
                        (head + "a\t1\t2\nb\t1\tinf\nc\t1\t2\n", ("line 3", "column depth", "'inf'")),
                        (head + "a\t1\t0x10\nb\t1\t1\nc\t1\t2\n", ("line 2", "column depth", "'0x10'")),
                        (head + "a\t1\t 2\nb\t1\t1\nc\t1\t2\n", ("line 2", "column depth")),
                        (head + "a\t1\t1e\nb\t1\t1\nc\t1\t2\n", ("line 2", "column depth", "'1e'")),
                        (head + "a\t.\t1\nb\t1\t1\nc\t1\t2\n", ("line 2", "column pH", "'.'")),
                        (head + "# x\na\t1\t1e999\nb\t1\t1\nc\t1\t2\n", ("line 3", "column depth", "overflows")),
                        (head + "a\t1\t2\nb\t1\nc\t1\t2\n", ("line 3", "2 fields, not 3")),
                        (head + "a\t1\t2\nb\t1\t2\t3\nc\t1\t2\n", ("line 3", "4 fields, not 3")),
                        (head + "a\t1\t2\nb\t1\t2\n\na\t3\t4\nc\t1\t2\n", ("line 5", "'a'", "twice")),
                        (head + "a\t1\t2\nb\t1\t2\n", ("no line", "'c'")),
                        ("name\tpH\na\t1\nb\t1\nc\t1\n", ("line 1", "'sample'")),
                        ("sample\n", ("line 1", "0 columns")),
                        (many, ("line 1", "65 columns")),
                        ("sample\tpH\tpH\n", ("line 1", "'pH'", "twice")),
                        ("sample\tpH\t\n", ("line 1", "column 2", "empty")),
                        ("# nothing\n\n", ("no header",))):
        path.write_text(text)
        with pytest.raises(ValueError) as e:
            cohort_mod.read_metadata(str(path), ["a", "b", "c"])
        assert all(w in str(e.value) for w in words), (text, str(e.value))


def test_the_two_files_read_back_and_keep_names(tmp_path):
    names = ["a", "skin 3", "it's", "none", "z.9_-", "q"]
    parent, _ = tree_case("tree15")
    first = numpy_first(parent)
    rng = np.random.default_rng(8)
    mass = random_cells(rng, 6, len(parent), bits=42)
    mass[3] = 0
    meta = metadata(rng, mass)
    meta[0, 2] = np.nan
    columns = ["pH", "depth m", "case"]
    records, used = cohort_mod.correlation_host(mass, first, meta)
    totals = cohort_mod.totals_of(mass)
    text = cohort_mod.format_correlation_tsv(names, totals, columns, records, used)
    lines = text.split("\n")
    assert lines[:6] == ["# epik_amd correlation v1  samples=6 used=5 columns=3", "# unused\tnone", "# column\t0\tpH\t5",
                         f"# column\t1\tdepth m\t5", f"# column\t2\tcase\t{used[2]}",
                         "edge_num\tcolumn\tmass_pearson\tmass_spearman\timbalance_pearson\timbalance_spearman"]
    assert lines[6] == "0\tpH\t%.17g\t%.17g\tNA\tNA" % (records["mass_pearson"][0, 0], records["mass_spearman"][0, 0])
    assert lines[7].startswith("0\tdepth m\t") and lines[9].startswith("1\tpH\t") and len(lines) == 6 + 3 * len(first) + 1
    path = tmp_path / "cohort_correlation_x.tsv"
    path.write_bytes(text.encode())
    back_columns, back, back_used, info = cohort_mod.read_correlation_tsv(str(path))
    assert back_columns == columns and np.array_equal(back_used, used) and info == {"samples": 6, "used": 5, "unused": ["none"]}
    assert same_records(back, records)
    disp = cohort_mod.dispersion_host(mass, first)
    text = cohort_mod.format_dispersion_tsv(names, totals, disp)
    lines = text.split("\n")
    assert lines[:3] == ["# epik_amd dispersion v1  samples=6 used=5", "# unused\tnone", "edge_num\t" + "\t".join(DISP_FIELDS)]
    assert lines[3] == "0" + "".join("\t%.17g" % disp[f][0] for f in DISP_FIELDS[:5]) + "\tNA\tNA\tNA" and len(lines) == 3 + len(first) + 1
    disp_path = tmp_path / "cohort_dispersion_x.tsv"
    disp_path.write_bytes(text.encode())
    back, info = cohort_mod.read_dispersion_tsv(str(disp_path))
    assert same_records(back, disp) and info == {"samples": 6, "used": 5, "unused": ["none"]}
    path.write_text("# something else\n")
    with pytest.raises(ValueError):
        cohort_mod.read_correlation_tsv(str(path))
    with pytest.raises(ValueError):
        cohort_mod.read_dispersion_tsv(str(path))
    with pytest.raises(ValueError):
        cohort_mod.format_correlation_tsv(names[:4], totals, columns, records, used)
    with pytest.raises(ValueError):
        cohort_mod.format_correlation_tsv(names, totals, columns[:2], records, used)
    with pytest.raises(ValueError):
        cohort_mod.format_dispersion_tsv(names, totals[:2], disp)
    # nothing used: every value NA
    zero = np.zeros((2, 3), U64)
    small = cohort_mod.first_of([2, 2, -1])
    assert cohort_mod.format_dispersion_tsv(["x y", "q"], [0, 0], cohort_mod.dispersion_host(zero, small)) == (
        "# epik_amd dispersion v1  samples=2 used=0\n# unused\tx y\n# unused\tq\nedge_num\t" + "\t".join(DISP_FIELDS) + "\n" +
        "".join(f"{b}" + "\tNA" * 8 + "\n" for b in range(3)))
    records, used = cohort_mod.correlation_host(zero, small, np.array([[1.0], [2.0]]))
    assert cohort_mod.format_correlation_tsv(["x y", "q"], [0, 0], ["pH"], records, used) == (
        "# epik_amd correlation v1  samples=2 used=0 columns=1\n# unused\tx y\n# unused\tq\n# column\t0\tpH\t0\n"
        "edge_num\tcolumn\tmass_pearson\tmass_spearman\timbalance_pearson\timbalance_spearman\n" +
        "".join(f"{b}\tpH" + "\tNA" * 4 + "\n" for b in range(3)))


@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_drivers_refuse_the_flags_without_cohort_and_read_the_metadata_first(host_bins, tmp_path, binary):
    out = tmp_path / "out"
    out.mkdir()
    base = [os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "none.list"), "-o", str(out)]
    for extra, flag in ((["--cohort-correlation", "meta.tsv"], "--cohort-correlation"), (["--cohort-dispersion"], "--cohort-dispersion"),
                        (["--cohort-correlation", "meta.tsv", "--cohort-dispersion", "--cohort-alpha"], "--cohort-")):
        run = subprocess.run(base + extra, capture_output=True, text=True)
        assert run.returncode == 255, run.stdout + run.stderr
        assert run.stderr.startswith("Error:") and flag in run.stderr and "--cohort " in run.stderr, (extra, run.stderr)
        assert "Loading database" not in run.stdout and "HIP device" not in run.stderr and not list(out.iterdir())
    shown = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert shown.returncode == 0 and "--cohort-correlation arg" in shown.stdout and "--cohort-dispersion " in shown.stdout
    assert "cohort_correlation_<list>.tsv" in shown.stdout and "cohort_dispersion_<list>.tsv" in shown.stdout
    # the metadata is read, and its errors named, before the database is opened (there is none)
    for name in "abc":
        (tmp_path / f"{name}.fasta").write_text(">r\nACGT\n")
    (tmp_path / "samples.list").write_text("a\ta.fasta\nb\tb.fasta\nc\tc.fasta\n")
    base[4] = str(tmp_path / "samples.list")
    head = "sample\tpH\tdepth\n"
    for text, words in ((head + "a\t1\t2\nb\t1\tx\nc\t1\t2\n", ("line 3", "column depth", "'x'")),
                        (head + "a\t1\t2\nb\t1\t1e999\nc\t1\t2\n", ("line 3", "column depth", "overflows")),
                        (head + "a\t1\t2\nb\tinf\t1\nc\t1\t2\n", ("line 3", "column pH", "'inf'")),
                        (head + "a\t1\t2\nb\t1\nc\t1\t2\n", ("line 3", "2 fields, not 3")),
                        (head + "a\t1\t2\nb\t1\t2\na\t3\t4\nc\t1\t2\n", ("line 4", "'a'", "twice")),
                        (head + "a\t1\t2\nb\t1\t2\n", ("no line", "'c'")),
                        ("sample\tpH\tpH\n", ("line 1", "'pH'", "twice")),
                        (None, ("cannot open",))):
        if text is not None:
            (tmp_path / "meta.tsv").write_text(text)
        else:
            os.remove(tmp_path / "meta.tsv")
        run = subprocess.run(base + ["--cohort", "--cohort-correlation", str(tmp_path / "meta.tsv")], capture_output=True, text=True)
        assert run.returncode == 255 and run.stderr.startswith("Error:") and "--cohort-correlation" in run.stderr, run.stderr
        assert all(w in run.stderr for w in words), (text, run.stderr)
        assert "Loading database" not in run.stdout and "HIP device" not in run.stderr and not list(out.iterdir())
    # a good file passes on to the device and the database (there is none); the skipped lines are counted
    (tmp_path / "meta.tsv").write_text(GOOD_METADATA)
    run = subprocess.run(base + ["--cohort", "--cohort-correlation", str(tmp_path / "meta.tsv"), "--cohort-dispersion"],
                         capture_output=True, text=True)
    assert run.returncode == 255 and "--cohort-correlation" not in run.stderr and "meta.tsv" not in run.stderr, run.stderr
    assert "3 columns, 1 lines of samples that are not in the list skipped" in run.stdout


def test_launcher_passes_the_flags_only_when_given():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw)
    assert "--cohort-correlation" not in " ".join(default) and "--cohort-dispersion" not in " ".join(default)
    assert epik.driver_command(**kw, cohort_correlation=None, cohort_dispersion=False) == default
    assert "--cohort-correlation" not in " ".join(epik.driver_command(**kw, cohort=True))
    assert "--cohort-dispersion" not in " ".join(epik.driver_command(**kw, cohort=True))
    assert epik.driver_command(**kw, cohort=True, cohort_dispersion=True)[:-1] == default[:-1] + ["--cohort", "--cohort-dispersion"]
    assert epik.driver_command(**kw, cohort=True, cohort_correlation="m.tsv")[:-1] == \
        default[:-1] + ["--cohort", "--cohort-correlation", "m.tsv"]
    assert epik.driver_command(**kw, cohort=True, cohort_squash=True, cohort_epca=True, cohort_kmeans=2, cohort_alpha=True,
                               cohort_correlation="m.tsv", cohort_dispersion=True, taxonomy="t.tsv", strand="both")[:-1] == \
        default[:-1] + ["--strand", "both", "--cohort", "--cohort-squash", "--cohort-epca", "--cohort-kmeans", "2", "--cohort-alpha",
                        "--cohort-correlation", "m.tsv", "--cohort-dispersion", "--taxonomy", "t.tsv"]
    for bad in (dict(cohort_correlation="m.tsv"), dict(cohort_dispersion=True)):
        with pytest.raises(click.UsageError):
            epik.driver_command(**kw, **bad)
    me = os.path.join(ROOT, "epik.py")
    out = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort-correlation" in out.stdout and "--cohort-dispersion" in out.stdout
    for flags in (["--cohort-correlation", me], ["--cohort-dispersion"]):
        run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, *flags, me], capture_output=True, text=True)
        assert run.returncode == 2 and "--cohort" in run.stderr and flags[0] in run.stderr, (run.stdout, run.stderr)


# ---- 7. the host code stand-alone --------------------------------------------------------------------------------------
def _cells_input(path, cells, first):
    with open(path, "wb") as fh:
        fh.write(np.array(cells.shape, dtype="<u8").tobytes() + np.ascontiguousarray(cells, U64).tobytes() +
                 np.ascontiguousarray(first, np.uint32).tobytes() + np.zeros(len(first)).tobytes())


@pytest.mark.parametrize("sanitized", [False, True])
def test_host_test_binary_correlation_and_dispersion_are_the_library_s(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    cases = [cohort_input("tree15", 7)[:3], cohort_input("tree2999", 3)[:3], cohort_input("tree2999", 7)[:3]]
    for name, (mass, parent) in forged_correlation_cohorts().items():
        cases.append((mass, numpy_first(parent), forged_metadata(name, mass)))
    wide = np.random.default_rng(3).normal(size=(7, 64))
    wide[np.random.default_rng(4).random(wide.shape) < 0.2] = np.nan
    cases.append(cohort_input("tree15", 7)[:2] + (wide,))
    for i, (mass, first, meta) in enumerate(cases):
        _cells_input(tmp_path / "mass.bin", mass, first)
        (tmp_path / "meta.bin").write_bytes(np.ascontiguousarray(meta, np.float64).tobytes())
        run = subprocess.run([binary, "correlation", str(tmp_path / "out.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "meta.bin")],
                             capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (i, run.stderr)
        records, used = cohort_mod.correlation_host(mass, first, meta)
        assert (tmp_path / "out.bin").read_bytes() == records.tobytes() + used.tobytes(), i
        run = subprocess.run([binary, "dispersion", str(tmp_path / "out.bin"), str(tmp_path / "mass.bin")], capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (i, run.stderr)
        assert (tmp_path / "out.bin").read_bytes() == cohort_mod.dispersion_host(mass, first).tobytes(), i
    bad = np.zeros((len(cases[-1][0]), 2))
    bad[1, 1] = np.inf
    (tmp_path / "meta.bin").write_bytes(bad.tobytes())
    run = subprocess.run([binary, "correlation", str(tmp_path / "o.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "meta.bin")],
                         capture_output=True, text=True)
    assert run.returncode == 1 and "infinite" in run.stderr
    (tmp_path / "meta.bin").write_bytes(b"\0" * 12)
    run = subprocess.run([binary, "correlation", str(tmp_path / "o.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "meta.bin")],
                         capture_output=True, text=True)
    assert run.returncode == 1 and "float64 [S][M]" in run.stderr
