"""The edge model (a sequential linear model per branch, by permutation, with the max-statistic adjustment) on the host
(epik_amd/host/cohort.cpp: edgemodel_records), without a GPU: the case derived by hand; the rule restated in numpy (a Python loop
over the positions, vectorised over columns, permutations, families and branches) against the host mirror bit for bit, every
record, the info block, the aliased bytes, every stat and every max; one defined branch; the siblings (the edge test, the edge
correlation, the sequential model's design); the observed sums against least squares in decimal arithmetic; the permutation
share against all 720 orders of six positions; the symbols and their refusals; the stand-alone host binary, plain and under the
sanitizers.
"""
import decimal
import itertools
import os
import subprocess

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod
from test_cohort_cpu import host_bins, numpy_first, random_cells, same_bits  # noqa: F401 (host_bins: a fixture)
from test_edgetest_cpu import edge_tree, numpy_vectors
from test_model_cpu import decimal_solve, design, designs_of, numpy_arrangements
from test_permanova_cpu import _cells_input
from test_strata_cpu import numpy_sigma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U64 = np.uint64
MISSING = capi.MODEL_MISSING
NA = float(np.uint64(capi.NA_BITS).view(np.float64))
DOUBLES = ("ss", "r2", "partial_r2", "f", "p", "p_adj")
COUNTS = ("at_least", "max_at_least", "sign", "pad")


# ---- the rule restated ------------------------------------------------------------------------------------------------------
def numpy_basis(totals, kind, labels, values):
    """Steps 1, 3 and 4 of the sequential model's rule: (used, basis [R][L], df [T], columns [T], aliased [64], C)."""
    kind, labels, values = np.asarray(kind), np.asarray(labels), np.asarray(values, dtype=np.float64)
    terms = labels.shape[1]
    present = np.where(kind[None, :] != 0, ~np.isnan(values), labels != MISSING)
    used = np.flatnonzero((np.asarray(totals) != 0) & present.all(axis=1))
    n = len(used)
    basis, df, columns, aliased, count = [], [0] * terms, [0] * terms, np.zeros(capi.MODEL_MAX_COLUMNS, dtype=np.uint8), 0
    for t in range(terms):
        if kind[t]:
            raw = [values[used, t].copy()]
        else:
            number = {}
            lam = np.array([number.setdefault(int(v), len(number)) for v in labels[used, t]], dtype=np.int64)
            raw = [(lam == g).astype(np.float64) for g in range(1, len(number))]
        for v in raw:
            columns[t] += 1
            n0 = 0.0
            if n:
                acc = 0.0
                for i in range(n):
                    acc = acc + v[i]
                v = v - acc / float(n)
                for i in range(n):
                    n0 = n0 + v[i] * v[i]
            accepted = np.array(basis).reshape(len(basis), n)
            for _ in range(2):
                h = np.zeros(len(basis))
                for i in range(n):
                    h = h + accepted[:, i] * v[i]
                for k in range(len(basis)):
                    v = v - h[k] * accepted[k]
            n1 = 0.0
            for i in range(n):
                n1 = n1 + v[i] * v[i]
            if n0 > 0.0 and n1 > 2.0 ** -40 * n0:
                basis.append(v / np.sqrt(n1))
                df[t] += 1
            else:
                aliased[count] = 1
            count += 1
    return used, np.array(basis).reshape(len(basis), n), df, columns, aliased, count


def numpy_edgemodel(mass, first, kind, labels, values, permutations, seed, strata=None):
    """`cohort_mod.Edgemodel` by the rule."""
    mass = np.asarray(mass, dtype=U64)
    n_branches, terms, row = mass.shape[1], np.asarray(labels).shape[1], permutations + 1
    xm, xi, inner, total = numpy_vectors(mass, first)
    used, basis, df, columns, aliased, count = numpy_basis(total, kind, labels, values)
    n, rank = len(used), len(basis)
    df_res = n - 1 - rank
    info = np.zeros(1, dtype=capi.EDGEMODEL_INFO)
    info["used"], info["terms"], info["columns"], info["rank"], info["df_res"] = n, terms, count, rank, df_res
    info["df"][0, :terms], info["term_columns"][0, :terms] = df, columns
    records = np.zeros((terms, n_branches), dtype=capi.EDGEMODEL)
    for f in DOUBLES:
        records["family"][f] = NA
    stat, most = np.full((terms, 2, n_branches, row), NA), np.full((terms, 2, row), NA)
    result = cohort_mod.Edgemodel(records, info[0], stat, most, aliased)
    if df_res < 1 or rank == 0:
        return result
    x = np.stack([xm[used], xi[used]])                                          # [2][L][N]
    acc = np.zeros((2, n_branches))
    for i in range(n):
        acc = acc + x[:, i, :]
    d = x - (acc / float(n))[:, None, :]
    sxx = np.zeros((2, n_branches))
    for i in range(n):
        sxx = sxx + d[:, i, :] * d[:, i, :]
    defined = (sxx > 0.0) & (inner[None, :] | (np.arange(2) == 0)[:, None])     # [2][N]
    sigma = numpy_arrangements(n, seed, permutations) if strata is None else numpy_sigma(np.asarray(strata)[used], seed, permutations)
    moved = basis[:, sigma]                                                     # [R][P + 1][L]: q_c[sigma_p(i)]
    s = np.zeros((rank, row, 2, n_branches))
    for i in range(n):
        s = s + moved[:, :, i][:, :, None, None] * d[None, None, :, i, :]
    ss, model, at = [], np.zeros((row, 2, n_branches)), 0
    for t in range(terms):
        term = np.zeros((row, 2, n_branches))
        for _ in range(df[t]):
            term = term + s[at] * s[at]
            at += 1
        ss.append(term)
        model = model + term
    res = sxx[None] - model
    at = 0
    for t in range(terms):
        if df[t]:
            with np.errstate(invalid="ignore", divide="ignore"):
                phi = np.where(res > 0.0, ss[t] / (ss[t] + res), np.where(ss[t] > 0.0, 1.0, 0.0))    # [P + 1][2][N]
                f_stat = (ss[t][0] / float(df[t])) / (res[0] / float(df_res))
            for f in range(2):
                live = defined[f]
                if not live.any():
                    continue
                mmax = phi[:, f, live].max(axis=1)
                most[t, f] = mmax
                stat[t, f, live, :] = phi[:, f, live].T
                fam = records["family"][t, :, f]
                fam["ss"][live] = ss[t][0, f, live]
                fam["r2"][live] = ss[t][0, f, live] / sxx[f, live]
                fam["partial_r2"][live] = phi[0, f, live]
                fam["f"][live] = np.where(res[0, f, live] > 0.0, f_stat[f, live], NA)
                if df[t] == 1:
                    fam["sign"][live] = np.sign(s[at, 0, f, live]).astype(np.int32)
                at_least = (phi[1:, f, :] >= phi[0, f][None, :]).sum(axis=0)
                max_at_least = (mmax[1:, None] >= phi[0, f][None, :]).sum(axis=0)
                fam["at_least"][live], fam["max_at_least"][live] = at_least[live], max_at_least[live]
                fam["p"][live] = (1 + at_least[live]).astype(np.float64) / float(permutations + 1)
                fam["p_adj"][live] = (1 + max_at_least[live]).astype(np.float64) / float(permutations + 1)
                records["family"][t, :, f] = fam
        at += df[t]
    return result


def only_na_or_numbers(result):
    """No arithmetic NaN reaches an output: a NaN is the NA pattern."""
    arrays = [result.records["family"][f] for f in DOUBLES] + [v for v in (result.stat, result.max) if v is not None]
    for v in arrays:
        v = np.ascontiguousarray(v)
        assert (v.view(U64)[np.isnan(v)] == U64(capi.NA_BITS)).all()
        assert not np.isinf(v).any()


def same_edgemodel(got, want, what=""):
    for f in COUNTS:
        a, b = got.records["family"][f], want.records["family"][f]
        assert np.array_equal(a, b), (what, f, np.argwhere(a != b)[:8])
    for f in DOUBLES:
        a, b = np.ascontiguousarray(got.records["family"][f]), np.ascontiguousarray(want.records["family"][f])
        assert same_bits(a, b), (what, f, np.argwhere(a.view(U64) != b.view(U64))[:8])
    assert got.info.tobytes() == want.info.tobytes(), (what, got.info, want.info)
    assert np.array_equal(got.aliased, want.aliased), (what, got.aliased, want.aliased)
    for name in ("stat", "max"):
        a, b = getattr(got, name), getattr(want, name)
        if a is not None and b is not None:
            assert same_bits(a, b), (what, name, np.argwhere(a.view(U64) != b.view(U64))[:8])
    only_na_or_numbers(got)
    return True


def family(result, t, f):
    return result.records["family"][t, :, f]


# ---- 1. by hand -------------------------------------------------------------------------------------------------------------
HAND_PARENT = np.array([2, 2, -1])
HAND_MASS = np.array([[0, 0, 4], [0, 2, 2], [2, 0, 2], [2, 2, 0]], dtype=U64)


def test_three_branches_four_samples_by_hand():
    """The model's by-hand case carried to a branch: the factor (a, a, b, b), then the covariate (0, 1, 2, 3), so q_0 = (-1/2,
    -1/2, 1/2, 1/2) and q_1 = (-1/2, 1/2, -1/2, 1/2).  The shares of all branches of a sample sum to one, so two branches cannot
    both have deviations of +-1/2 in these two patterns (the samples' shares would reach 2); the deviations are +-1/4 instead.
    Every total is 4.  Leaf 0 has the shares (0, 0, 1/2, 1/2): d = q_0 / 2, sxx = 1/4, s_0 = 1/2, s_1 = 0: SS = 1/4 and 0,
    SS_res = 0: r2 = 1 and 0, the partial R2 1 and +0.0 (the guard), f NA, sign +1 and 0.  Leaf 1 has (0, 1/2, 0, 1/2):
    d = q_1 / 2, the same with the terms exchanged.  The root keeps (1, 1/2, 1/2, 0): d = (1/2, 0, 0, -1/2), sxx = 1/2,
    s_0 = s_1 = -1/2: SS = 1/4 and 1/4, SS_res = 0, r2 = 1/2 twice, the partial R2 1 twice, sign -1; its imbalance is
    (0, 1/2, 1/2, 1) - 1 + 1: the same numbers with sign +1.  The leaves have no imbalance: NA.  The factor alone on the root:
    SS_res = 1/4, the partial R2 1/2, f = (1/4 / 1) / (1/4 / 2) = 2.  Every number is exact in binary."""
    first = numpy_first(HAND_PARENT)
    both = design(("f", [5, 5, 2, 2]), ("n", [0.0, 1.0, 2.0, 3.0]))
    got = cohort_mod.edgemodel_host(HAND_MASS, first, *both, permutations=50, seed=3)
    assert tuple(got.info)[:5] == (4, 2, 2, 2, 1) and list(got.info["df"][:3]) == [1, 1, 0] and not got.aliased.any()
    for f, want in (("ss", [[0.25, 0.0, 0.25], [0.0, 0.25, 0.25]]), ("r2", [[1.0, 0.0, 0.5], [0.0, 1.0, 0.5]]),
                    ("partial_r2", [[1.0, 0.0, 1.0], [0.0, 1.0, 1.0]]), ("f", [[NA] * 3] * 2)):
        assert same_bits(np.ascontiguousarray(got.records["family"][f][:, :, 0]), np.array(want)), f
    assert got.records["family"]["sign"][:, :, 0].tolist() == [[1, 0, -1], [0, 1, -1]]
    imbalance = got.records["family"][:, :, 1]
    for f in DOUBLES:
        assert same_bits(np.ascontiguousarray(imbalance[f][:, :2]), np.full((2, 2), NA)), f      # the leaves
    assert same_bits(np.ascontiguousarray(imbalance["ss"][:, 2]), [0.25, 0.25]) and imbalance["sign"][:, 2].tolist() == [1, 1]
    assert same_bits(np.ascontiguousarray(imbalance["partial_r2"][:, 2]), [1.0, 1.0]) and not imbalance["sign"][:, :2].any()
    same_edgemodel(got, numpy_edgemodel(HAND_MASS, first, *both, 50, 3), "by hand")
    alone = cohort_mod.edgemodel_host(HAND_MASS, first, *design(("f", [5, 5, 2, 2])), permutations=50, seed=3)
    root = family(alone, 0, 0)[2]
    assert alone.info["df_res"] == 2 and same_bits(root["ss"], 0.25) and same_bits(root["partial_r2"], 0.5) and same_bits(root["f"], 2.0)
    assert same_bits(root["r2"], 0.5) and root["sign"] == -1
    same_edgemodel(alone, numpy_edgemodel(HAND_MASS, first, *design(("f", [5, 5, 2, 2])), 50, 3), "the factor alone")


# ---- 2. the host mirror against the restatement -------------------------------------------------------------------------------
def special_cells(rng, num_samples, num_branches):
    """One sample without mass (L = num_samples); branch 1 without mass anywhere; branch 3 with mass in one sample only."""
    mass = random_cells(rng, num_samples + 1, num_branches, empty=1, bits=42)
    mass[:, 1] = 0
    mass[:, 3] = 0
    mass[int(np.flatnonzero(mass.sum(axis=1))[0]), 3] = 5
    return mass


@pytest.mark.parametrize("num_samples", (2, 3, 5, 33, 65))
def test_host_mirror_equals_the_numpy_restatement_bit_for_bit(num_samples):
    parent, first = edge_tree(7)
    rng = np.random.default_rng(2800 + num_samples)
    mass = special_cells(rng, num_samples, len(parent))
    seen = {}
    for at, (name, (kind, labels, values)) in enumerate(designs_of(rng, num_samples + 1).items()):
        permutations, seed = (1, 63, 64, 65)[at % 4], int(rng.integers(0, 1 << 63))
        want = numpy_edgemodel(mass, first, kind, labels, values, permutations, seed)
        got = cohort_mod.edgemodel_host(mass, first, kind, labels, values, permutations, seed)
        same_edgemodel(got, want, (num_samples, name))
        lean = cohort_mod.edgemodel_host(mass, first, kind, labels, values, permutations, seed, with_stat=False, with_max=False)
        assert lean.stat is None and lean.max is None and lean.records.tobytes() == got.records.tobytes()
        seen[name] = got
        # the design's half is the sequential model's, byte for byte
        bl = np.ones(len(parent))
        model = cohort_mod.model_host(mass, first, bl, kind, labels, values, 1, seed)
        assert got.info.tobytes()[:24] == model.info.tobytes()[:24] and np.array_equal(got.aliased, model.aliased), name
        terms = len(kind)
        assert np.array_equal(got.info["df"][:terms], model.records["df"][:terms]), name
        assert np.array_equal(got.info["term_columns"][:terms], model.records["columns"][:terms]), name
        assert not got.info["df"][terms:].any() and not got.info["term_columns"][terms:].any()
    assert seen["a term missing everywhere"].info["used"] == 0
    assert np.isnan(seen["a term missing everywhere"].records["family"]["ss"]).all()
    assert seen["a covariate given twice"].info["df"][2] == 0 and np.isnan(family(seen["a covariate given twice"], 2, 0)["ss"]).all()
    assert seen["a constant column"].aliased[0] == 1 and np.isnan(family(seen["a constant column"], 0, 0)["ss"]).all()
    full = seen["rank L - 1"]
    if num_samples <= 33:
        assert full.info["df_res"] <= 0 and np.isnan(full.records["family"]["ss"]).all() and np.isnan(full.max).all()
    lone = seen["a lone covariate"]
    if lone.info["df_res"] >= 1:
        mass_family = family(lone, 0, 0)
        assert np.isnan(mass_family["ss"][1]) and mass_family["at_least"][1] == 0          # no mass anywhere: sxx = 0
        assert not np.isnan(mass_family["ss"][3]) and not np.isnan(mass_family["ss"][0])
        inner = first < np.arange(len(parent))
        assert np.isnan(family(lone, 0, 1)["ss"][~inner]).all()


def test_the_guard_of_a_residual_that_is_not_positive():
    """A branch with mass in one sample, and that sample a group of its own: the factor explains the branch's share entirely,
    SS_res is not > 0, and phi is 1.0 where the term has a sum and +0.0 where it has none, in every permutation."""
    parent, first = edge_tree(7)
    rng = np.random.default_rng(77)
    mass = random_cells(rng, 9, len(parent), bits=42)
    mass[:, 0] = 0
    mass[4, 0] = 1 << 30
    groups = np.array([0, 0, 1, 1, 2, 0, 1, 0, 1], dtype=np.uint32)
    terms = design(("f", groups), ("n", rng.normal(size=9)))
    got = cohort_mod.edgemodel_host(mass, first, *terms, permutations=65, seed=5)
    same_edgemodel(got, numpy_edgemodel(mass, first, *terms, 65, 5), "a singleton group")
    factor, covariate = family(got, 0, 0)[0], family(got, 1, 0)[0]
    assert abs(factor["r2"] - 1.0) < 1e-12 and factor["partial_r2"] > 0.999     # (the residual is zero but for the rounding of Q)
    observed = got.stat[:, 0, 0, 0]
    assert ((got.stat[:, 0, 0, :] >= 0.0) & (got.stat[:, 0, 0, :] <= 1.0)).all() and same_bits(observed[0], factor["partial_r2"])
    assert same_bits(observed[1], covariate["partial_r2"])


def test_identical_samples_have_no_defined_branch():
    parent, first = edge_tree(7)
    mass = np.tile(np.array([[8, 8, 16, 8, 8, 8, 8]], dtype=U64), (6, 1))      # every share a power of two: the deviations are zero
    terms = design(("f", [0, 1, 0, 1, 0, 1]), ("n", [1.0, 2.0, 4.0, 8.0, 16.0, 3.0]))
    got = cohort_mod.edgemodel_host(mass, first, *terms, permutations=9, seed=1)
    assert tuple(got.info)[:5] == (6, 2, 2, 2, 3)
    for f in DOUBLES:
        assert np.isnan(got.records["family"][f]).all(), f
    assert not got.records["family"]["at_least"].any() and np.isnan(got.stat).all() and np.isnan(got.max).all()
    same_edgemodel(got, numpy_edgemodel(mass, first, *terms, 9, 1))


@pytest.mark.parametrize("num_samples", (5, 33, 65))
def test_strata_host_mirror_equals_the_restatement(num_samples):
    """Three strata of unequal size and a singleton; None gives the bytes of the entry without strata."""
    parent, first = edge_tree(7)
    rng = np.random.default_rng(2900 + num_samples)
    mass = special_cells(rng, num_samples, len(parent))
    s = num_samples + 1
    strata = np.where(np.arange(s) == 2, 900, np.minimum(np.arange(s) * 7 // s, 2) * 4000000000 // 3).astype(np.uint32)
    assert len(set(strata.tolist())) == 4 or s < 8
    for name in ("a lone covariate", "factor, covariate", "a covariate given twice"):
        kind, labels, values = designs_of(rng, s)[name]
        seed = int(rng.integers(0, 1 << 63))
        got = cohort_mod.edgemodel_host(mass, first, kind, labels, values, 65, seed, strata=strata)
        same_edgemodel(got, numpy_edgemodel(mass, first, kind, labels, values, 65, seed, strata=strata), (num_samples, name))
        plain = cohort_mod.edgemodel_host(mass, first, kind, labels, values, 65, seed)
        one = cohort_mod.edgemodel_host(mass, first, kind, labels, values, 65, seed, strata=np.full(s, 12345, dtype=np.uint32))
        assert one.records.tobytes() == plain.records.tobytes() and one.stat.tobytes() == plain.stat.tobytes()
        if num_samples >= 33 and got.info["df_res"] >= 1:
            assert got.stat.tobytes() != plain.stat.tobytes()
            for t in range(len(kind)):                                           # the observed half does not know the strata
                for f in ("ss", "r2", "partial_r2", "f", "sign"):
                    a, b = np.ascontiguousarray(got.records["family"][f][t]), np.ascontiguousarray(plain.records["family"][f][t])
                    assert a.tobytes() == b.tobytes(), (name, t, f)


# ---- 3. one defined branch ----------------------------------------------------------------------------------------------------
def test_with_one_defined_branch_the_adjusted_p_is_the_plain_one():
    first = numpy_first(HAND_PARENT)
    rng = np.random.default_rng(31)
    mass = np.zeros((12, 3), dtype=U64)
    mass[:, 0] = rng.integers(1, 1 << 20, size=12)                              # all mass on leaf 0 but for ...
    mass[:, 2] = (1 << 22) - mass[:, 0]                                         # ... the root: shares that sum to one, exactly
    mass[:, 1] = 0
    terms = design(("n", rng.normal(size=12)), ("f", np.arange(12) % 3))
    got = cohort_mod.edgemodel_host(mass, first, *terms, permutations=199, seed=8)
    same_edgemodel(got, numpy_edgemodel(mass, first, *terms, 199, 8))
    # (the shares of a sample sum to one, so where one branch varies another does: the mass family never has one defined branch)
    for t in range(2):
        fam = family(got, t, 0)
        assert np.isnan(fam["p"][1]) and not np.isnan(fam["p"][[0, 2]]).any() and (fam["p_adj"][[0, 2]] >= fam["p"][[0, 2]]).all()
        # the imbalance family: the root alone is inner
        alone = family(got, t, 1)
        assert np.isnan(alone["p"][:2]).all() and same_bits(alone["p_adj"][2], alone["p"][2]) and not np.isnan(alone["p"][2])
        assert same_bits(got.max[t, 1], got.stat[t, 1, 2])


# ---- 4. the siblings ------------------------------------------------------------------------------------------------------------
#: the worst relative deviation between the edge model's host mirror and its siblings' over the cases below, measured on the
#: CPU, and the bound, 16 times that: the same numbers by different sums
SIBLING_WORST = 4.3e-14
SIBLING_BOUND = 16 * SIBLING_WORST


@pytest.mark.parametrize("num_samples", (6, 12, 40))
def test_a_lone_factor_is_the_edge_test_and_a_lone_covariate_the_edge_correlation(num_samples):
    parent, first = edge_tree(7)
    worst = 0.0
    for trial in range(4):
        rng = np.random.default_rng(3400 + 10 * num_samples + trial)
        mass = random_cells(rng, num_samples, len(parent), empty=trial % 2, bits=42)
        groups = rng.permutation(np.arange(num_samples) % (2 + trial % 2)).astype(np.uint32)
        factor = design(("f", groups))
        model = cohort_mod.edgemodel_host(mass, first, *factor, permutations=9, seed=trial)
        edge = cohort_mod.edgetest_host(mass, first, factor[1], permutations=9, seed=trial).records[0]
        x = rng.normal(size=num_samples)
        covariate = design(("n", x))
        lone = cohort_mod.edgemodel_host(mass, first, *covariate, permutations=9, seed=trial)
        correlation, _ = cohort_mod.correlation_host(mass, first, x[:, None])
        for f, theirs, name in ((0, 0, "mass_pearson"), (1, 2, "imbalance_pearson")):
            ours, fam = family(model, 0, f), edge["family"][:, theirs]
            live = ~np.isnan(fam["eta2"])
            assert np.array_equal(live, ~np.isnan(ours["r2"])), (num_samples, trial, f)
            pairs = [(ours["r2"][live], fam["eta2"][live])]
            both = live & ~np.isnan(fam["stat"]) & ~np.isnan(ours["f"])
            pairs.append((ours["f"][both], fam["stat"][both]))
            r = correlation[name][0]
            ours = family(lone, 0, f)
            live = ~np.isnan(r) & ~np.isnan(ours["r2"])
            assert live.any()
            pairs.append((ours["r2"][live], r[live] * r[live]))
            clear = live & (np.abs(r) > 1e-9)
            assert np.array_equal(ours["sign"][clear], np.sign(r[clear]).astype(np.int32)), (num_samples, trial, f)
            for got, want in pairs:
                deviation = float(np.max(np.abs(got - want) / np.abs(want), initial=0.0))
                worst = max(worst, deviation)
                assert deviation <= SIBLING_BOUND, (num_samples, trial, f, deviation)
    print(f"the siblings, S = {num_samples}: worst relative deviation {worst:.3e}")


# ---- 5. the textbook form -------------------------------------------------------------------------------------------------------
#: the worst relative deviation of the observed SS and F of the later term from least squares in 60-digit decimal arithmetic over
#: the cases below, measured on the CPU, and the bound, 16 times that
TEXTBOOK_WORST = 5.4e-15
TEXTBOOK_BOUND = 16 * TEXTBOOK_WORST


def decimal_rss(columns, y):
    """The residual sum of squares of y on the columns (the intercept among them), by the normal equations in Decimal."""
    n, p = len(y), len(columns)
    xtx = [[sum(columns[a][i] * columns[b][i] for i in range(n)) for b in range(p)] for a in range(p)]
    beta = decimal_solve(xtx, [sum(columns[a][i] * y[i] for i in range(n)) for a in range(p)])
    return sum((y[i] - sum(beta[a] * columns[a][i] for a in range(p))) ** 2 for i in range(n))


def test_observed_sums_are_least_squares_in_decimal():
    D = decimal.Decimal
    parent, first = edge_tree(7)
    worst = 0.0
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        for num_samples in (7, 12, 19):
            rng = np.random.default_rng(4500 + num_samples)
            mass = random_cells(rng, num_samples, len(parent), bits=42)
            mass[:, 0] |= U64(1)
            groups = (np.arange(num_samples) % 3).astype(np.uint32)
            x = rng.normal(size=num_samples)
            got = cohort_mod.edgemodel_host(mass, first, *design(("f", groups), ("n", x)), permutations=1, seed=1)
            assert not got.aliased.any() and list(got.info["df"][:2]) == [2, 1]
            xm, xi, inner, _ = numpy_vectors(mass, first)
            one = [D(1)] * num_samples
            before = [one, [D(int(g == 1)) for g in groups], [D(int(g == 2)) for g in groups]]
            full = before + [[D(float(v)) for v in x]]
            for b in range(len(parent)):
                for f, vector in ((0, xm), (1, xi)):
                    if f == 1 and not inner[b]:
                        continue
                    y = [D(float(v)) for v in vector[:, b]]
                    rss_before, rss = decimal_rss(before, y), decimal_rss(full, y)
                    ss = rss_before - rss
                    want_f = (ss / 1) / (rss / int(got.info["df_res"]))
                    fam = family(got, 1, f)[b]
                    for got_value, want in ((fam["ss"], ss), (fam["f"], want_f)):
                        deviation = float(abs(D(float(got_value)) - want) / abs(want))
                        worst = max(worst, deviation)
                        assert deviation <= TEXTBOOK_BOUND, (num_samples, b, f, got_value, want, deviation)
    print(f"least squares in decimal: worst relative deviation {worst:.3e}")


# ---- 6. the permutations -------------------------------------------------------------------------------------------------------
def test_the_share_of_permutations_at_least_the_observed_follows_all_720_orders():
    first = numpy_first(HAND_PARENT)
    rng = np.random.default_rng(6)
    mass = np.array([[10, 3, 7], [4, 9, 7], [12, 1, 7], [2, 2, 16], [8, 8, 4], [15, 2, 3]], dtype=U64)
    kind, labels, values = design(("n", [0.1, 0.5, 0.2, 0.9, 0.6, 1.4]))
    phi0 = family(cohort_mod.edgemodel_host(mass, first, kind, labels, values, permutations=1, seed=1), 0, 0)["partial_r2"][0]
    # every order of the rows of Q is an order of the covariate: the exact share
    exact = 0
    for order in itertools.permutations(range(6)):
        moved = design(("n", np.asarray(values[:, 0])[list(order)]))
        exact += family(cohort_mod.edgemodel_host(mass, first, *moved, permutations=1, seed=1), 0, 0)["partial_r2"][0] >= phi0 * (1 - 1e-12)
    share = exact / 720.0
    at_least = total = 0
    for seed in rng.integers(0, 1 << 62, size=40):
        got = cohort_mod.edgemodel_host(mass, first, kind, labels, values, permutations=500, seed=int(seed), with_stat=False)
        at_least, total = at_least + int(family(got, 0, 0)["at_least"][0]), total + 500
    sd = (share * (1 - share) / total) ** 0.5
    assert abs(at_least / total - share) <= 5 * sd, (at_least / total, share, sd)


# ---- 7. the symbols --------------------------------------------------------------------------------------------------------------
def test_edgemodel_symbols_exist_and_refuse_what_the_header_says():
    lib = capi.load()
    for name in ("epik_amd_cohort_edgemodel_device", "epik_amd_cohort_edgemodel", "epik_amd_cohort_edgemodel_host",
                 "epik_amd_cohort_edgemodel_strata_device", "epik_amd_cohort_edgemodel_strata", "epik_amd_cohort_edgemodel_strata_host"):
        assert hasattr(lib, name) and name in capi.EXPORTS, name
    assert capi.EDGEMODEL_FAMILY.itemsize == 72 and capi.EDGEMODEL.itemsize == 144 and capi.EDGEMODEL_INFO.itemsize == 152
    err = lambda: lib.epik_amd_last_error().decode()
    parent, first = edge_tree(7)
    first = np.ascontiguousarray(first, dtype=np.uint32)
    mass = random_cells(np.random.default_rng(1), 40, 7, bits=30)
    kind, labels, values = design(("f", np.arange(40) % 3), ("n", np.arange(40.0) ** 2))
    out, info = np.zeros((16, 7), dtype=capi.EDGEMODEL), np.zeros(1, dtype=capi.EDGEMODEL_INFO)
    stat, most, aliased = np.zeros((16, 2, 7, 10)), np.zeros((16, 2, 10)), np.zeros(64, dtype=np.uint8)

    def call(m=mass, fi=first, kd=kind, la=labels, va=values, terms=2, p=9, o=out.ctypes.data, i=info.ctypes.data, a=aliased.ctypes.data):
        m, fi, kd, la, va = (None if v is None else np.ascontiguousarray(v) for v in (m, fi, kd, la, va))
        return lib.epik_amd_cohort_edgemodel_host(*(None if v is None else v.ctypes.data for v in (m,)), 40, 7,
                                                  *(None if v is None else v.ctypes.data for v in (fi, kd, la, va)), terms, p, 5, o, i,
                                                  stat.ctypes.data, most.ctypes.data, a)

    assert call() == capi.OK
    for null in ("m", "fi", "kd", "la", "va", "o", "i", "a"):
        assert call(**{null: None}) == capi.ERR_INVALID and "null argument" in err(), null
    for bad in (0, 17):
        assert call(terms=bad) == capi.ERR_INVALID and "num_terms" in err() and "[1, 16]" in err()
    for bad in (0, 1_000_000):
        assert call(p=bad) == capi.ERR_INVALID and "num_permutations" in err() and "[1, 999999]" in err()
    assert call(kd=np.array([0, 2], dtype=np.uint32)) == capi.ERR_INVALID and "term 1" in err() and "kind 2" in err()
    wrong = labels.copy()
    wrong[17, 0] = 32
    assert call(la=wrong) == capi.ERR_INVALID and "sample 17" in err() and "term 0" in err() and "32" in err()
    wrong = values.copy()
    wrong[23, 1] = -np.inf
    assert call(va=wrong) == capi.ERR_INVALID and "sample 23" in err() and "infinite" in err()
    wide = design(*[("f", (np.arange(40) * (t + 1)) % 23) for t in range(3)])
    assert call(kd=wide[0], la=wide[1], va=wide[2], terms=3) == capi.ERR_INVALID and "66 columns" in err() and "64" in err()
    above = first.copy()
    above[2] = 3
    assert call(fi=above) == capi.ERR_INVALID and "branch 2" in err() and "first[b]" in err()
    before = out.tobytes()
    assert call(p=0) == capi.ERR_INVALID and out.tobytes() == before            # nothing written
    with pytest.raises(ValueError):
        cohort_mod.edgemodel_host(mass, first, kind, labels[:, :1], values, 9, 5)
    # without strata: the bytes of the entry that takes none
    a = cohort_mod.edgemodel_host(mass, first, kind, labels, values, 9, 5)
    assert lib.epik_amd_cohort_edgemodel_strata_host(mass.ctypes.data, 40, 7, first.ctypes.data, kind.ctypes.data, labels.ctypes.data,
                                                     values.ctypes.data, 2, 9, 5, out.ctypes.data, info.ctypes.data, None, None,
                                                     aliased.ctypes.data, None) == capi.OK
    assert out[:2].tobytes() == a.records.tobytes() and info[0].tobytes() == a.info.tobytes()


# ---- 8. the host code stand-alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitized", [False, True])
def test_host_test_binary_edgemodel_is_the_library_s(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    parent, first = edge_tree(7)
    bl = np.ones(len(parent))
    seed = 12345678901234567890
    for num_samples in (2, 5, 33, 65):
        rng = np.random.default_rng(7800 + num_samples)
        mass = special_cells(rng, num_samples - 1, len(parent))
        strata = (np.arange(num_samples) * 3 // num_samples * 1000003).astype(np.uint32)
        (tmp_path / "strata.bin").write_bytes(strata.tobytes())
        _cells_input(tmp_path / "mass.bin", mass, first, bl)
        for name, (kind, labels, values) in designs_of(rng, num_samples).items():
            permutations = int(rng.integers(1, 30))
            (tmp_path / "design.bin").write_bytes(np.array([len(kind)], dtype="<u8").tobytes() + kind.tobytes() + labels.tobytes() +
                                                  values.tobytes())
            for within in (None, strata):
                mode = ["edgemodel"] if within is None else ["edgemodel-strata"]
                files = [str(tmp_path / "out.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "design.bin")]
                files += [] if within is None else [str(tmp_path / "strata.bin")]
                run = subprocess.run([binary] + mode + files + [str(permutations), str(seed)], capture_output=True, text=True)
                assert run.returncode == 0 and not run.stderr, (num_samples, name, run.stderr)
                want = cohort_mod.edgemodel_host(mass, first, kind, labels, values, permutations, seed, strata=within)
                assert (tmp_path / "out.bin").read_bytes() == want.records.tobytes() + want.info.tobytes() + want.stat.tobytes() + \
                    want.max.tobytes() + want.aliased.tobytes(), (num_samples, name, within is not None)
    bad = labels.copy()
    bad[1, 0] = 32
    (tmp_path / "design.bin").write_bytes(np.array([len(kind)], dtype="<u8").tobytes() + kind.tobytes() + bad.tobytes() + values.tobytes())
    run = subprocess.run([binary, "edgemodel", str(tmp_path / "o.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "design.bin"), "9", "1"],
                         capture_output=True, text=True)
    assert run.returncode == 1 and "sample 1" in run.stderr and "32" in run.stderr
