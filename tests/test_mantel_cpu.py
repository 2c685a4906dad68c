"""The Mantel and partial Mantel tests and ANOSIM of a cohort's samples over their distances on the host
(epik_amd/host/cohort.cpp: mantel_records_of_kr, anosim_records_of_kr), without a GPU: the rule restated in numpy (the keys in
uint64 arithmetic, stable argsorts for the arrangements, the triangle chains in Python's order) against the host mirror bit for
bit, every record and every stat[p]; the strata; the textbook forms, which are not shaped like the rule; two cases by hand; the
refusals.

The textbook forms.  The worst relative deviations of the host mirror, measured over TEXTBOOK_CASES: from the exact-rational r
(Fractions of the doubles, rounded once) pearson 1.33e-15 and spearman 1.80e-16; from scipy's pearsonr 2.84e-15 and spearmanr
2.51e-16; the partial statistic from the correlation of the residuals of x and y regressed on z 3.93e-15 (every case has
1 - r_xz^2 >= 0.5); ANOSIM's R from Clarke's form over scipy's rankdata 0 (its sums are exact).  The bounds are 16 times these.
"""
import math
import os
import subprocess
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod
from test_cohort_cpu import host_bins, numpy_first, random_cells, same_bits, tree_case  # noqa: F401 (host_bins: a fixture)
from test_permanova_cpu import _cells_input, numpy_keys  # noqa: F401 (numpy_sigma restates the arrangements on numpy_keys)
from test_strata_cpu import numpy_sigma

U64 = np.uint64
MISSING = capi.PERMANOVA_MISSING
NA = float(np.uint64(capi.NA_BITS).view(np.float64))
MANTEL_DOUBLES = ("r", "r_xz", "r_yz", "stat", "p")
ANOSIM_DOUBLES = ("r", "mean_between", "mean_within", "p")
NONE = capi.MANTEL_NO_CONTROL


# ---- the rule restated ------------------------------------------------------------------------------------------------------
def triangle_chain(a):
    """The rule's triangle chain of a[..., n, n] over the pairs i < j: t_i over j ascending, then the chain of t_0 .. t_{n-2}."""
    n = a.shape[-1]
    t = np.zeros(a.shape[:-1])
    for j in range(n):
        t = np.where(np.arange(n) < j, t + a[..., :, j], t)
    total = np.zeros(a.shape[:-2])
    for i in range(n - 1):
        total = total + t[..., i]
    return total


def midranks_of_pairs(table):
    """The symmetric table of the midranks of the m values above the diagonal among themselves: less + (equal + 1) / 2."""
    n = table.shape[0]
    upper = np.triu_indices(n, 1)
    v = table[upper]
    less = (v[None, :] < v[:, None]).sum(axis=1)
    equal = (v[None, :] == v[:, None]).sum(axis=1)
    ranks = np.zeros_like(table)
    ranks[upper] = less.astype(np.float64) + (equal + 1).astype(np.float64) / 2.0
    return ranks + ranks.T


def centred(table):
    """(the deviations from the chain's mean off the diagonal, ss)."""
    n = table.shape[0]
    dev = np.where(np.eye(n, dtype=bool), 0.0, table - triangle_chain(table) / float(n * (n - 1) // 2))
    return dev, float(triangle_chain(dev * dev))


def partial_statistic(r_xy, r_xz, r_yz):
    """(the rule's partial statistic, whether both radicands are > 0), elementwise."""
    rad_x, rad_y = 1.0 - r_xz * r_xz, 1.0 - r_yz * r_yz
    ok = (rad_x > 0.0) & (rad_y > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        stat = (r_xy - r_xz * r_yz) / (np.sqrt(np.where(ok, rad_x, 1.0)) * np.sqrt(np.where(ok, rad_y, 1.0)))
    return stat, ok


def side_table(q, u, values, matrices):
    """The side's distances over the list u as a symmetric table: only the cells [s][t], s < t, are read."""
    if q < len(values):
        v = values[q][u]
        return np.abs(v[:, None] - v[None, :])
    upper = np.triu(matrices[q - len(values)][np.ix_(u, u)], 1)
    return upper + upper.T


def numpy_mantel(kr, totals, values, matrices, present, methods, control, permutations, seed, strata=None):
    """`cohort_mod.Mantel` by the rule."""
    s = kr.shape[0]
    values = np.zeros((0, s)) if values is None else np.asarray(values, dtype=np.float64)
    matrices = np.zeros((0, s, s)) if matrices is None else np.asarray(matrices, dtype=np.float64)
    present = np.ones(matrices.shape[:2], bool) if present is None else np.asarray(present).astype(bool)
    has = [~np.isnan(v) for v in values] + [p for p in present]
    bits = sum(capi.MANTEL_METHODS[name] for name in methods)
    tests = [(q, method) for q in range(len(has)) for method in (0, 1) if bits >> method & 1]
    records = np.zeros(len(tests), dtype=capi.MANTEL)
    for f in MANTEL_DOUBLES:
        records[f] = NA
    stat = np.full((len(tests), permutations + 1), NA)
    for k, (q, method) in enumerate(tests):
        partial = control is not None and control != q
        keep = (np.asarray(totals) != 0) & has[q] & (has[control] if partial else True)
        u = np.flatnonzero(keep)
        n = len(u)
        records[k]["used"], records[k]["side"], records[k]["method"], records[k]["partial"] = n, q, method, partial
        if n < 3:
            continue
        upper = np.triu(kr[np.ix_(u, u)], 1)
        tables = [upper + upper.T, side_table(q, u, values, matrices)] + ([side_table(control, u, values, matrices)] if partial else [])
        if method == 1:
            tables = [midranks_of_pairs(t) for t in tables]
        (x, ss_x), (y, ss_y) = centred(tables[0]), centred(tables[1])
        z, ss_z = centred(tables[2]) if partial else (None, 1.0)
        if ss_x == 0.0 or ss_y == 0.0 or ss_z == 0.0:
            continue
        sigma = numpy_sigma(np.zeros(n, np.int64) if strata is None else np.asarray(strata)[u], seed, permutations)
        xp = x[sigma[:, :, None], sigma[:, None, :]]                                # x'_p, [P + 1][n][n]; p = 0 is x' itself
        den_xy = np.sqrt(ss_x * ss_y)
        value = triangle_chain(xp * y[None]) / den_xy
        r_xy, counted = float(value[0]), np.ones(permutations + 1, bool)
        if partial:
            den_xz = np.sqrt(ss_x * ss_z)
            r_xz = triangle_chain(xp * z[None]) / den_xz
            r_yz = float(triangle_chain(y * z)) / np.sqrt(ss_y * ss_z)
            value, counted = partial_statistic(value, r_xz, r_yz)
            if not counted[0]:
                continue
            records[k]["r_xz"], records[k]["r_yz"] = r_xz[0], r_yz
        records[k]["r"], records[k]["stat"] = r_xy, value[0]
        stat[k] = np.where(counted, value, NA)
        records[k]["at_least"] = int((counted[1:] & (value[1:] >= value[0])).sum())
        records[k]["p"] = float(1 + int(records[k]["at_least"])) / float(permutations + 1)
    return cohort_mod.Mantel(records, stat)


def numpy_anosim(kr, totals, labels, permutations, seed, strata=None):
    """`cohort_mod.Anosim` by the rule."""
    labels = np.asarray(labels)
    s, m_cols = labels.shape
    records = np.zeros(m_cols, dtype=capi.ANOSIM)
    for f in ANOSIM_DOUBLES:
        records[f] = NA
    stat = np.full((m_cols, permutations + 1), NA)
    for c in range(m_cols):
        idx, lam, number = [], [], {}
        for i in range(s):
            if int(totals[i]) == 0 or labels[i, c] == MISSING:
                continue
            idx.append(i)
            lam.append(number.setdefault(int(labels[i, c]), len(number)))
        u, lam = np.array(idx, dtype=np.int64), np.array(lam, dtype=np.int64)
        n, groups = len(u), len(number)
        sizes = [int((lam == g).sum()) for g in range(groups)]
        m, m_within = n * (n - 1) // 2, sum(k * (k - 1) // 2 for k in sizes)
        records[c]["used"], records[c]["groups"] = n, groups
        if groups < 2 or m_within < 1:
            continue
        upper = np.triu(kr[np.ix_(u, u)], 1)
        ranks = np.triu(midranks_of_pairs(upper + upper.T), 1)
        sigma = numpy_sigma(np.zeros(n, np.int64) if strata is None else np.asarray(strata)[u], seed, permutations)
        mu = lam[sigma]                                                             # lambda^p, [P + 1][n]
        w = (ranks[None] * (mu[:, :, None] == mu[:, None, :])).sum(axis=(1, 2))     # exact: every term is a multiple of 0.5
        within, between = w / float(m_within), (float(m * (m + 1) // 2) - w) / float(m - m_within)
        r = (between - within) / (float(m) / 2.0)
        records[c]["r"], records[c]["mean_between"], records[c]["mean_within"] = r[0], between[0], within[0]
        stat[c] = r
        records[c]["at_least"] = int((r[1:] >= r[0]).sum())
        records[c]["p"] = float(1 + int(records[c]["at_least"])) / float(permutations + 1)
    return cohort_mod.Anosim(records, stat)


def same_result(got, want, doubles, what=""):
    """Every field of every record and every stat[p], bit for bit; no arithmetic NaN reaches an output."""
    for f in got.records.dtype.names:
        if f in doubles:
            assert same_bits(got.records[f], want.records[f]), (what, f, got.records[f], want.records[f])
            v = got.records[f]
            assert (v.view(U64)[np.isnan(v)] == U64(capi.NA_BITS)).all(), (what, f)
        else:
            assert np.array_equal(got.records[f], want.records[f]), (what, f, got.records[f], want.records[f])
    if want.stat is not None and got.stat is not None:
        assert same_bits(got.stat, want.stat), (what, "stat", np.argwhere(got.stat.view(U64) != want.stat.view(U64))[:8])
        assert (got.stat.view(U64)[np.isnan(got.stat)] == U64(capi.NA_BITS)).all(), what
    return True


def same_mantel(got, want, what=""):
    return same_result(got, want, MANTEL_DOUBLES, what)


def same_anosim(got, want, what=""):
    return same_result(got, want, ANOSIM_DOUBLES, what)


# ---- the cases --------------------------------------------------------------------------------------------------------------
def mantel_sides(rng, kr):
    """(values [5][S], matrices [2][S][S], present [2][S]) for a cohort with the distances kr: a column that follows one
    sample's distances; small integers, so |v_s - v_t| is heavily tied; a column with a fifth missing; a constant column
    (undefined); noise; a matrix that follows kr, one sample missing from it; and a matrix of noise, all present."""
    s = kr.shape[0]
    kr = np.where(kr < 0.0, 0.0, kr)                                 # (the distance to a sample without mass is -1)
    values = np.array([kr[int(np.argmax(kr.sum(axis=1)))] + 0.1 * rng.random(s), rng.integers(0, 3, size=s).astype(np.float64),
                       np.where(rng.random(s) < 0.2, np.nan, rng.normal(size=s)), np.full(s, 2.5), rng.normal(size=s)])
    noise = rng.random((2, s, s))
    matrices = np.array([kr + 0.25 * (noise[0] + noise[0].T), noise[1] + noise[1].T])
    present = np.ones((2, s), np.uint8)
    present[0, s // 2] = 0
    return values, matrices, present


def anosim_labels(rng, num_samples):
    """labels [S][4]: two groups; three unbalanced groups under scattered ids with a fifth missing; one group (undefined); and
    every sample its own group (no pair within: undefined)."""
    s = num_samples
    cols = [rng.integers(0, 2, size=s), np.where(rng.random(s) < 0.2, MISSING, np.array([255, 3, 77])[rng.choice(3, size=s, p=[0.5, 0.3, 0.2])]),
            np.full(s, 17), np.arange(s) % 256]
    return np.ascontiguousarray(np.array(cols, dtype=np.uint32).T)


def cohort_case(num_samples, seed=11, tree_name="tree15"):
    """(mass, first, bl, kr, totals) of a random cohort: one sample empty and, from 5 samples, two samples identical."""
    parent, bl = tree_case(tree_name)
    first = numpy_first(parent)
    rng = np.random.default_rng(seed * 1000 + num_samples)
    mass = random_cells(rng, num_samples, len(parent), empty=1, bits=42)
    if num_samples >= 5:
        full = np.flatnonzero(mass.any(axis=1))
        mass[full[2]] = mass[full[1]]
    return mass, first, bl, cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass)


SAMPLE_COUNTS = (3, 4, 5, 33, 65)
PERMUTATIONS = (1, 63, 64, 65)


@pytest.mark.parametrize("num_samples", SAMPLE_COUNTS)
def test_the_host_mirror_equals_the_numpy_restatement_bit_for_bit(num_samples):
    mass, first, bl, kr, totals = cohort_case(num_samples)
    rng = np.random.default_rng(40 + num_samples)
    values, matrices, present = mantel_sides(rng, kr)
    labels = anosim_labels(rng, num_samples)
    exist = defined = 0
    for permutations in PERMUTATIONS:
        seed = int(rng.integers(0, 1 << 63))
        for control in (None, 0, 5):                                # none, a column, a matrix
            methods = ("pearson", "spearman") if permutations != 63 else ("spearman",)
            want = numpy_mantel(kr, totals, values, matrices, present, methods, control, permutations, seed)
            got = cohort_mod.mantel_kr_host(kr, totals, values, matrices, present, methods, control, permutations, seed)
            same_mantel(got, want, (num_samples, permutations, control))
            exist += int((want.records["used"] >= 3).sum())
            defined += int((~np.isnan(want.records["p"])).sum())
            assert np.array_equal(want.records["partial"], [control is not None and q != control for q in want.records["side"]])
        same_mantel(cohort_mod.mantel_host(mass, first, bl, values, matrices, present, ("pearson",), 0, permutations, seed),
                    numpy_mantel(kr, totals, values, matrices, present, ("pearson",), 0, permutations, seed), "from the cells")
        want = numpy_anosim(kr, totals, labels, permutations, seed)
        same_anosim(cohort_mod.anosim_kr_host(kr, totals, labels, permutations, seed), want, (num_samples, permutations))
        same_anosim(cohort_mod.anosim_host(mass, first, bl, labels, permutations, seed), want, "from the cells")
        if num_samples >= 5:
            assert not np.isnan(want.records["p"][:2]).any() and np.isnan(want.records["p"][2:]).all()
    if num_samples == 3:                                            # n = 2: nothing is defined
        assert (want.records["used"] <= 2).all() and np.isnan(want.records["p"]).all()
    if num_samples >= 5:
        # the comparison cannot pass on NAs alone: more than half of the records with used >= 3 are defined
        assert 2 * defined > exist >= 100, (defined, exist)


def test_a_lean_call_and_one_method_are_the_rows_of_the_full_call():
    mass, first, bl, kr, totals = cohort_case(33)
    values, matrices, present = mantel_sides(np.random.default_rng(3), kr)
    both = cohort_mod.mantel_kr_host(kr, totals, values, matrices, present, ("pearson", "spearman"), 0, 20, 5)
    for method, name in enumerate(("pearson", "spearman")):
        one = cohort_mod.mantel_kr_host(kr, totals, values, matrices, present, (name,), 0, 20, 5, with_stat=False)
        assert one.stat is None and one.records.tobytes() == both.records[method::2].tobytes()
    assert both.records["method"].tolist() == [0, 1] * 7 and both.records["side"].tolist() == [q for q in range(7) for _ in (0, 1)]


# ---- strata -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_samples", (5, 33))
def test_strata_one_stratum_is_no_strata_and_singletons_cannot_move(num_samples):
    mass, first, bl, kr, totals = cohort_case(num_samples)
    rng = np.random.default_rng(50 + num_samples)
    values, matrices, present = mantel_sides(rng, kr)
    labels = anosim_labels(rng, num_samples)
    plain = cohort_mod.mantel_kr_host(kr, totals, values, matrices, present, ("pearson", "spearman"), 0, 19, 3)
    ranked = cohort_mod.anosim_kr_host(kr, totals, labels, 19, 3)
    one = np.full(num_samples, 9, np.uint32)
    assert same_mantel(cohort_mod.mantel_kr_host(kr, totals, values, matrices, present, ("pearson", "spearman"), 0, 19, 3, strata=one), plain)
    assert same_anosim(cohort_mod.anosim_kr_host(kr, totals, labels, 19, 3, strata=one), ranked)
    alone = np.arange(num_samples, dtype=np.uint32)[::-1].copy()     # every sample its own stratum: sigma_p is the identity
    fixed = cohort_mod.mantel_kr_host(kr, totals, values, matrices, present, ("pearson", "spearman"), 0, 19, 3, strata=alone)
    defined = ~np.isnan(fixed.records["p"])
    assert defined.any() and (fixed.records["at_least"][defined] == 19).all() and (fixed.records["p"][defined] == 1.0).all()
    assert same_bits(fixed.stat[defined], np.repeat(fixed.stat[defined][:, :1], 20, axis=1))
    still = cohort_mod.anosim_kr_host(kr, totals, labels, 19, 3, strata=alone)
    moved = ~np.isnan(still.records["p"])
    assert moved[0] and (still.records["at_least"][moved] == 19).all() and same_bits(still.stat[0], np.full(20, still.stat[0, 0]))
    three = (np.arange(num_samples) % 3).astype(np.uint32)
    same_mantel(cohort_mod.mantel_kr_host(kr, totals, values, matrices, present, ("pearson", "spearman"), 5, 19, 3, strata=three),
                numpy_mantel(kr, totals, values, matrices, present, ("pearson", "spearman"), 5, 19, 3, strata=three), "three strata")
    same_anosim(cohort_mod.anosim_kr_host(kr, totals, labels, 19, 3, strata=three), numpy_anosim(kr, totals, labels, 19, 3, strata=three))


# ---- the textbook forms -----------------------------------------------------------------------------------------------------
TEXTBOOK_CASES = (12, 20, 33)
# 16 times the worst relative deviations of the host mirror from the forms, measured over TEXTBOOK_CASES (the docstring)
RATIONAL_PEARSON_BOUND, RATIONAL_SPEARMAN_BOUND = 16 * 1.33e-15, 16 * 1.80e-16
SCIPY_PEARSON_BOUND, SCIPY_SPEARMAN_BOUND = 16 * 2.84e-15, 16 * 2.51e-16
RESIDUAL_BOUND = 16 * 3.93e-15


def relative(got, want):
    return abs(got - want) / max(abs(want), 1e-300)


def rational_r(a, b):
    """Pearson's r of two vectors of doubles in exact rationals, rounded once at the end."""
    a, b = [Fraction(float(v)) for v in a], [Fraction(float(v)) for v in b]
    ma, mb = sum(a) / len(a), sum(b) / len(b)
    sab = sum((p - ma) * (q - mb) for p, q in zip(a, b))
    squared = sab * sab / (sum((p - ma) ** 2 for p in a) * sum((q - mb) ** 2 for q in b))
    getcontext().prec = 60
    root = (Decimal(squared.numerator) / Decimal(squared.denominator)).sqrt()
    return math.copysign(float(root), float(sab))


def test_the_observed_statistics_are_the_textbook_forms():
    """The deviations are printed before they are bounded; the module's docstring has what was measured."""
    try:
        from scipy import stats as scipy_stats
    except ImportError:
        scipy_stats = None
    worst = {}
    note = lambda name, value: worst.__setitem__(name, max(worst.get(name, 0.0), value))
    for num_samples in TEXTBOOK_CASES:
        mass, first, bl, kr, totals = cohort_case(num_samples, seed=13)
        rng = np.random.default_rng(60 + num_samples)
        values, matrices, present = mantel_sides(rng, kr)
        values[2:4] = rng.normal(size=(2, num_samples))             # (no constant column, nothing missing: every test is defined)
        labels = anosim_labels(rng, num_samples)[:, :2].copy()
        for control in (None, 4):                                   # the noise column as the control: 1 - r_xz^2 is near 1
            got = cohort_mod.mantel_kr_host(kr, totals, values, matrices, present, ("pearson", "spearman"), control, 1, 1)
            for rec in got.records:
                q, partial = int(rec["side"]), bool(rec["partial"])
                has = ~np.isnan(values[q]) if q < 5 else present[q - 5].astype(bool)
                u = np.flatnonzero((totals != 0) & has)
                upper = np.triu_indices(len(u), 1)
                flat = [kr[np.ix_(u, u)][upper], side_table(q, u, values, matrices)[upper]]
                if partial:
                    flat.append(side_table(control, u, values, matrices)[upper])
                name = ("pearson", "spearman")[int(rec["method"])]
                raw = flat[:2]
                if name == "spearman":
                    flat = [scipy_stats.rankdata(v) for v in flat] if scipy_stats else [midranks_of_pairs_flat(v) for v in flat]
                assert not np.isnan(rec["p"]), (num_samples, q, name)
                note("rational " + name, relative(float(rec["r"]), rational_r(flat[0], flat[1])))
                if scipy_stats:
                    form = scipy_stats.pearsonr(*raw)[0] if name == "pearson" else scipy_stats.spearmanr(*raw)[0]
                    note("scipy " + name, relative(float(rec["r"]), float(form)))
                if partial:
                    assert 1.0 - float(rec["r_xz"]) ** 2 >= 0.5, (num_samples, q, name)
                    design = np.column_stack([np.ones(len(flat[2])), flat[2]])
                    residual = [v - design @ np.linalg.lstsq(design, v, rcond=None)[0] for v in flat[:2]]
                    note("residual", relative(float(rec["stat"]), float(np.corrcoef(residual[0], residual[1])[0, 1])))
                else:
                    assert rec["stat"] == rec["r"]
        ranked = cohort_mod.anosim_kr_host(kr, totals, labels, 1, 1)
        for c, rec in enumerate(ranked.records):
            u = np.flatnonzero((totals != 0) & (labels[:, c] != MISSING))
            upper = np.triu_indices(len(u), 1)
            ranks = scipy_stats.rankdata(kr[np.ix_(u, u)][upper]) if scipy_stats else midranks_of_pairs_flat(kr[np.ix_(u, u)][upper])
            same = (labels[u, c][:, None] == labels[u, c][None, :])[upper]
            clarke = (ranks[~same].mean() - ranks[same].mean()) / (len(ranks) / 2.0)
            note("clarke", relative(float(rec["r"]), float(clarke)))
    print({k: f"{v:.2e}" for k, v in sorted(worst.items())})
    assert worst["rational pearson"] <= RATIONAL_PEARSON_BOUND and worst["rational spearman"] <= RATIONAL_SPEARMAN_BOUND, worst
    assert worst["residual"] <= RESIDUAL_BOUND, worst
    assert worst["clarke"] <= 16 * 2.0 ** -52, worst                # (two means of exact sums: a few roundings)
    if scipy_stats:
        assert worst["scipy pearson"] <= SCIPY_PEARSON_BOUND and worst["scipy spearman"] <= SCIPY_SPEARMAN_BOUND, worst


def midranks_of_pairs_flat(v):
    v = np.asarray(v)
    return (v[None, :] < v[:, None]).sum(axis=1) + ((v[None, :] == v[:, None]).sum(axis=1) + 1) / 2.0


# ---- by hand ----------------------------------------------------------------------------------------------------------------
def test_two_separated_groups_of_two_give_r_one_exactly():
    """Within ranks 1 and 2, between ranks 3 .. 6: (4.5 - 1.5) / 3 = 1."""
    kr = np.array([[0, 1, 5, 6], [1, 0, 7, 8], [5, 7, 0, 2], [6, 8, 2, 0]], dtype=np.float64)
    got = cohort_mod.anosim_kr_host(kr, np.ones(4, U64), np.array([[0, 0, 1, 1]], np.uint32).T.copy(), 99, 1)
    rec = got.records[0]
    assert rec["r"] == 1.0 and rec["mean_between"] == 4.5 and rec["mean_within"] == 1.5 and rec["used"] == 4 and rec["groups"] == 2
    assert (got.stat[0] <= 1.0).all() and rec["at_least"] == int((got.stat[0, 1:] == 1.0).sum())
    assert rec["p"] == (1 + int(rec["at_least"])) / 100.0 and 0 < rec["at_least"] < 99       # a third of the 24 shuffles keep the groups


def test_the_distance_against_itself_is_one_and_counts_the_shuffles_that_keep_it():
    mass, first, bl, kr, totals = cohort_case(5)
    itself = np.where(kr < 0.0, 0.0, kr)[None]                      # (the distance to the sample without mass is -1: not a side's)
    got = cohort_mod.mantel_kr_host(kr, totals, None, itself, None, ("pearson", "spearman"), None, 200, 1)
    for k, rec in enumerate(got.records):
        assert rec["used"] == 4 and abs(float(rec["r"]) - 1.0) <= 4 * 2.0 ** -52 and rec["stat"] == rec["r"]
        # samples 1 and 2 are identical: swapping them moves no distance, so one shuffle in 12 beside the identity keeps s_xy
        keeps = got.stat[k, 1:] >= got.stat[k, 0]
        assert rec["at_least"] == int(keeps.sum()) and 0 < keeps.sum() < 100
        assert same_bits(got.stat[k, 1:][keeps], np.full(int(keeps.sum()), got.stat[k, 0]))


# ---- the refusals -----------------------------------------------------------------------------------------------------------
def test_the_entries_refuse_what_the_header_says():
    lib = capi.load()
    err = lambda: lib.epik_amd_last_error().decode()
    s = 6
    kr, totals = np.zeros((s, s)), np.ones(s, U64)
    values, matrices, present = np.zeros((65, s)), np.zeros((9, s, s)), np.ones((9, s), np.uint8)
    out, labels = np.zeros(130, capi.MANTEL), np.zeros((s, 1), np.uint32)
    call = lambda k=kr.ctypes.data, n=s, v=values.ctypes.data, mv=1, m=matrices.ctypes.data, pr=present.ctypes.data, mm=1, methods=1, \
        control=NONE, p=9, o=out.ctypes.data: lib.epik_amd_cohort_mantel_kr_host(k, totals.ctypes.data, n, v, mv, m, pr, mm, methods,
                                                                                 control, p, 1, None, o, None)
    assert call() == capi.OK
    for bad, words in ((dict(mv=65), ("num_columns", "[0, 64]")), (dict(mm=9), ("num_matrices", "[0, 8]")), (dict(mv=0, mm=0), ("side",)),
                       (dict(control=2), ("control = 2", "no side")), (dict(methods=0), ("methods",)), (dict(methods=4), ("methods",)),
                       (dict(p=0), ("num_permutations", "[1, 999999]")), (dict(p=1_000_000), ("num_permutations",)),
                       (dict(k=None), ("null argument",)), (dict(o=None), ("null argument",)), (dict(v=None), ("null argument",)),
                       (dict(pr=None), ("null argument",)), (dict(n=8193), ("8192",))):
        assert call(**bad) == capi.ERR_INVALID and all(w in err() for w in words), (bad, err())
    assert call(v=None, mv=0) == capi.OK and call(m=None, pr=None, mm=0) == capi.OK
    values[0, 3] = np.inf
    assert call() == capi.ERR_INVALID and "sample 3" in err() and "infinite" in err()
    values[0, 3] = np.nan                                           # (missing: no error)
    matrices[0, 1, 4] = -1.0
    assert call() == capi.ERR_INVALID and "[1][4]" in err() and "negative" in err()
    matrices[0, 4, 1], matrices[0, 1, 4] = -1.0, 0.0                # (below the diagonal: never read)
    assert call() == capi.OK
    ranked = np.zeros(1, capi.ANOSIM)
    again = lambda n=s, m=1, p=9, l=labels.ctypes.data, o=ranked.ctypes.data: lib.epik_amd_cohort_anosim_kr_host(
        kr.ctypes.data, totals.ctypes.data, n, l, m, p, 1, None, o, None)
    assert again() == capi.OK
    for bad, words in ((dict(n=8193), ("8192",)), (dict(m=0), ("num_columns",)), (dict(m=65), ("num_columns",)), (dict(p=0), ("num_permutations",)),
                       (dict(l=None), ("null argument",)), (dict(o=None), ("null argument",))):
        assert again(**bad) == capi.ERR_INVALID and all(w in err() for w in words), (bad, err())
    labels[2, 0] = 256
    assert again() == capi.ERR_INVALID and "sample 2" in err() and "256" in err()
    with pytest.raises(ValueError, match="unknown method"):
        cohort_mod.mantel_kr_host(kr, totals, values[:1], methods=("kendall",))


# ---- the host code stand-alone ---------------------------------------------------------------------------------------------
def test_host_test_binary_mantel_and_anosim_are_the_library_s(host_bins, tmp_path):
    binary = os.path.join(host_bins, "cohort_test")
    for num_samples, permutations, control, layered in ((3, 1, None, False), (5, 64, 0, False), (33, 65, 5, True), (65, 20, None, True)):
        mass, first, bl, kr, totals = cohort_case(num_samples, seed=17)
        rng = np.random.default_rng(70 + num_samples)
        values, matrices, present = mantel_sides(rng, kr)
        labels = anosim_labels(rng, num_samples)
        strata = (np.arange(num_samples) % 3).astype(np.uint32) if layered else None
        _cells_input(tmp_path / "mass.bin", mass, first, bl)
        head = np.array([len(values), len(matrices), 3, NONE if control is None else control], dtype="<u8")
        (tmp_path / "sides.bin").write_bytes(head.tobytes() + values.tobytes() + matrices.tobytes() + present.tobytes())
        (tmp_path / "labels.bin").write_bytes(labels.tobytes())
        (tmp_path / "strata.bin").write_bytes(strata.tobytes() if layered else b"")
        tail = [str(tmp_path / "strata.bin") if layered else "-", str(permutations), "12345678901234567890"]
        run = subprocess.run([binary, "mantel", str(tmp_path / "out.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "sides.bin")] + tail,
                             capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (num_samples, run.stderr)
        want = cohort_mod.mantel_host(mass, first, bl, values, matrices, present, ("pearson", "spearman"), control, permutations,
                                      12345678901234567890, strata=strata)
        assert (tmp_path / "out.bin").read_bytes() == want.records.tobytes() + want.stat.tobytes(), num_samples
        run = subprocess.run([binary, "anosim", str(tmp_path / "out.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "labels.bin")] + tail,
                             capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (num_samples, run.stderr)
        want = cohort_mod.anosim_host(mass, first, bl, labels, permutations, 12345678901234567890, strata=strata)
        assert (tmp_path / "out.bin").read_bytes() == want.records.tobytes() + want.stat.tobytes(), num_samples
    head[3] = 9
    (tmp_path / "sides.bin").write_bytes(head.tobytes() + values.tobytes() + matrices.tobytes() + present.tobytes())
    run = subprocess.run([binary, "mantel", str(tmp_path / "o.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "sides.bin"), "-", "9", "1"],
                         capture_output=True, text=True)
    assert run.returncode == 1 and "control = 9" in run.stderr


# ---- the files --------------------------------------------------------------------------------------------------------------
FILE_NAMES = ["a", "skin 3", "it's", "none", "z.9_-", "q", "r", "s", "t"]
FILE_META = ("sample\tph\tdepth\n" "q\t6.5\t3\n" "a\t7.25\t1\n" "skin 3\t5\t2\n" "it's\t8.125\t3\n" "none\t7\t1\n" "z.9_-\t6\tNA\n"
             "r\t5.5\t2\n" "s\t9\t1\n" "t\t4.75\t3\n" "other\t1\t2\n")
FILE_FACTORS = ("sample\tstate\tsite\n" "q\tsick\tgut\n" "a\thealthy\tskin\n" "skin 3\tsick\tskin\n" "it's\thealthy\tgut\n" "none\tsick\tmouth\n"
                "z.9_-\thealthy\tNA\n" "r\tsick\tgut\n" "s\thealthy\tmouth of 2\n" "t\tsick\tgut\n" "other\t1\t2\n")


def matrix_text(names, matrix):
    return "name\t" + "\t".join(names) + "\n" + "".join(
        name + "".join(f"\t{v:.17g}" for v in row) + "\n" for name, row in zip(names, matrix))


def files_case(tmp_path):
    """Nine named samples (one empty), a metadata file, a factor file and a matrix file that lacks sample `r` and has one more."""
    mass, first, bl, kr, totals = cohort_case(9, seed=19)
    rng = np.random.default_rng(91)
    noise = rng.random((9, 9))
    geo = np.where(np.eye(9, dtype=bool), 0.0, np.where(kr < 0.0, 0.0, kr) + (noise + noise.T))
    keep = [i for i, name in enumerate(FILE_NAMES) if name != "r"]
    order = keep[::-1]                                              # the file's own order, and a name outside the list
    block = np.zeros((len(order) + 1, len(order) + 1))
    block[:-1, :-1] = geo[np.ix_(order, order)]
    block[-1, :-1] = block[:-1, -1] = 2.5
    (tmp_path / "geo.tsv").write_text("# distances by road\n" + matrix_text([FILE_NAMES[i] for i in order] + ["elsewhere"], block))
    (tmp_path / "meta.tsv").write_text(FILE_META)
    (tmp_path / "factors.tsv").write_text(FILE_FACTORS)
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in FILE_NAMES))
    _cells_input(tmp_path / "mass.bin", mass, first, bl)
    present = np.array([[name != "r" for name in FILE_NAMES]], np.uint8)
    geo[~present[0].astype(bool)] = 0.0
    geo[:, ~present[0].astype(bool)] = 0.0
    return mass, first, bl, totals, geo[None], present


def test_the_files_from_python_and_from_cpp_agree_and_read_back(host_bins, tmp_path):
    mass, first, bl, totals, matrices, present = files_case(tmp_path)
    binary = os.path.join(host_bins, "cohort_test")
    columns, meta, _ = cohort_mod.read_metadata(str(tmp_path / "meta.tsv"), FILE_NAMES)
    values = np.ascontiguousarray(np.asarray(meta, dtype=np.float64).T)
    sides = list(columns) + ["geo"]
    for method, partial in (("pearson", None), ("both", "geo"), ("spearman", "ph")):
        control = None if partial is None else sides.index(partial)
        methods = ("pearson", "spearman") if method == "both" else (method,)
        run = subprocess.run([binary, "mantel-tsv", str(tmp_path / "cpp.tsv"), str(tmp_path / "mass.bin"), str(tmp_path / "names.txt"),
                              str(tmp_path / "meta.tsv"), "geo=" + str(tmp_path / "geo.tsv"), method, partial or "-", "99", "7"],
                             capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, run.stderr
        got = cohort_mod.mantel_host(mass, first, bl, values, matrices, present, methods, control, 99, 7, with_stat=False)
        text = cohort_mod.format_mantel_tsv(FILE_NAMES, totals, sides, len(columns), method, control, 99, 7, got.records)
        assert (tmp_path / "cpp.tsv").read_text() == text, (method, partial)
        assert not np.isnan(got.records["p"]).any() and text.startswith("# epik_amd mantel v1  samples=9 used=8 sides=3 permutations=99 seed=7")
        names, kinds, records, info = cohort_mod.read_mantel_tsv(str(tmp_path / "cpp.tsv"))
        assert names == sides and kinds == ["column", "column", "matrix"] and records.tobytes() == got.records.tobytes()
        assert info["partial"] == partial and info["method"] == method and info["distance"] == "kr" and len(info["unused"]) == 1
    layered = cohort_mod.format_mantel_tsv(FILE_NAMES, totals, sides, 2, method, control, 99, 7, got.records, "weighted", "subject")
    assert layered.split("\n")[0].endswith("partial=ph\tdistance=weighted\tstrata=subject")
    (tmp_path / "layered.tsv").write_text(layered)
    assert cohort_mod.read_mantel_tsv(str(tmp_path / "layered.tsv"))[3]["strata"] == "subject"
    run = subprocess.run([binary, "anosim-tsv", str(tmp_path / "cpp.tsv"), str(tmp_path / "mass.bin"), str(tmp_path / "names.txt"),
                          str(tmp_path / "factors.tsv"), "99", "7"], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr
    columns, labels, label_names, _ = cohort_mod.read_factors(str(tmp_path / "factors.tsv"), FILE_NAMES)
    got = cohort_mod.anosim_host(mass, first, bl, labels, 99, 7, with_stat=False)
    text = cohort_mod.format_anosim_tsv(FILE_NAMES, totals, columns, label_names, labels, 99, 7, got.records)
    assert (tmp_path / "cpp.tsv").read_text() == text and not np.isnan(got.records["p"]).any()
    names, groups, records, info = cohort_mod.read_anosim_tsv(str(tmp_path / "cpp.tsv"))
    assert names == list(columns) and records.tobytes() == got.records.tobytes() and info["permutations"] == 99
    assert [sum(n for _, n in g) for g in groups] == [int(u) for u in records["used"]]


def test_every_error_of_the_matrix_file_names_its_line(host_bins, tmp_path):
    files_case(tmp_path)
    binary = os.path.join(host_bins, "cohort_test")
    good = (tmp_path / "geo.tsv").read_text().split("\n")            # line 1 a comment, line 2 the names, line 3 .. the rows

    def refused(lines, *words, partial="-"):
        (tmp_path / "bad.tsv").write_text("\n".join(lines))
        run = subprocess.run([binary, "mantel-tsv", str(tmp_path / "o.tsv"), str(tmp_path / "mass.bin"), str(tmp_path / "names.txt"), "-",
                              "geo=" + str(tmp_path / "bad.tsv"), "pearson", partial, "9", "1"], capture_output=True, text=True)
        assert run.returncode == 1 and all(w in run.stderr for w in words), (words, run.stderr)

    cells = good[3].split("\t")
    refused(good[:3] + ["\t".join(cells[:3] + ["-1"] + cells[4:])] + good[4:], "line 4", "column 3", "negative or not finite")
    refused(good[:3] + ["\t".join(cells[:3] + ["inf"] + cells[4:])] + good[4:], "line 4", "column 3")
    refused(good[:3] + ["\t".join(cells[:3] + ["x"] + cells[4:])] + good[4:], "line 4", "column 3", "not a number")
    refused(good[:3] + ["\t".join(cells[:1] + ["0.125"] + cells[2:])] + good[4:], "line 4", "column 1", "mirror")
    refused(good[:4] + [good[2]] + good[4:], "line 5", "given twice")
    refused(good[:1] + [good[1] + "\t" + good[1].split("\t")[1]] + good[2:], "line 2", "given twice")
    refused(good[:3] + ["\t".join(cells[:-1])] + good[4:], "line 4", "fields")
    refused(good[:3] + ["\t".join(["nobody"] + cells[1:])] + good[4:], "line 4", "nobody")
    refused(good[:3] + good[4:], "no row", cells[0])
    refused(good, "--cohort-mantel-partial", "'depth'", partial="depth")


# ---- the drivers' flags -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_drivers_refuse_the_flags_and_read_the_sides_before_the_database(host_bins, tmp_path, binary):
    files_case(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    (tmp_path / "samples.list").write_text("".join(f"{name}\tnone.fasta\n" for name in FILE_NAMES))
    (tmp_path / "none.fasta").write_text(">r\nACGT\n")
    base = [os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "samples.list"), "-o", str(out)]
    meta, geo, factors = str(tmp_path / "meta.tsv"), "geo=" + str(tmp_path / "geo.tsv"), str(tmp_path / "factors.tsv")

    def refused(extra, *words):
        run = subprocess.run(base + extra, capture_output=True, text=True)
        assert run.returncode == 255 and run.stderr.startswith("Error:"), (extra, run.stdout + run.stderr)
        assert all(w in run.stderr for w in words), (extra, run.stderr)
        assert "Loading database" not in run.stdout and "HIP device" not in run.stderr and not list(out.iterdir())

    for flag, value in (("--cohort-mantel", meta), ("--cohort-mantel-matrix", geo), ("--cohort-anosim", factors)):
        refused([flag, value], flag + " needs --cohort")
    for flag, value in (("--cohort-mantel-method", "both"), ("--cohort-mantel-partial", "ph"), ("--cohort-mantel-permutations", "9"),
                        ("--cohort-mantel-seed", "1")):
        refused(["--cohort", flag, value], flag + " needs --cohort-mantel or --cohort-mantel-matrix")
        refused([flag, value], flag + " needs", "--cohort )")
    for flag in ("--cohort-anosim-permutations", "--cohort-anosim-seed"):
        refused(["--cohort", flag, "9"], flag + " needs --cohort-anosim")
    refused(["--cohort", "--cohort-strata", factors], "--cohort-strata needs --cohort-permanova, --cohort-permdisp, --cohort-edge-test or --cohort-model")
    refused(["--cohort", "--cohort-distance", "weighted"], "--cohort-distance needs --cohort-permanova, --cohort-pcoa or --cohort-permdisp")
    for flag in ("--cohort-mantel-permutations", "--cohort-anosim-permutations"):
        for bad in ("0", "1000000", "x"):
            refused(["--cohort", "--cohort-mantel", meta, "--cohort-anosim", factors, flag, bad], flag + " " + bad, "[1, 999999]")
    refused(["--cohort", "--cohort-mantel", meta, "--cohort-mantel-seed", "-1"], "not a uint64")
    refused(["--cohort", "--cohort-mantel", meta, "--cohort-mantel-method", "kendall"], "pearson, spearman or both", "kendall")
    refused(["--cohort", "--cohort-mantel", meta, "--cohort-mantel-partial", "salinity"], "--cohort-mantel-partial", "'salinity'")
    refused(["--cohort", "--cohort-mantel", meta, "--cohort-mantel-matrix", "ph=" + str(tmp_path / "geo.tsv")], "'ph' is given twice")
    refused(["--cohort", "--cohort-mantel-matrix", "geo"], "NAME=FILE")
    refused(["--cohort"] + [x for k in range(9) for x in ("--cohort-mantel-matrix", f"g{k}=" + str(tmp_path / "geo.tsv"))], "9 times", "8 at the most")
    refused(["--cohort", "--cohort-mantel-matrix", "geo=" + str(tmp_path / "nowhere.tsv")], "cannot open", "nowhere.tsv")
    (tmp_path / "bad.tsv").write_text(FILE_META.replace("8.125", "eight"))
    refused(["--cohort", "--cohort-mantel", str(tmp_path / "bad.tsv")], "line 5", "eight")
    # what is allowed gets as far as the device or, where there is one, the database, which is not there: the sides were read
    # first, strata and distance accepted
    run = subprocess.run(base + ["--cohort", "--cohort-mantel", meta, "--cohort-mantel-matrix", geo, "--cohort-mantel-matrix",
                                 "road=" + str(tmp_path / "geo.tsv"), "--cohort-mantel-partial", "road", "--cohort-anosim", factors,
                                 "--cohort-strata", factors, "--cohort-strata-column", "state", "--cohort-distance", "weighted"],
                         capture_output=True, text=True)
    assert run.returncode == 255 and "Cohort Mantel sides: 2 columns, 2 matrices, 3 lines of samples that are not in the list skipped" in run.stdout
    assert "Cohort ANOSIM factors: 2 columns, 1 lines" in run.stdout and ("none.ekdb" in run.stderr or "HIP device" in run.stderr), run.stdout + run.stderr
    shown = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert shown.returncode == 0 and "cohort_mantel_<list>.tsv" in shown.stdout and "cohort_anosim_<list>.tsv" in shown.stdout
    for flag in ("--cohort-mantel arg", "--cohort-mantel-matrix arg", "--cohort-mantel-method arg", "--cohort-mantel-partial arg",
                 "--cohort-mantel-permutations arg", "--cohort-mantel-seed arg", "--cohort-anosim arg", "--cohort-anosim-permutations arg",
                 "--cohort-anosim-seed arg"):
        assert flag in shown.stdout, flag


def test_the_launcher_passes_the_flags_on_and_refuses_them_alone():
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import epik
    base = dict(database="db", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram=None, gpus=1, input_file="q")
    argv = epik.driver_command(**base, cohort=True, cohort_mantel="m.tsv", cohort_mantel_matrix=("a=1.tsv", "b=2.tsv"), cohort_mantel_method="both",
                               cohort_mantel_partial="a", cohort_mantel_permutations=9, cohort_mantel_seed=(1 << 64) - 1,
                               cohort_anosim="f.tsv", cohort_anosim_permutations=7, cohort_anosim_seed=2, cohort_strata="f.tsv",
                               cohort_distance="weighted")
    text = " ".join(argv)
    for piece in ("--cohort-mantel m.tsv", "--cohort-mantel-matrix a=1.tsv --cohort-mantel-matrix b=2.tsv", "--cohort-mantel-method both",
                  "--cohort-mantel-partial a", "--cohort-mantel-permutations 9", "--cohort-mantel-seed 18446744073709551615",
                  "--cohort-anosim f.tsv --cohort-anosim-permutations 7 --cohort-anosim-seed 2", "--cohort-strata f.tsv",
                  "--cohort-distance weighted"):
        assert piece in text, piece
    assert "--cohort-mantel" not in " ".join(epik.driver_command(**base, cohort=True))
    import click
    for options, word in ((dict(cohort_mantel="m.tsv"), "--cohort-mantel needs --cohort"), (dict(cohort_anosim="f.tsv"), "--cohort-anosim needs --cohort"),
                          (dict(cohort_mantel_matrix=("a=1",)), "--cohort-mantel-matrix needs --cohort"),
                          (dict(cohort=True, cohort_mantel_seed=1), "--cohort-mantel-seed needs"),
                          (dict(cohort=True, cohort_mantel_method="both"), "--cohort-mantel-method needs"),
                          (dict(cohort=True, cohort_anosim_seed=1), "--cohort-anosim-seed needs --cohort-anosim"),
                          (dict(cohort=True, cohort_strata="f.tsv"), "--cohort-strata needs"),
                          (dict(cohort=True, cohort_distance="weighted"), "--cohort-distance needs"),
                          (dict(cohort=True, cohort_mantel_matrix=tuple(f"g{k}=x" for k in range(9))), "8 times")):
        with pytest.raises(click.UsageError, match=word):
            epik.driver_command(**base, **options)
    me = os.path.join(root, "epik.py")
    out = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("--cohort-mantel ", "--cohort-mantel-matrix", "--cohort-mantel-method", "--cohort-mantel-partial", "--cohort-mantel-permutations",
                 "--cohort-mantel-seed", "--cohort-anosim ", "--cohort-anosim-permutations", "--cohort-anosim-seed"):
        assert flag in out.stdout, flag
