"""The sequential model (adonis2, by = "terms") of a cohort's samples over their distances on the host
(epik_amd/host/cohort.cpp: model_records_of_kr), without a GPU: the case derived by hand; the rule restated in numpy (a Python
loop over j, vectorised over rows, columns and permutations) against the host mirror bit for bit, every F of every
permutation, every field and every aliased byte; a model of one factor against PERMANOVA; the observed sums against the
textbook form tr(H G) in decimal arithmetic; the permutation share against all 720 orders of six positions; the symbols and
their refusals; the stand-alone host binary, plain and under the sanitizers.
"""
import decimal
import itertools
import os
import subprocess

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod
from test_cohort_cpu import host_bins, numpy_first, random_cells, same_bits, tree_case  # noqa: F401 (host_bins: a fixture)
from test_permanova_cpu import _cells_input, numpy_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
MISSING = capi.MODEL_MISSING
NA = float(np.uint64(capi.NA_BITS).view(np.float64))
DOUBLES = ("ss", "f", "r2", "p")


# ---- the rule restated ------------------------------------------------------------------------------------------------------
def numpy_arrangements(n, seed, permutations):
    """sigma_p for p = 0 .. P, [P + 1][n]: a stable argsort of the keys is the order of (key, position); the position at slot
    r has rank r."""
    order = np.argsort(numpy_keys(seed, permutations, n), axis=1, kind="stable")
    sigma = np.empty((permutations + 1, n), dtype=np.int64)
    np.put_along_axis(sigma, order, np.broadcast_to(np.arange(n), sigma.shape), axis=1)
    sigma[0] = np.arange(n)
    return sigma


def numpy_gower(kr, used):
    """B over the used samples as the centring paragraph of the principal coordinates forms it, and ss_total."""
    n = len(used)
    a2 = kr[np.ix_(used, used)] * kr[np.ix_(used, used)]
    r = np.zeros(n)
    for j in range(n):
        r = r + a2[j, :]                                                    # r_i reads KR[u_j][u_i]
    g = 0.0
    if n:
        r = r / float(n)
        for i in range(n):
            g = g + r[i]
        g = g / float(n)
    upper = -0.5 * (((a2 - r[:, None]) - r[None, :]) + g)
    b = np.triu(upper) + np.triu(upper, 1).T
    total = 0.0
    for i in range(n):
        total = total + b[i, i]
    return b, float(total)


def numpy_sums(b, basis, sigma):
    """s_c of every arrangement sigma[Q][n] and every accepted column basis[R][n]: [Q][R].  Every chain in the rule's order."""
    q, n = sigma.shape
    moved = basis[:, sigma].transpose(1, 0, 2)                              # [Q][R][n]: q_c[sigma(j)]
    t = np.zeros((q, basis.shape[0], n))
    for j in range(n):
        t = t + b[:, j][None, None, :] * moved[:, :, j][:, :, None]
    s = np.zeros((q, basis.shape[0]))
    for i in range(n):
        s = s + moved[:, :, i] * t[:, :, i]
    return s


def numpy_model(kr, totals, kind, labels, values, permutations, seed):
    """`cohort_mod.Model` by the rule."""
    kr, kind, labels, values = np.asarray(kr, dtype=np.float64), np.asarray(kind), np.asarray(labels), np.asarray(values, dtype=np.float64)
    s, terms = labels.shape
    present = np.where(kind[None, :] != 0, ~np.isnan(values), labels != MISSING)
    used = np.flatnonzero((np.asarray(totals) != 0) & present.all(axis=1))
    n = len(used)
    b, ss_total = numpy_gower(kr, used)
    basis, df, columns, aliased = [], [0] * (terms + 1), [0] * (terms + 1), np.zeros(capi.MODEL_MAX_COLUMNS, dtype=np.uint8)
    count = 0
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
    rank = len(basis)
    df[terms], columns[terms] = rank, count
    df_res = n - 1 - rank
    basis = np.array(basis).reshape(rank, n)

    def sums(sigma):
        """SS_k [Q][T + 1], the model's last."""
        s_c = numpy_sums(b, basis, sigma)
        out, model, at = np.zeros((len(sigma), terms + 1)), np.zeros(len(sigma)), 0
        for t in range(terms):
            acc = np.zeros(len(sigma))
            for _ in range(df[t]):
                acc = acc + s_c[:, at]
                at += 1
            out[:, t] = acc
            model = model + acc
        out[:, terms] = model
        return out

    sigma = numpy_arrangements(n, seed, permutations)
    ss0 = sums(sigma[:1])[0]
    ss_res = ss_total - ss0[terms]
    info = np.zeros(1, dtype=capi.MODEL_INFO)
    info[0] = (n, terms, count, rank, df_res, ss_total, ss_res)
    testable = df_res >= 1 and ss_res > 0.0
    records = np.zeros(terms + 1, dtype=capi.MODEL_TERM)
    for f in DOUBLES:
        records[f] = NA
    records["df"], records["columns"] = df, columns
    stat = np.full((terms + 1, permutations + 1), NA)
    every = sums(sigma) if testable and rank else None
    for k in range(terms + 1):
        if not df[k]:
            continue
        records["ss"][k] = ss0[k]
        if ss_total > 0.0:
            records["r2"][k] = ss0[k] / ss_total
        if not testable:
            continue
        res = ss_total - every[:, terms]
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(res > 0.0, (every[:, k] / float(df[k])) / (res / float(df_res)), np.inf)
        stat[k] = f
        records["f"][k] = f[0]
        records["at_least"][k] = int((f[1:] >= f[0]).sum())
        records["p"][k] = float(1 + int(records["at_least"][k])) / float(permutations + 1)
    return cohort_mod.Model(records, info[0], stat, aliased)


def same_model(got, want, what=""):
    for f in ("df", "columns", "at_least"):
        assert np.array_equal(got.records[f], want.records[f]), (what, f, got.records[f], want.records[f])
    for f in DOUBLES:
        assert same_bits(got.records[f], want.records[f]), (what, f, got.records[f], want.records[f])
    assert got.info.tobytes() == want.info.tobytes(), (what, got.info, want.info)
    assert np.array_equal(got.aliased, want.aliased), (what, got.aliased, want.aliased)
    if want.stat is not None and got.stat is not None:
        assert same_bits(got.stat, want.stat), (what, "stat", np.argwhere(got.stat.view(U64) != want.stat.view(U64))[:8])
    for v in [got.records[f] for f in DOUBLES] + ([got.stat] if got.stat is not None else []):
        assert (v.view(U64)[np.isnan(v)] == U64(capi.NA_BITS)).all(), what       # a NaN is the NA pattern, never arithmetic
    return True


def design(*terms):
    """(kind [T], labels [S][T], values [S][T]) from ("f", labels [S]) and ("n", values [S]) in test order."""
    s = len(terms[0][1])
    kind = np.array([0 if k == "f" else 1 for k, _ in terms], dtype=np.uint32)
    labels, values = np.full((s, len(terms)), MISSING, dtype=np.uint32), np.full((s, len(terms)), np.nan)
    for t, (k, column) in enumerate(terms):
        if k == "f":
            labels[:, t] = column
        else:
            values[:, t] = column
    return kind, labels, values


def designs_of(rng, s):
    """The designs the tests walk, by name, for s samples.  Every covariate has a missing value somewhere, unless that would
    leave nothing to test."""
    x, y = rng.normal(size=s), rng.integers(0, 9, size=s).astype(np.float64)
    two = (np.arange(s) % 2).astype(np.uint32)
    three = rng.choice(np.array([7, 3, 30], dtype=np.uint32), size=s)
    nested = two * 2 + rng.integers(0, 2, size=s).astype(np.uint32)             # each of its groups lies in one group of `two`
    if s > 8:
        x[3], three[5] = np.nan, MISSING
    return {
        "a lone covariate": design(("n", x)),
        "a lone factor": design(("f", three)),
        "factor, covariate": design(("f", two), ("n", x)),
        "covariate, factor": design(("n", x), ("f", two)),
        "a covariate given twice": design(("n", y), ("f", two), ("n", y)),
        "a factor nested in an earlier one": design(("f", nested), ("n", x), ("f", two)),
        "a constant column": design(("n", np.full(s, 2.5)), ("n", x)),
        "a factor of one group": design(("f", np.full(s, 4, dtype=np.uint32)), ("f", two)),
        "a term missing everywhere": design(("n", x), ("n", np.full(s, np.nan))),
        "rank L - 1": design(("f", np.arange(s, dtype=np.uint32) % 32), ("n", x)) if s <= 32 else
                      design(("f", np.arange(s, dtype=np.uint32) % 32), ("f", (np.arange(s, dtype=np.uint32) // 32) % 32), ("n", x), ("n", y)),
    }


def line_kr(x):
    x = np.asarray(x, dtype=np.float64)
    return np.abs(x[:, None] - x[None, :])


# ---- 1. by hand -------------------------------------------------------------------------------------------------------------
def test_four_points_on_a_line_by_hand():
    """Samples at 0, 1, 2, 3; the factor (a, a, b, b), then the covariate (0, 1, 2, 3).  The centred coordinates are -3/2, -1/2,
    1/2, 3/2: ss_total = 5.  q_0 = (-1/2, -1/2, 1/2, 1/2): SS_1 = (q_0 . x)^2 = 4.  The covariate less its part along q_0 is
    (-1/2, 1/2, -1/2, 1/2) = q_1: SS_2 = 1.  SS_res = 0: both F are NA, R2 = 0.8 and 0.2.  The factor alone: SS_res = 1,
    F = (4 / 1) / (1 / 2) = 8, PERMANOVA's numbers for that column.  Every number is exact in binary."""
    kr, ones = line_kr([0, 1, 2, 3]), np.ones(4, U64)
    both = design(("f", [5, 5, 2, 2]), ("n", [0.0, 1.0, 2.0, 3.0]))
    got = cohort_mod.model_kr_host(kr, ones, *both, permutations=50, seed=3)
    assert tuple(got.info) == (4, 2, 2, 2, 1, 5.0, 0.0)
    assert list(got.records["df"]) == [1, 1, 2] and list(got.records["columns"]) == [1, 1, 2] and not got.aliased.any()
    assert same_bits(got.records["ss"], [4.0, 1.0, 5.0]) and same_bits(got.records["r2"], [0.8, 0.2, 1.0])
    assert same_bits(got.records["f"], [NA] * 3) and same_bits(got.records["p"], [NA] * 3) and not got.records["at_least"].any()
    assert same_bits(got.stat, np.full((3, 51), NA))
    same_model(got, numpy_model(kr, ones, *both, 50, 3), "by hand")
    alone = design(("f", [5, 5, 2, 2]))
    got = cohort_mod.model_kr_host(kr, ones, *alone, permutations=200, seed=3)
    assert tuple(got.info) == (4, 1, 1, 1, 2, 5.0, 1.0)
    assert same_bits(got.records["ss"], [4.0, 4.0]) and same_bits(got.records["f"], [8.0, 8.0]) and same_bits(got.records["r2"], [0.8, 0.8])
    permanova = cohort_mod.permanova_kr_host(kr, ones, alone[1], permutations=200, seed=3).records[0, 0]
    assert same_bits(permanova["f"], 8.0) and same_bits(permanova["r2"], 0.8) and same_bits(permanova["ss_total"], 5.0)
    assert got.records["at_least"][0] == permanova["at_most"] and same_bits(got.records["p"][0], permanova["p"])
    same_model(got, numpy_model(kr, ones, *alone, 200, 3), "the factor alone")
    # a sample without mass, or without a value for ANY term, is not a position: the same model of the other four
    wide = np.full((6, 6), -1.0)
    wide[np.ix_([0, 2, 3, 5], [0, 2, 3, 5])] = kr
    more = design(("f", [5, 1, 5, 2, 2, 2]), ("n", [0.0, 9.0, 1.0, 2.0, np.nan, 3.0]))
    again = cohort_mod.model_kr_host(wide, np.array([3, 0, 1, 1, 9, 2], U64), *more, permutations=50, seed=3)
    same_model(again, cohort_mod.model_kr_host(kr, ones, *both, permutations=50, seed=3), "two samples that are no positions")


# ---- 2. the host mirror against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("num_samples", (2, 3, 5, 33, 65))
def test_host_mirror_equals_the_numpy_restatement_bit_for_bit(num_samples):
    parent, bl = tree_case("tree15")
    first = numpy_first(parent)
    rng = np.random.default_rng(2100 + num_samples)
    mass = random_cells(rng, num_samples + 1, len(parent), empty=1, bits=42)     # one sample without mass: L = num_samples
    kr, totals = cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass)
    seen = {}
    for name, (kind, labels, values) in designs_of(rng, num_samples + 1).items():
        permutations, seed = int(rng.integers(1, 40)), int(rng.integers(0, 1 << 63))
        want = numpy_model(kr, totals, kind, labels, values, permutations, seed)
        got = cohort_mod.model_kr_host(kr, totals, kind, labels, values, permutations, seed)
        same_model(got, want, (num_samples, name))
        same_model(cohort_mod.model_host(mass, first, bl, kind, labels, values, permutations, seed), want, (num_samples, name, "cells"))
        lean = cohort_mod.model_kr_host(kr, totals, kind, labels, values, permutations, seed, with_stat=False)
        assert lean.stat is None and lean.records.tobytes() == got.records.tobytes()
        seen[name] = got
    assert seen["a term missing everywhere"].info["used"] == 0 and seen["a term missing everywhere"].info["df_res"] == -1
    assert seen["a covariate given twice"].records["df"][2] == 0
    assert seen["a constant column"].aliased[0] == 1 and seen["a constant column"].records["df"][0] == 0
    assert seen["a factor of one group"].records["columns"][0] == 0
    nested = seen["a factor nested in an earlier one"]
    assert nested.records["df"][2] == 0
    if num_samples >= 5:                                                         # (below, the rank runs out first)
        assert list(seen["a covariate given twice"].aliased[:3]) == [0, 0, 1] and list(seen["a constant column"].aliased[:2]) == [1, 0]
        assert nested.aliased[:nested.info["columns"]].sum() == 1
    full = seen["rank L - 1"]
    if num_samples <= 33:
        assert full.info["df_res"] <= 0 and np.isnan(full.records["f"]).all() and not np.isnan(full.records["ss"][-1])
    # the order of the terms: the first term's sum changes, the model's does not beyond the rounding of its chains
    a, b = seen["factor, covariate"], seen["covariate, factor"]
    if num_samples >= 5:
        assert a.records["ss"][0] != b.records["ss"][1] and a.records["ss"][1] != b.records["ss"][0]
        assert abs(a.records["ss"][2] - b.records["ss"][2]) <= 1e-12 * abs(a.info["ss_total"])
        assert a.info["rank"] == b.info["rank"] == 2


def test_identical_samples_have_no_total():
    kind, labels, values = design(("f", [0, 1, 0, 1, 1]), ("n", [1.0, 2.0, 4.0, 8.0, 16.0]))
    got = cohort_mod.model_kr_host(np.zeros((5, 5)), np.ones(5, U64), kind, labels, values, permutations=9, seed=1)
    assert tuple(got.info) == (5, 2, 2, 2, 2, 0.0, 0.0) and list(got.records["df"]) == [1, 1, 2]
    assert same_bits(got.records["ss"], [0.0] * 3)
    for f in ("r2", "f", "p"):
        assert same_bits(got.records[f], [NA] * 3), f
    same_model(got, numpy_model(np.zeros((5, 5)), np.ones(5, U64), kind, labels, values, 9, 1))


# ---- 3. one factor: PERMANOVA ----------------------------------------------------------------------------------------------------
#: the worst relative deviation of ss and r2 between the two host mirrors over the cases below, measured on the CPU, and the
#: bound, 16 times that: the cases are a sample, and an error of formula shows at 1e-3
PERMANOVA_WORST = 1.4e-13
PERMANOVA_BOUND = 16 * PERMANOVA_WORST


@pytest.mark.parametrize("num_samples", (6, 12, 40))
def test_a_model_of_one_factor_is_permanova(num_samples):
    parent, bl = tree_case("tree15")
    first = numpy_first(parent)
    worst = 0.0
    for trial in range(4):
        rng = np.random.default_rng(3300 + 10 * num_samples + trial)
        mass = random_cells(rng, num_samples, len(parent), empty=trial, bits=42)
        kr, totals = cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass)
        groups = rng.permutation(np.arange(num_samples) % (2 + trial % 2)).astype(np.uint32)
        groups[rng.integers(0, num_samples)] = MISSING
        kind, labels, values = design(("f", groups))
        permutations, seed = 199, int(rng.integers(0, 1 << 63))
        model = cohort_mod.model_kr_host(kr, totals, kind, labels, values, permutations, seed)
        permanova = cohort_mod.permanova_kr_host(kr, totals, labels, permutations, seed)
        record = permanova.records[0, 0]
        assert model.info["used"] == record["used"] and model.records["df"][0] == record["groups"] - 1
        among = record["ss_total"] - record["ss_within"]
        for got, want in ((model.records["ss"][0], among), (model.records["r2"][0], record["r2"]), (model.info["ss_total"], record["ss_total"]),
                          (model.records["f"][0], record["f"])):
            deviation = abs(got - want) / abs(want)
            worst = max(worst, deviation)
            assert deviation <= PERMANOVA_BOUND, (num_samples, trial, got, want, deviation)
        # the same shuffles: F falls as SSW rises, so the permutations come in the same order wherever neither side ties
        f, ssw = model.stat[0], permanova.ssw[0, 0]
        for p, q in itertools.combinations(range(0, permutations + 1, 7), 2):
            if abs(ssw[p] - ssw[q]) > 1e-9 * abs(record["ss_total"]):
                assert (f[p] > f[q]) == (ssw[p] < ssw[q]), (num_samples, trial, p, q)
        clear = np.abs(ssw[1:] - ssw[0]) > 1e-9 * abs(record["ss_total"])
        assert ((f[1:] >= f[0]) == (ssw[1:] <= ssw[0]))[clear].all()
    print(f"one factor against PERMANOVA, S = {num_samples}: worst relative deviation {worst:.3e}")


# ---- 4. the textbook form -------------------------------------------------------------------------------------------------------
#: the worst relative deviation of the observed SS and F from the textbook form in 60-digit decimal arithmetic over the cases
#: below, measured on the CPU, and the bound, 16 times that
TEXTBOOK_WORST = 7.8e-16
TEXTBOOK_BOUND = 16 * TEXTBOOK_WORST


def decimal_solve(a, b):
    """x with a x = b by Gauss-Jordan elimination with partial pivoting, in Decimal."""
    n = len(a)
    m = [row[:] + [b[i]] for i, row in enumerate(a)]
    for c in range(n):
        pivot = max(range(c, n), key=lambda r: abs(m[r][c]))
        m[c], m[pivot] = m[pivot], m[c]
        for r in range(n):
            if r != c:
                factor = m[r][c] / m[c][c]
                m[r] = [x - factor * y for x, y in zip(m[r], m[c])]
    return [m[i][n] / m[i][i] for i in range(n)]


def textbook_sums(kr, columns_by_term):
    """SS of each term fitted after the ones before it, tr(H_k G) - tr(H_{k-1} G) with H the hat matrix of the intercept and
    the terms' columns up to k (least squares by the normal equations), and ss_total = tr(G), all in Decimal."""
    D = decimal.Decimal
    n = len(kr)
    a2 = [[D(float(kr[i][j])) ** 2 for j in range(n)] for i in range(n)]
    row = [sum(a2[i]) / n for i in range(n)]
    grand = sum(row) / n
    gower = [[-(a2[i][j] - row[i] - row[j] + grand) / 2 for j in range(n)] for i in range(n)]
    total = sum(gower[i][i] for i in range(n))
    design_columns, fitted, sums = [[D(1)] * n], D(0), []
    for columns in columns_by_term:
        design_columns += [[D(float(v)) for v in column] for column in columns]
        p = len(design_columns)
        xtx = [[sum(design_columns[a][i] * design_columns[b][i] for i in range(n)) for b in range(p)] for a in range(p)]
        # tr(H G) = tr((X'X)^-1 X' G X)
        xtgx = [[sum(design_columns[a][i] * gower[i][j] * design_columns[b][j] for i in range(n) for j in range(n)) for b in range(p)]
                for a in range(p)]
        trace = sum(decimal_solve(xtx, [xtgx[a][b] for a in range(p)])[b] for b in range(p))
        sums.append(trace - fitted)
        fitted = trace
    return sums, total


def test_observed_sums_are_the_textbook_s_in_decimal():
    parent, bl = tree_case("tree15")
    first = numpy_first(parent)
    worst = 0.0
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        for num_samples in (7, 12, 19):
            rng = np.random.default_rng(4400 + num_samples)
            mass = random_cells(rng, num_samples, len(parent), bits=42)
            mass[:, 0] |= U64(1)
            kr, totals = cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass)
            groups = (np.arange(num_samples) % 3).astype(np.uint32)
            x, y = rng.normal(size=num_samples), rng.integers(0, 5, size=num_samples).astype(np.float64)
            got = cohort_mod.model_kr_host(kr, totals, *design(("n", x), ("f", groups), ("n", y)), permutations=1, seed=1)
            assert not got.aliased.any() and list(got.records["df"]) == [1, 2, 1, 4]
            sums, total = textbook_sums(kr, [[x], [(groups == 1).astype(float), (groups == 2).astype(float)], [y]])
            residual = total - sum(sums)
            for k in range(3):
                f = (sums[k] / int(got.records["df"][k])) / (residual / int(got.info["df_res"]))
                for got_value, want in ((got.records["ss"][k], sums[k]), (got.records["f"][k], f)):
                    deviation = float(abs(decimal.Decimal(float(got_value)) - want) / abs(want))
                    worst = max(worst, deviation)
                    assert deviation <= TEXTBOOK_BOUND, (num_samples, k, got_value, want, deviation)
            assert float(abs(decimal.Decimal(float(got.info["ss_total"])) - total) / total) <= TEXTBOOK_BOUND
    print(f"the textbook form in decimal: worst relative deviation {worst:.3e}")


# ---- 5. the permutations -------------------------------------------------------------------------------------------------------
def test_the_share_of_permutations_at_least_the_observed_follows_all_720_orders():
    rng = np.random.default_rng(6)
    kr = line_kr([0.0, 0.7, 1.1, 3.0, 3.2, 4.5])
    kind, labels, values = design(("n", [0.1, 0.5, 0.2, 0.9, 0.6, 1.4]))
    ones = np.ones(6, U64)
    observed = cohort_mod.model_kr_host(kr, ones, kind, labels, values, permutations=1, seed=1)
    f0 = observed.records["f"][0]
    # every order of the rows of Q is an order of the covariate: the exact share
    exact = 0
    for order in itertools.permutations(range(6)):
        moved = design(("n", np.asarray(values[:, 0])[list(order)]))
        exact += cohort_mod.model_kr_host(kr, ones, *moved, permutations=1, seed=1).records["f"][0] >= f0 * (1 - 1e-12)
    share = exact / 720.0
    at_least = total = 0
    for seed in rng.integers(0, 1 << 62, size=40):
        got = cohort_mod.model_kr_host(kr, ones, kind, labels, values, permutations=500, seed=int(seed))
        at_least, total = at_least + int(got.records["at_least"][0]), total + 500
    sd = (share * (1 - share) / total) ** 0.5
    assert abs(at_least / total - share) <= 5 * sd, (at_least / total, share, sd)


# ---- 6. the symbols --------------------------------------------------------------------------------------------------------------
def test_model_symbols_exist_and_refuse_what_the_header_says():
    lib = capi.load()
    for name in ("epik_amd_cohort_model_device", "epik_amd_cohort_model", "epik_amd_cohort_model_metric", "epik_amd_cohort_model_host",
                 "epik_amd_cohort_model_metric_host", "epik_amd_cohort_model_kr_host"):
        assert hasattr(lib, name) and name in capi.EXPORTS, name
    assert capi.MODEL_TERM.itemsize == 48 and capi.MODEL_INFO.itemsize == 40
    err = lambda: lib.epik_amd_last_error().decode()
    kr, totals = line_kr(np.arange(40.0)), np.ones(40, U64)
    kind, labels, values = design(("f", np.arange(40) % 3), ("n", np.arange(40.0) ** 2))
    out, info = np.zeros(18, dtype=capi.MODEL_TERM), np.zeros(1, dtype=capi.MODEL_INFO)
    stat, aliased = np.zeros((18, 10)), np.zeros(64, dtype=np.uint8)

    def call(k=kr.ctypes.data, t=totals.ctypes.data, kd=kind, la=labels, va=values, terms=2, p=9, o=out.ctypes.data, i=info.ctypes.data,
             a=aliased.ctypes.data):
        kd, la, va = (None if v is None else np.ascontiguousarray(v) for v in (kd, la, va))
        return lib.epik_amd_cohort_model_kr_host(k, t, 40, *(None if v is None else v.ctypes.data for v in (kd, la, va)), terms, p, 5, o, i,
                                                 stat.ctypes.data, a)

    assert call() == capi.OK
    for null in ("k", "t", "kd", "la", "va", "o", "i", "a"):
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
    assert call(va=wrong) == capi.ERR_INVALID and "sample 23" in err() and "term 1" in err() and "infinite" in err()
    wrong[23, 0] = np.inf                                                        # (a factor's value is not read)
    wrong[23, 1] = 1.0
    assert call(va=wrong) == capi.OK
    # three factors of 23 labels: 66 columns
    wide = design(*[("f", (np.arange(40) * (t + 1)) % 23) for t in range(3)])
    assert call(kd=wide[0], la=wide[1], va=wide[2], terms=3) == capi.ERR_INVALID and "66 columns" in err() and "64" in err()
    assert lib.epik_amd_cohort_model_host(None, 40, 7, None, None, kind.ctypes.data, labels.ctypes.data, values.ctypes.data, 2, 9, 5,
                                          out.ctypes.data, info.ctypes.data, None, aliased.ctypes.data) == capi.ERR_INVALID
    assert "null argument" in err()
    with pytest.raises(ValueError):
        cohort_mod.model_kr_host(kr, totals, kind, labels[:, :1], values, 9, 5)


# ---- 7. the host code stand-alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitized", [False, True])
def test_host_test_binary_model_is_the_library_s(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    parent, bl = tree_case("tree15")
    first = numpy_first(parent)
    for num_samples in (2, 5, 33, 65):
        rng = np.random.default_rng(7700 + num_samples)
        mass = random_cells(rng, num_samples, len(parent), empty=1, bits=42)
        _cells_input(tmp_path / "mass.bin", mass, first, bl)
        for name, (kind, labels, values) in designs_of(rng, num_samples).items():
            permutations = int(rng.integers(1, 30))
            (tmp_path / "design.bin").write_bytes(np.array([len(kind)], dtype="<u8").tobytes() + kind.tobytes() + labels.tobytes() +
                                                  values.tobytes())
            run = subprocess.run([binary, "model", str(tmp_path / "out.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "design.bin"),
                                  str(permutations), "12345678901234567890"], capture_output=True, text=True)
            assert run.returncode == 0 and not run.stderr, (num_samples, name, run.stderr)
            want = cohort_mod.model_host(mass, first, bl, kind, labels, values, permutations, 12345678901234567890)
            assert (tmp_path / "out.bin").read_bytes() == \
                want.records.tobytes() + want.info.tobytes() + want.stat.tobytes() + want.aliased.tobytes(), (num_samples, name)
    bad = labels.copy()
    bad[1, 0] = 32
    (tmp_path / "design.bin").write_bytes(np.array([len(kind)], dtype="<u8").tobytes() + kind.tobytes() + bad.tobytes() + values.tobytes())
    run = subprocess.run([binary, "model", str(tmp_path / "o.bin"), str(tmp_path / "mass.bin"), str(tmp_path / "design.bin"), "9", "1"],
                         capture_output=True, text=True)
    assert run.returncode == 1 and "sample 1" in run.stderr and "32" in run.stderr
