"""The observed statistics of the edge test and of PERMANOVA against the textbook forms, which are not shaped like the rule.

The numpy restatements of test_edgetest_cpu and test_permanova_cpu follow the rule term by term (eta = A / sxx from centred
sums, ssw = sxx - A, SSW from the rows' chains) and would share a wrong formula with it.  Here the host mirror
(epik_amd_cohort_edgetest_host, epik_amd_cohort_permanova_host) is held to
  F         the one-way ANOVA F from the group means: (sum n_g (m_g - m)^2 / (G - 1)) / (sum (x_i - m_g(i))^2 / (L - G));
  H         the Kruskal-Wallis H, 12 / (n (n + 1)) * sum R_g^2 / n_g - 3 (n + 1), over the tie correction
            1 - sum (t^3 - t) / (n^3 - n): the rule's (L - 1) * eta2 on midranks;
  pseudo-F  Anderson's (2001) SS_T = sum_{i<j} d_ij^2 / N, SS_W = sum_g sum_{i<j in g} d_ij^2 / n_g, SS_A = SS_T - SS_W,
  and R^2   F = (SS_A / (G - 1)) / (SS_W / (N - G)), R^2 = SS_A / SS_T, from the squared distances of kr_host,
and to scipy.stats.f_oneway and scipy.stats.kruskal where scipy imports (on the large tree every eighth branch: the calls
are slow).

F and H are worked out in exact rational arithmetic from the doubles x_i (a double is a fraction) and rounded once at the
end; pseudo-F and R^2 with math.fsum over the squared distances.  math.fsum is not enough for F: with the sums exact, m_g
and m are still rounded quotients, and among 3 000 branches some F is as small as 3e-8 (eta2 = 5e-10, an imbalance of mean
-0.995 and deviation 0.003), where m_g - m keeps seven digits: that form was 9.1e-10 off the exact value there, the mirror
2.4e-16.  The tolerances are those of forms in doubles all the same: 1e-10 relative for F and pseudo-F, well-conditioned
sums of at most 70 terms while 1 - eta2 >= 0.5 (asserted: ssw = sxx - A loses a bit at the most), and 1e-7 relative for H.
A wrong degree of freedom, a missing tie correction or L in place of L - 1 moves a value by more than 1e-2.

The worst relative deviations measured over every defined branch of the cases below: F 2.3e-13 (f_oneway 3.0e-14), H 4.1e-16
(kruskal 5.9e-11), pseudo-F 3.6e-14, R^2 3.5e-14.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from epik_amd import cohort as cohort_mod, synth
from test_cohort_cpu import numpy_first, random_cells
from test_correlation_cpu import is_na
from test_edgetest_cpu import column_groups, numpy_midranks, numpy_vectors, sparser
from test_permanova_cpu import MISSING

try:
    from scipy import stats as scipy_stats
except ImportError:
    scipy_stats = None

F_BOUND, H_BOUND = 1e-10, 1e-7
CASES = ((7, 33), (999, 70))             # (N, S)
SCALE = 1 << 1074


def grouped_labels(rng, num_samples):
    """labels [S][2]: two groups and five groups, about a seventh of each column missing."""
    cols = [rng.integers(0, 2, size=num_samples), rng.integers(0, 5, size=num_samples)]
    cols = [np.where(rng.random(num_samples) < 1 / 7, MISSING, c) for c in cols]
    return np.ascontiguousarray(np.array(cols, dtype=np.uint32).T)


def textbook_case(num_branches, num_samples, kind):
    tree = synth.make_tree((num_branches + 1) // 2, seed=30)
    parent = np.asarray(tree.parent, dtype=np.int64)
    assert len(parent) == num_branches
    bl = np.array(tree.branch_length, dtype=np.float64)
    rng = np.random.default_rng(2600 + num_branches + num_samples)
    mass = random_cells(rng, num_samples, num_branches, empty=1, bits=42)
    labels = grouped_labels(rng, num_samples)
    if kind == "sparser":
        mass = sparser(rng, mass)
        mass[:, 0] |= np.uint64(1)        # (every sample keeps some mass, but the one that is empty)
        mass[1] = 0
    return mass, numpy_first(parent), bl, labels


def relative(got, want):
    return 0.0 if got == want else abs(got - want) / abs(want) if want != 0.0 else math.inf


def note(worst, name, value):
    worst[name] = max(worst.get(name, 0.0), value)


def exact(values):
    """The doubles as the integers values * 2^1074: every double is such an integer."""
    return [p * (SCALE // q) for p, q in map(float.as_integer_ratio, values.tolist())]


def anova_f(x, lam, sizes):
    """The one-way F of x[L] under the groups lam[L], from the group means, exactly; rounded once."""
    L, G = len(x), len(sizes)
    xs, lam = exact(x), lam.tolist()
    sums = [sum(v for v, g in zip(xs, lam) if g == k) for k in range(G)]
    mean = Fraction(sum(xs), L)
    among = sum(sizes[k] * (Fraction(sums[k], sizes[k]) - mean) ** 2 for k in range(G))
    # (x_i - m_g)^2 = (n_g x_i - sum_g)^2 / n_g^2: the squares summed as integers, a division a group
    within = sum(Fraction(sum((sizes[k] * v - sums[k]) ** 2 for v, g in zip(xs, lam) if g == k), sizes[k] ** 2) for k in range(G))
    return float((among / (G - 1)) / (within / (L - G)))


def kruskal_h(ranks, lam, sizes):
    """The Kruskal-Wallis H of the midranks ranks[L] under the groups lam[L], with the tie correction, exactly; rounded once."""
    n = len(ranks)
    doubled = [int(2 * r) for r in ranks.tolist()]
    assert all(d == 2 * r for d, r in zip(doubled, ranks.tolist()))
    sums = [Fraction(sum(d for d, g in zip(doubled, lam.tolist()) if g == k), 2) for k in range(len(sizes))]
    h = Fraction(12, n * (n + 1)) * sum(r * r / n_g for r, n_g in zip(sums, sizes)) - 3 * (n + 1)
    _, ties = np.unique(ranks, return_counts=True)
    return float(h / (1 - Fraction(sum(int(t) ** 3 - int(t) for t in ties), n ** 3 - n)))


@pytest.mark.parametrize("kind", ["dense", "sparser"])
@pytest.mark.parametrize("num_branches, num_samples", CASES)
def test_f_and_h_of_every_defined_branch_are_the_textbook_s(num_branches, num_samples, kind):
    mass, first, bl, labels = textbook_case(num_branches, num_samples, kind)
    got = cohort_mod.edgetest_host(mass, first, labels, 1, 1, with_stat=False, with_max=False).records
    xm, xi, inner, total = numpy_vectors(mass, first)
    checked, worst = 0, {}
    for c in range(labels.shape[1]):
        used, lam, sizes = column_groups(labels[:, c], total)
        L, G = len(used), len(sizes)
        assert G == (2, 5)[c] and num_samples - 1 > L >= num_samples // 2 and int(got["used"][c, 0]) == L and int(got["groups"][c, 0]) == G
        for family, x in enumerate((xm[used], None, xi[used], None)):
            if x is None:
                continue
            ranks = numpy_midranks(x)
            for b in range(num_branches):
                for f, v in ((family, x[:, b]), (family + 1, ranks[:, b])):
                    rec = got["family"][c, b, f]
                    if is_na(rec["stat"]):
                        continue
                    assert 1.0 - float(rec["eta2"]) >= 0.5, (c, b, f, rec)
                    groups = [v[lam == g] for g in range(G)]
                    if f % 2 == 0:
                        note(worst, "F", relative(float(rec["stat"]), anova_f(v, lam, sizes)))
                        if scipy_stats is not None and (num_branches < 100 or b % 8 == 0):
                            note(worst, "f_oneway", relative(float(rec["stat"]), float(scipy_stats.f_oneway(*groups).statistic)))
                    else:
                        note(worst, "H", relative(float(rec["stat"]), kruskal_h(v, lam, sizes)))
                        if scipy_stats is not None and (num_branches < 100 or b % 8 == 0):
                            note(worst, "kruskal", relative(float(rec["stat"]), float(scipy_stats.kruskal(*groups).statistic)))
                    checked += 1
    print(num_branches, num_samples, kind, "checked", checked, {k: f"{v:.2e}" for k, v in worst.items()})
    assert checked > 2 * num_branches
    assert worst["F"] <= F_BOUND and worst["H"] <= H_BOUND, worst
    if scipy_stats is not None:
        assert worst["f_oneway"] <= F_BOUND and worst["kruskal"] <= H_BOUND, worst


@pytest.mark.parametrize("kind", ["dense", "sparser"])
@pytest.mark.parametrize("num_branches, num_samples", CASES)
def test_pseudo_f_and_r2_are_anderson_s(num_branches, num_samples, kind):
    mass, first, bl, labels = textbook_case(num_branches, num_samples, kind)
    got = cohort_mod.permanova_host(mass, first, bl, labels, 1, 1, False, with_ssw=False).records
    kr = cohort_mod.kr_host(mass, first, bl)
    total, worst = cohort_mod.totals_of(mass), {}
    for c in range(labels.shape[1]):
        used, lam, sizes = column_groups(labels[:, c], total)
        L, G = len(used), len(sizes)
        rec = got[c, 0]
        assert int(rec["used"]) == L and int(rec["groups"]) == G == (2, 5)[c] and not is_na(rec["f"]) and not is_na(rec["r2"])
        d2 = kr[np.ix_(used, used)] ** 2
        upper = np.triu(np.ones((L, L), dtype=bool), 1)
        ss_total = math.fsum(d2[upper].tolist()) / L
        ss_within = math.fsum(math.fsum(d2[upper & np.outer(lam == g, lam == g)].tolist()) / sizes[g] for g in range(G))
        ss_among = ss_total - ss_within
        assert ss_among / ss_total >= 1e-3                    # (the difference ss_total - ss_within loses ten bits at the most)
        note(worst, "pseudo-F", relative(float(rec["f"]), (ss_among / (G - 1)) / (ss_within / (L - G))))
        note(worst, "R2", relative(float(rec["r2"]), ss_among / ss_total))
    print(num_branches, num_samples, kind, {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["pseudo-F"] <= F_BOUND and worst["R2"] <= F_BOUND, worst
