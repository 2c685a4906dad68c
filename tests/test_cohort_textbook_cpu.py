"""The observed statistics of the edge test and of PERMANOVA, and the KR and UniFrac distances, against the textbook forms,
which are not shaped like the rule.

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

The distances that feed PERMANOVA, PCoA, PERMDISP and the model are held to the numpy restatements bit for bit elsewhere, and
those follow the rule's prefix sums over first[b] .. b term by term.  Here kr_host and unifrac_host are held to forms that
walk parent pointers and know neither first[] nor C and B, on random multifurcating trees and stars of 7, 15, 16 and 33
branches (test_cohort_edges_cpu.cohort_edge_tree), six samples, one of them empty, every pair of the other five:
  KR           the optimal-transport cost between the two samples' masses, each branch's mass at its midpoint, under the
               path length between midpoints: scipy.optimize.linprog (HiGHS), where scipy imports;
  weighted     KR over Lozupone's normaliser sum_a (p_a + q_a) depth(a), depth from a's midpoint to the top of the root branch;
  unweighted   Lozupone & Knight's share of the half branches that lead to one sample alone, from the sets of mass-bearing
               branches at or below each half branch, in fractions;
  generalized  Chen's sum with alpha = 0.5 over the same sets, in 60-digit decimals from the integer masses.
The worst relative deviations of the mirror from these forms, measured over those cases: KR 4.5e-16, weighted 3.8e-16,
unweighted 3.5e-16, generalized 7.2e-16; the bounds are 16 times these.  The error of KR relative to itself grows like
1 / weighted UniFrac (compared_pairs), which is asserted to be at least 1e-3 for every compared pair.  Shown once on a
scratch copy of the forms: mass at the upper end of its branch instead of the midpoint, a branch's own mass counted below
both of its halves, or the root branch left out of depth() each move some value by more than 1e-3 relative.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from epik_amd import cohort as cohort_mod, synth
from test_cohort_cpu import numpy_first, random_cells
from test_cohort_edges_cpu import cohort_edge_tree
from test_correlation_cpu import is_na
from test_edgetest_cpu import column_groups, numpy_midranks, numpy_vectors, sparser
from test_permanova_cpu import MISSING

try:
    from scipy import stats as scipy_stats
    from scipy.optimize import linprog
except ImportError:
    scipy_stats = linprog = None

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


# ---- the distances against forms that are not shaped like the rule ---------------------------------------------------
# The rule takes a distance from prefix sums over first[b] .. b: clade mass C and the mass below B per branch, and a sum of
# half lengths times |C_s - C_t| + |B_s - B_t| (or its UniFrac counterparts).  The forms below know nothing of first[], of
# clades as ranges or of C and B: they walk parent pointers.
DISTANCE_TREES = tuple((n, shape) for n in (7, 15, 16, 33) for shape in ("random", "star"))
DISTANCE_SAMPLES = 6
# 16 times the worst relative deviation of the host mirror from the form, measured over DISTANCE_TREES (the docstring)
KR_LP_BOUND = 16 * 4.5e-16
WEIGHTED_BOUND = 16 * 3.8e-16
UNWEIGHTED_BOUND = 16 * 3.5e-16
GENERALIZED_BOUND = 16 * 7.2e-16
WELL_CONDITIONED = 1e-3


def distance_case(num_branches, shape):
    """(parent, bl, first, mass, used): six samples, sample 1 empty, on a tree of test_cohort_edges_cpu."""
    parent, bl = cohort_edge_tree(num_branches, shape)
    rng = np.random.default_rng(2700 + 2 * num_branches + (shape == "star"))
    mass = random_cells(rng, DISTANCE_SAMPLES, num_branches, empty=1, bits=42)
    used = np.flatnonzero(mass.any(axis=1))
    assert used.tolist() == [0, 2, 3, 4, 5]
    return parent, bl, numpy_first(parent), mass, used


def compared_pairs(mass, first, bl, used):
    """The pairs of samples with mass, (S - 1)(S - 2) / 2 of them; each one's weighted UniFrac is at least 1e-3 in the mirror.
    A rounded quotient C_s is off by 2^-53 of its own size, so |C_s - C_t| is off by that much of C_s + C_t and KR, relative to
    itself, by 2^-53 * den / num = 2^-53 / weighted UniFrac: two samples that nearly agree have no digits to compare."""
    weighted = cohort_mod.unifrac_host(mass, first, bl, "weighted")
    pairs = [(int(s), int(t)) for i, s in enumerate(used) for t in used[i + 1:]]
    assert len(pairs) >= (DISTANCE_SAMPLES - 1) * (DISTANCE_SAMPLES - 2) // 2
    assert min(float(weighted[s, t]) for s, t in pairs) >= WELL_CONDITIONED, weighted
    return pairs


def chain(parent, a):
    """a, its parent, ... , the root."""
    out = []
    while a >= 0:
        out.append(int(a))
        a = int(parent[a])
    return out


def midpoint_distance(parent, bl, a, b):
    """The length of the path between the midpoints of the branches a and b: up from each to the first branch that lies above
    both.  Where that is one of the two the path ends at its midpoint; otherwise the two climbs meet at its lower end."""
    if a == b:
        return 0.0
    up_a, up_b = chain(parent, a), chain(parent, b)
    meet = next(x for x in up_a if x in up_b)
    terms = []
    for start, up in ((a, up_a), (b, up_b)):
        if start != meet:
            terms += [bl[start] / 2] + [bl[y] for y in up[1:up.index(meet)]]
    if meet in (a, b):
        terms.append(bl[meet] / 2)
    return math.fsum(terms)


def depth(parent, bl, a):
    """From the midpoint of a to the upper end of the root branch."""
    return math.fsum([bl[a] / 2] + [bl[y] for y in chain(parent, a)[1:]])


def shares(mass_row):
    return mass_row.astype(np.float64) / float(mass_row.sum(dtype=np.uint64))


def transport_cost(p, q, cost):
    """min sum f_ab cost_ab over f >= 0 with row sums p and column sums q (Kantorovich's form of the KR distance)."""
    rows, cols = np.flatnonzero(p), np.flatnonzero(q)
    a_eq = np.zeros((len(rows) + len(cols), len(rows) * len(cols)))
    for i in range(len(rows)):
        a_eq[i, i * len(cols):(i + 1) * len(cols)] = 1.0
    for j in range(len(cols)):
        a_eq[len(rows) + j, j::len(cols)] = 1.0
    res = linprog(cost[np.ix_(rows, cols)].ravel(), A_eq=a_eq, b_eq=np.concatenate([p[rows], q[cols]]), bounds=(0, None), method="highs")
    assert res.status == 0, res.message
    return float(res.fun)


@pytest.mark.parametrize("num_branches, shape", DISTANCE_TREES)
def test_kr_is_the_optimal_transport_cost_between_the_midpoints(num_branches, shape):
    """Where scipy imports, against the optimum of the linear program; everywhere, against the transport problem that needs no
    solver: towards a sample with all its mass on one branch there is one plan, every share along the cost matrix's column
    (shares and costs above 0 only: that sum is as well conditioned as the mirror's, and held to the same bound)."""
    parent, bl, first, mass, used = distance_case(num_branches, shape)
    kr = cohort_mod.kr_host(mass, first, bl)
    n = num_branches
    cost = np.array([[midpoint_distance(parent, bl, a, b) for b in range(n)] for a in range(n)])
    assert (cost == cost.T).all() and (cost[~np.eye(n, dtype=bool)] >= 0).all()
    # a sample on one branch: the only plan moves every share p_a from a to that branch
    for b in (0, n // 2, n - 1):
        point = np.zeros((1, n), np.uint64)
        point[0, b] = 5
        to_point = cohort_mod.kr_host(np.concatenate([mass[used], point]), first, bl)[-1, :-1]
        for i, s in enumerate(used):
            plan = math.fsum((shares(mass[s]) * cost[:, b]).tolist())
            assert relative(float(to_point[i]), plan) <= KR_LP_BOUND, (b, s, float(to_point[i]), plan)
    worst = 0.0
    for s, t in compared_pairs(mass, first, bl, used):
        if linprog is not None:
            worst = max(worst, relative(float(kr[s, t]), transport_cost(shares(mass[s]), shares(mass[t]), cost)))
    print(num_branches, shape, f"KR against the transport optimum {worst:.2e}")
    assert worst <= KR_LP_BOUND, worst


@pytest.mark.parametrize("num_branches, shape", DISTANCE_TREES)
def test_weighted_unifrac_is_kr_over_lozupone_s_normaliser(num_branches, shape):
    """Lozupone et al. (2007): the raw weighted distance over sum_a (p_a + q_a) depth(a), the mass-weighted mean distance of
    either sample from the root."""
    parent, bl, first, mass, used = distance_case(num_branches, shape)
    kr = cohort_mod.kr_host(mass, first, bl)
    weighted = cohort_mod.unifrac_host(mass, first, bl, "weighted")
    depths = [depth(parent, bl, a) for a in range(num_branches)]
    worst = 0.0
    for s, t in compared_pairs(mass, first, bl, used):
        p, q = shares(mass[s]), shares(mass[t])
        normaliser = math.fsum((p[a] + q[a]) * depths[a] for a in range(num_branches))
        worst = max(worst, relative(float(weighted[s, t]), float(kr[s, t]) / normaliser))
    print(num_branches, shape, f"weighted UniFrac against KR over the normaliser {worst:.2e}")
    assert worst <= WEIGHTED_BOUND, worst


def half_branch_sets(parent, mass_row):
    """(upper[b], lower[b]): the branches with mass at or below the upper and the lower half of every branch.  A branch's own
    mass sits at its midpoint: below the upper half, not below the lower one."""
    upper, lower = [set() for _ in parent], [set() for _ in parent]
    for a in np.flatnonzero(mass_row).tolist():
        upper[a].add(a)
        for y in chain(parent, a)[1:]:
            upper[y].add(a)
            lower[y].add(a)
    return upper, lower


@pytest.mark.parametrize("num_branches, shape", DISTANCE_TREES)
def test_unweighted_and_generalized_unifrac_from_descendant_sets(num_branches, shape):
    """Lozupone & Knight (2005): the length of the tree that leads to one sample alone over the length that leads to either;
    Chen et al. (2012) with alpha = 0.5: sum h (x + y)^alpha |x - y| / (x + y) over sum h (x + y)^alpha, x and y the shares
    below a half branch.  The first in fractions, the second in 60-digit decimals from the integer masses; rounded once."""
    import decimal
    parent, bl, first, mass, used = distance_case(num_branches, shape)
    got_u = cohort_mod.unifrac_host(mass, first, bl, "unweighted")
    got_g = cohort_mod.unifrac_host(mass, first, bl, "generalized")
    sets = {int(s): half_branch_sets(parent, mass[s]) for s in used}
    total = {int(s): int(mass[s].sum(dtype=np.uint64)) for s in used}
    worst = {}
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        D = decimal.Decimal
        for s, t in compared_pairs(mass, first, bl, used):
            one, either, num, den = Fraction(0), Fraction(0), D(0), D(0)
            for b in range(num_branches):
                for half in (0, 1):
                    in_s, in_t = sets[s][half][b], sets[t][half][b]
                    if not in_s and not in_t:
                        continue
                    either += Fraction(float(bl[b])) / 2
                    if not in_s or not in_t:
                        one += Fraction(float(bl[b])) / 2
                    x = D(sum(int(mass[s, a]) for a in in_s)) / D(total[s])
                    y = D(sum(int(mass[t, a]) for a in in_t)) / D(total[t])
                    h = D(float(bl[b])) / 2
                    num += h * (x + y).sqrt() * abs(x - y) / (x + y)
                    den += h * (x + y).sqrt()
            note(worst, "unweighted", relative(float(got_u[s, t]), float(one / either)))
            note(worst, "generalized", relative(float(got_g[s, t]), float(num / den)))
    print(num_branches, shape, {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["unweighted"] <= UNWEIGHTED_BOUND and worst["generalized"] <= GENERALIZED_BOUND, worst
