"""Permutations within strata (the strata rule of include/epik_amd.h) for the four permutation tests of a cohort, on the host
mirror and without a GPU: sigma_p restated in numpy from the rule (stratum by stratum, a stable argsort of each stratum's own
keys -- not the one sort by (stratum, key, position) of the C++), put in place of rank_p in the restatements that the four
analyses' own tests have, and compared with the mirror bit for bit; then the properties that do not rest on a restatement:
one stratum, singletons, a factor nested in the strata, the paired line, the exact share over all arrangements, the model
against PERMANOVA; and the C symbols.
"""
import contextlib
import ctypes
import itertools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_edgetest_cpu as edge_cpu
import test_model_cpu as model_cpu
import test_permanova_cpu as nova_cpu
import test_permdisp_cpu as disp_cpu
from epik_amd import capi, cohort as cohort_mod
from test_cohort_cpu import host_bins, numpy_first, numpy_kr, random_cells, same_bits, tree_case  # noqa: F401 (host_bins: a fixture)
from test_permanova_cpu import numpy_keys, numpy_ssw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
MISSING = 0xFFFFFFFF
SAMPLE_COUNTS = (2, 3, 5, 33, 65, 130)


# ---- the rule restated ------------------------------------------------------------------------------------------------------
def numpy_sigma(h, seed, permutations):
    """sigma_p for p = 0 .. P, [P + 1][n], for the strata h[n] of the positions.  Stratum by stratum: its members in ascending
    position; a stable argsort of their keys puts at slot w the member with w_p = w, and that member takes member(h, w)."""
    h = np.asarray(h)
    n = len(h)
    keys = numpy_keys(seed, permutations, n)
    sigma = np.empty((permutations + 1, n), dtype=np.int64)
    for stratum in set(h.tolist()):
        members = np.flatnonzero(h == stratum)
        order = np.argsort(keys[:, members], axis=1, kind="stable")
        inside = np.empty_like(order)
        np.put_along_axis(inside, order, np.broadcast_to(members, order.shape), axis=1)
        sigma[:, members] = inside
    sigma[0] = np.arange(n)
    return sigma


@contextlib.contextmanager
def restated_with(strata, model_used=None):
    """The four analyses' numpy restatements (test_permanova_cpu, test_permdisp_cpu, test_edgetest_cpu, test_model_cpu) with
    sigma_p in place of rank_p: their tests take the samples of their positions, from which the strata follow.  `strata` is by
    sample; None leaves the restatements as they are."""
    if strata is None:
        yield
        return
    strata = np.asarray(strata)
    state = {}

    def labellings(lam, seed, permutations):
        lam = np.asarray(lam)
        return lam[numpy_sigma(state["h"], seed, permutations)]

    nova_test, disp_test, disp_column = nova_cpu.numpy_test, disp_cpu.numpy_test, disp_cpu.numpy_column

    def permanova_test(kr, idx, lam, sizes, permutations, seed):
        state["h"] = strata[np.asarray(idx, dtype=np.int64)]
        return nova_test(kr, idx, lam, sizes, permutations, seed)

    def permdisp_column(kr, idx, lam, sizes):
        state["column"] = np.asarray(idx, dtype=np.int64)
        return disp_column(kr, idx, lam, sizes)

    def permdisp_test(z, r, clip, pos, lam, sizes, permutations, seed):
        state["h"] = strata[state["column"][np.asarray(pos, dtype=np.int64)]]
        return disp_test(z, r, clip, pos, lam, sizes, permutations, seed)

    def arrangements(n, seed, permutations):
        assert n == len(model_used)
        return numpy_sigma(strata[model_used], seed, permutations)

    saved = [(nova_cpu, "numpy_test", nova_test), (nova_cpu, "numpy_labellings", nova_cpu.numpy_labellings),
             (disp_cpu, "numpy_test", disp_test), (disp_cpu, "numpy_column", disp_column),
             (disp_cpu, "numpy_labellings", disp_cpu.numpy_labellings), (model_cpu, "numpy_arrangements", model_cpu.numpy_arrangements)]
    try:
        nova_cpu.numpy_test, nova_cpu.numpy_labellings = permanova_test, labellings
        disp_cpu.numpy_test, disp_cpu.numpy_column, disp_cpu.numpy_labellings = permdisp_test, permdisp_column, labellings
        model_cpu.numpy_arrangements = arrangements
        yield
    finally:
        for module, name, value in saved:
            setattr(module, name, value)


def numpy_permanova(kr, totals, labels, permutations, seed, pairwise, strata):
    with restated_with(strata):
        return nova_cpu.numpy_permanova(kr, totals, labels, permutations, seed, pairwise)


def numpy_permdisp(kr, totals, labels, permutations, seed, pairwise, strata):
    with restated_with(strata):
        return disp_cpu.numpy_permdisp(kr, totals, labels, permutations, seed, pairwise)


def numpy_edgetest(mass, first, labels, permutations, seed, strata):
    """A column at a time: the labellings of a column come from the strata of its used samples."""
    totals = cohort_mod.totals_of(mass)
    parts = []
    for c in range(labels.shape[1]):
        used = np.flatnonzero((totals != 0) & (labels[:, c] != MISSING))

        def labellings(lam, seed, permutations, used=used):
            return np.asarray(lam)[numpy_sigma(np.asarray(strata)[used], seed, permutations)]

        parts.append(edge_cpu.numpy_edgetest(mass, first, labels[:, c:c + 1], permutations, seed,
                                             labellings=edge_cpu.numpy_labellings if strata is None else labellings))
    return cohort_mod.Edgetest(np.concatenate([p.records for p in parts]), np.concatenate([p.stat for p in parts]),
                               np.concatenate([p.max for p in parts]))


def numpy_model(kr, totals, kind, labels, values, permutations, seed, strata):
    kind, labels, values = np.asarray(kind), np.asarray(labels), np.asarray(values, dtype=np.float64)
    present = np.where(kind[None, :] != 0, ~np.isnan(values), labels != MISSING)
    used = np.flatnonzero((np.asarray(totals) != 0) & present.all(axis=1))
    with restated_with(strata, used):
        return model_cpu.numpy_model(kr, totals, kind, labels, values, permutations, seed)


def strata_layouts(num_samples):
    """Singletons; pairs; contiguous blocks; interleaved; one huge stratum plus singletons.  The ids are no 0 .. H - 1 and
    come in no order: only their equality may matter."""
    i = np.arange(num_samples)
    block = max(1, (num_samples + 3) // 4)
    layouts = {"singletons": i, "pairs": i // 2, "blocks": i // block, "interleaved": i % 3,
               "huge": np.where(i % 5 == 4, i + 1, 0)}
    scramble = lambda h: ((h.astype(np.uint64) * 2654435761 + 0xFFFFFF00) % (1 << 32)).astype(np.uint32)  # injective on the ids used
    return {name: scramble(h) for name, h in layouts.items()}


def strata_case(num_samples, seed=7, tree_name="tree15"):
    """Cells with one sample without mass, and the columns of labels of the four analyses: two balanced groups; three groups
    with missing labels (so strata lose members, also to the pairwise sub-lists); groups that alternate within pairs."""
    parent, bl = tree_case(tree_name)
    first = numpy_first(parent)
    rng = np.random.default_rng(seed * 1000 + num_samples)
    mass = random_cells(rng, num_samples, len(parent), empty=1, bits=42)
    i = np.arange(num_samples)
    three = np.where(rng.random(num_samples) < 0.2, MISSING, rng.integers(0, 3, num_samples))
    labels = np.ascontiguousarray(np.array([rng.permutation(i % 2), three, i % 2], dtype=np.uint32).T)
    return mass, first, bl, labels, rng


def model_design(labels, rng):
    """A factor with missing labels, a numeric term with a missing value, a second factor."""
    s = labels.shape[0]
    values = rng.normal(size=s)
    if s > 4:
        values[3] = np.nan
    return model_cpu.design(("f", labels[:, 1]), ("n", values), ("f", labels[:, 0]))


def same_records(got, want):
    assert got.records.tobytes() == want.records.tobytes()
    for name in ("ssw", "stat", "max", "group_ss", "group_mean", "z", "aliased"):
        a, b = getattr(got, name, None), getattr(want, name, None)
        if a is not None and b is not None:
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), name
    if hasattr(got, "info"):
        assert got.info.tobytes() == want.info.tobytes()
    return True


# ---- 1. the restatement itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_samples", SAMPLE_COUNTS)
def test_sigma_keeps_every_stratum_and_its_labels(num_samples):
    """(d) on the restatement: sigma_p is a bijection that maps every stratum onto itself, so the multiset of labels of a
    stratum is the same for every p; one stratum gives rank_p; sigma is the count of the rule."""
    rng = np.random.default_rng(num_samples)
    lam = rng.integers(0, 4, num_samples)
    for name, h in strata_layouts(num_samples).items():
        sigma = numpy_sigma(h, 99, 20)
        assert (np.sort(sigma, axis=1) == np.arange(num_samples)[None, :]).all(), name
        assert (h[sigma] == h[None, :]).all(), name
        mu = lam[sigma]
        for stratum in set(h.tolist()):
            members = h == stratum
            assert (np.sort(mu[:, members], axis=1) == np.sort(lam[members])[None, :]).all(), name
        keys = numpy_keys(99, 20, num_samples)
        for p in (1, 20):                                                       # the rule's own words: w_p by counting, then member
            for i in range(num_samples):
                w = sum(h[j] == h[i] and (keys[p, j], j) < (keys[p, i], i) for j in range(num_samples))
                assert sigma[p, i] == np.flatnonzero(h == h[i])[w]
    one = numpy_sigma(np.full(num_samples, 77), 99, 20)
    assert np.array_equal(one, model_cpu.numpy_arrangements(num_samples, 99, 20))


# ---- 2. the host mirror against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("num_samples", SAMPLE_COUNTS)
def test_host_equals_the_numpy_restatement_bit_for_bit(num_samples):
    mass, first, bl, labels, rng = strata_case(num_samples)
    kr, totals = numpy_kr(mass, first, bl), cohort_mod.totals_of(mass)
    kind, mlabels, values = model_design(labels, rng)
    for name, strata in strata_layouts(num_samples).items():
        permutations = 65 if name in ("pairs", "huge") else 9
        seed = int(rng.integers(0, 1 << 63)) * 2 + 1
        what = (num_samples, name)
        for pairwise in (False, True):
            got = cohort_mod.permanova_host(mass, first, bl, labels, permutations, seed, pairwise, strata=strata)
            want = numpy_permanova(kr, totals, labels, permutations, seed, pairwise, strata)
            nova_cpu.same_permanova(got, want, what)
            nova_cpu.same_permanova(cohort_mod.permanova_kr_host(kr, totals, labels, permutations, seed, pairwise, strata=strata), want, what)
            # (d) through the mirror: SSW of a labelling depends on the labelling alone, so the mirror's labellings are the
            # restatement's, whose strata keep their labels
            got = cohort_mod.permdisp_host(mass, first, bl, labels, permutations, seed, pairwise, strata=strata)
            want = numpy_permdisp(kr, totals, labels, permutations, seed, pairwise, strata)
            disp_cpu.same_permdisp(got, want, what)
            disp_cpu.same_permdisp(cohort_mod.permdisp_kr_host(kr, totals, labels, permutations, seed, pairwise, strata=strata), want, what)
        edge_cpu.same_edgetest(cohort_mod.edgetest_host(mass, first, labels, permutations, seed, strata=strata),
                               numpy_edgetest(mass, first, labels, permutations, seed, strata), what)
        want = numpy_model(kr, totals, kind, mlabels, values, permutations, seed, strata)
        model_cpu.same_model(cohort_mod.model_host(mass, first, bl, kind, mlabels, values, permutations, seed, strata=strata), want, what)
        model_cpu.same_model(cohort_mod.model_kr_host(kr, totals, kind, mlabels, values, permutations, seed, strata=strata), want, what)


# ---- 3. properties that rest on no restatement ------------------------------------------------------------------------------
def all_four(mass, first, bl, labels, design, permutations, seed, strata, pairwise=True):
    return (cohort_mod.permanova_host(mass, first, bl, labels, permutations, seed, pairwise, strata=strata),
            cohort_mod.permdisp_host(mass, first, bl, labels, permutations, seed, pairwise, strata=strata),
            cohort_mod.edgetest_host(mass, first, labels, permutations, seed, strata=strata),
            cohort_mod.model_host(mass, first, bl, *design, permutations, seed, strata=strata))


@pytest.mark.parametrize("num_samples", (5, 33, 130))
def test_one_stratum_gives_the_bytes_without_strata(num_samples):
    """(a)"""
    mass, first, bl, labels, rng = strata_case(num_samples)
    design = model_design(labels, rng)
    plain = all_four(mass, first, bl, labels, design, 33, 5, None)
    for stratum in (0, 0xFFFFFFFF):
        for got, want in zip(all_four(mass, first, bl, labels, design, 33, 5, np.full(num_samples, stratum, np.uint32)), plain):
            same_records(got, want)
    # and renumbering the strata changes no byte: only equality enters the rule
    h = strata_layouts(num_samples)["interleaved"]
    other = (0xFFFFFFFF - h.astype(np.int64) // 3).astype(np.uint32)
    for got, want in zip(all_four(mass, first, bl, labels, design, 33, 5, h), all_four(mass, first, bl, labels, design, 33, 5, other)):
        same_records(got, want)


@pytest.mark.parametrize("nested", (False, True))
def test_nothing_to_permute_gives_p_one(nested):
    """(b) every sample a stratum of its own, and (c) a factor that is constant inside every stratum: every permuted statistic
    is the observed one bit for bit, the count is P and p = 1 (PERMDISP, whose permuted statistic is another: see below)."""
    num_samples, permutations = 33, 40
    mass, first, bl, labels, rng = strata_case(num_samples)
    i = np.arange(num_samples)
    if nested:
        strata = (i // 3).astype(np.uint32)
        labels = np.ascontiguousarray(np.array([(i // 3) % 2, (i // 6) % 3, (i // 3) % 5], dtype=np.uint32).T)
    else:
        strata = (1000 - i).astype(np.uint32)
    design = model_cpu.design(("f", labels[:, 0]), ("f", labels[:, 1]))
    nova, disp, edge, model = all_four(mass, first, bl, labels, design, permutations, 11, strata)
    defined = ~np.isnan(nova.records["p"])
    assert defined[:, 0].all() and defined.sum() > 3
    assert (nova.ssw[defined].view(U64) == nova.ssw[defined][:, :1].view(U64)).all()
    assert (nova.records["at_most"][defined] == permutations).all() and (nova.records["p"][defined] == 1.0).all()
    # PERMDISP permutes the residuals r, and its observed statistic is that of z: every permuted statistic is eta_r of the
    # residuals where they are, one value whatever p (0 but for rounding: a group's residuals sum to nothing)
    defined = ~np.isnan(disp.records["p"])
    assert defined[:, 0].all() and defined.sum() > 3
    assert (disp.stat[defined][:, 1:].view(U64) == disp.stat[defined][:, 1:2].view(U64)).all()
    assert np.isin(disp.records["at_least"][defined], (0, permutations)).all() and (disp.stat[defined][:, 1] < 1e-20).all()
    fam = edge.records["family"]
    defined = ~np.isnan(fam["p"])
    assert defined.sum() > 10 and (fam["at_least"][defined] == permutations).all() and (fam["p"][defined] == 1.0).all()
    assert (fam["p_adj"][defined] == 1.0).all()
    rows = ~np.isnan(edge.stat[..., 0])
    assert (edge.stat[rows].view(U64) == edge.stat[rows][:, :1].view(U64)).all()
    tested = model.records["df"] > 0
    assert tested.sum() == 3 and (model.records["at_least"][tested] == permutations).all() and (model.records["p"][tested] == 1.0).all()
    assert (model.stat[tested].view(U64) == model.stat[tested][:, :1].view(U64)).all()


def paired_line():
    """Eight subjects on a line at x = 0, 10, .., 70, each sampled twice, the second sample at x + 1; the treatment is the
    factor, the subject the stratum."""
    x = np.array([[10.0 * i, 10.0 * i + 1.0] for i in range(8)]).ravel()
    return np.abs(x[:, None] - x[None, :]), np.ones(16, U64), np.tile([0, 1], 8).astype(np.uint32)[:, None].copy(), np.repeat(np.arange(8), 2)


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_the_paired_line_needs_its_strata(seed):
    """(e) Free shuffles drown the treatment in the subjects' spread; within subjects only 2 of the 256 sign patterns reach
    the observed SSW."""
    kr, totals, labels, strata = paired_line()
    free = cohort_mod.permanova_kr_host(kr, totals, labels, 999, seed).records[0, 0]
    within = cohort_mod.permanova_kr_host(kr, totals, labels, 999, seed, strata=strata).records[0, 0]
    print("paired line, seed", seed, "free p", free["p"], "within subjects p", within["p"])
    assert within["p"] < 0.05 and free["p"] > 0.5
    assert same_bits(free["ss_within"], within["ss_within"]) and same_bits(free["f"], within["f"])


def test_the_share_of_permutations_follows_the_exact_share_of_all_36_arrangements():
    """(f) L = 6 in the strata {0, 1, 2} and {3, 4, 5}: q is the share of the 3! * 3! = 36 arrangements with SSW <= SSW_0.
    at_most summed over 40 seeds of 999 draws is a sum of D = 39 960 draws; were they independent and uniform its share would
    lie within 5 sqrt(q (1 - q) / D) of q but for one run in two million (the margin of the unstratified test).  The seeds
    are fixed: the check is deterministic."""
    parent, bl = tree_case("tree15")
    first = numpy_first(parent)
    mass = random_cells(np.random.default_rng(11006), 6, len(parent), bits=42)
    mass[mass.sum(axis=1) == 0] = 1
    labels = np.array([[0, 1, 1, 0, 1, 0]], dtype=np.uint32).T.copy()
    strata = np.array([8, 8, 8, 2, 2, 2], dtype=np.uint32)
    kr = numpy_kr(mass, first, bl)
    lam = labels[:, 0].astype(np.int64)
    every = np.array([lam[list(a) + [3 + v for v in b]] for a in itertools.permutations(range(3)) for b in itertools.permutations(range(3))])
    ssw, _ = numpy_ssw(kr * kr, np.vstack([lam[None, :], every]), [3, 3])
    q = float((ssw[1:] <= ssw[0]).mean())
    assert len(every) == 36 and 0.0 < q < 1.0
    draws = 40 * 999
    at_most = sum(int(cohort_mod.permanova_host(mass, first, bl, labels, 999, seed, with_ssw=False, strata=strata).records["at_most"][0, 0])
                  for seed in range(1, 41))
    share = at_most / draws
    print("q", q, "share", share, "bound", 5 * np.sqrt(q * (1 - q) / draws))
    assert abs(share - q) <= 5 * np.sqrt(q * (1 - q) / draws)


@pytest.mark.parametrize("num_samples", (6, 12, 40))
def test_a_stratified_model_of_one_factor_is_stratified_permanova(num_samples):
    """(g) As test_model_cpu's test of the pair without strata, with its bound: the observed sums agree within it, and the
    same arrangements put the permutations in the same order wherever neither side ties."""
    parent, bl = tree_case("tree15")
    first = numpy_first(parent)
    for trial in range(4):
        rng = np.random.default_rng(4400 + 10 * num_samples + trial)
        mass = random_cells(rng, num_samples, len(parent), empty=trial, bits=42)
        kr, totals = cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass)
        groups = rng.permutation(np.arange(num_samples) % (2 + trial % 2)).astype(np.uint32)
        groups[rng.integers(0, num_samples)] = MISSING
        strata = (np.arange(num_samples) // (2 + trial)).astype(np.uint32)
        kind, labels, values = model_cpu.design(("f", groups))
        permutations, seed = 199, int(rng.integers(0, 1 << 63))
        model = cohort_mod.model_kr_host(kr, totals, kind, labels, values, permutations, seed, strata=strata)
        permanova = cohort_mod.permanova_kr_host(kr, totals, labels, permutations, seed, strata=strata)
        record = permanova.records[0, 0]
        among = record["ss_total"] - record["ss_within"]
        for got, want in ((model.records["ss"][0], among), (model.records["r2"][0], record["r2"]), (model.info["ss_total"], record["ss_total"]),
                          (model.records["f"][0], record["f"])):
            assert abs(got - want) / abs(want) <= model_cpu.PERMANOVA_BOUND, (num_samples, trial, got, want)
        f, ssw = model.stat[0], permanova.ssw[0, 0]
        for p, q in itertools.combinations(range(0, permutations + 1, 7), 2):
            if abs(ssw[p] - ssw[q]) > 1e-9 * abs(record["ss_total"]):
                assert (f[p] > f[q]) == (ssw[p] < ssw[q]), (num_samples, trial, p, q)
        clear = np.abs(ssw[1:] - ssw[0]) > 1e-9 * abs(record["ss_total"])
        assert ((f[1:] >= f[0]) == (ssw[1:] <= ssw[0]))[clear].all()
        free = cohort_mod.permanova_kr_host(kr, totals, labels, permutations, seed)
        assert not same_bits(free.ssw[0, 0, 1:], ssw[1:])                       # (the strata did change the shuffles)


# ---- 4. the C ABI -----------------------------------------------------------------------------------------------------------
STRATA_SYMBOLS = [f"epik_amd_cohort_{a}_strata{e}" for a in ("permanova", "permdisp", "model") for e in ("_device", "", "_host", "_kr_host")] + \
                 [f"epik_amd_cohort_edgetest_strata{e}" for e in ("_device", "", "_host")]


def test_strata_symbols_exist_and_refuse_what_their_siblings_refuse():
    lib = capi.load()
    for name in STRATA_SYMBOLS:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert capi.ABI_VERSION == 3 and len(STRATA_SYMBOLS) == 15
    err = lambda: lib.epik_amd_last_error().decode()
    labels, strata = np.zeros((4, 1), np.uint32), np.zeros(4, np.uint32)
    for analysis in ("permanova", "permdisp", "model", "edgetest"):               # no cohort: before anything is touched
        entry = getattr(lib, f"epik_amd_cohort_{analysis}_strata_device")
        args = [None] * (len(entry.argtypes) - 1) + [strata.ctypes.data]
        args = [0 if t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32) else a for a, t in zip(args, entry.argtypes)]
        assert entry(*args) == capi.ERR_INVALID and "null cohort" in err()
    first = cohort_mod.first_of([2, 2, -1])
    cells, bl = np.ones((4, 3), U64), np.ones(3)
    out, group_ss = np.zeros(1, dtype=capi.PERMANOVA), np.zeros(capi.PERMANOVA_MAX_GROUPS)
    call = lambda m=cells.ctypes.data, c=1, p=9, o=out.ctypes.data: lib.epik_amd_cohort_permanova_strata_host(
        m, 4, 3, first.ctypes.data, bl.ctypes.data, 0, labels.ctypes.data, c, p, 1, 0, o, None, group_ss.ctypes.data, strata.ctypes.data)
    assert call() == capi.OK
    assert call(m=None) == capi.ERR_INVALID and "null argument" in err()
    assert call(o=None) == capi.ERR_INVALID and "null argument" in err()
    assert call(c=65) == capi.ERR_INVALID and "num_columns = 65" in err()
    assert call(p=0) == capi.ERR_INVALID and "num_permutations = 0" in err()
    labels[2, 0] = 256
    assert call() == capi.ERR_INVALID and "the label 256 is not below 256" in err()
    # one refusal each of the other analyses' host entries, as their siblings refuse
    labels[2, 0] = 32
    kr, totals, ptr = np.zeros((4, 4)), np.ones(4, U64), (lambda a: a.ctypes.data)
    disp = cohort_mod._permdisp_buffers(1, 4, 9, False, True)
    assert lib.epik_amd_cohort_permdisp_strata_host(ptr(cells), 4, 3, ptr(first), ptr(bl), 0, ptr(labels), 1, 9, 1, 0, ptr(disp.records),
                                                    ptr(disp.stat), ptr(disp.group_mean), ptr(disp.z), ptr(strata)) == capi.ERR_INVALID
    assert "the label 32 is not below 32" in err()
    assert lib.epik_amd_cohort_permdisp_strata_kr_host(ptr(kr), ptr(totals), 4, ptr(labels), 1, 0, 1, 0, ptr(disp.records), ptr(disp.stat),
                                                       ptr(disp.group_mean), ptr(disp.z), ptr(strata)) == capi.ERR_INVALID
    assert "num_permutations = 0" in err()
    edge = cohort_mod.Edgetest(*cohort_mod._edgetest_buffers(1, 3, 9, True, True))
    assert lib.epik_amd_cohort_edgetest_strata_host(ptr(cells), 4, 3, ptr(first), ptr(labels), 1, 9, 1, ptr(edge.records), ptr(edge.stat),
                                                    ptr(edge.max), ptr(strata)) == capi.ERR_INVALID
    assert "the label 32 is not below 32" in err()
    assert lib.epik_amd_cohort_edgetest_strata_host(ptr(cells), 4, 3, ptr(first), None, 1, 9, 1, ptr(edge.records), None, None,
                                                    ptr(strata)) == capi.ERR_INVALID and "null argument" in err()
    kind, mlabels, values = model_cpu.design(("f", [0, 1, 0, 1]))
    records, info, stat, aliased = cohort_mod._model_buffers(1, 9, True)
    model_args = (ptr(kind), ptr(mlabels), ptr(values))
    assert lib.epik_amd_cohort_model_strata_host(ptr(cells), 4, 3, ptr(first), ptr(bl), 0, *model_args, 17, 9, 1, ptr(records), ptr(info),
                                                 ptr(stat), ptr(aliased), ptr(strata)) == capi.ERR_INVALID and "num_terms = 17" in err()
    assert lib.epik_amd_cohort_model_strata_kr_host(ptr(kr), ptr(totals), 4, *model_args, 1, 1_000_000, 1, ptr(records), ptr(info), ptr(stat),
                                                    ptr(aliased), ptr(strata)) == capi.ERR_INVALID and "num_permutations = 1000000" in err()
    assert lib.epik_amd_cohort_model_strata_kr_host(ptr(kr), ptr(totals), 4, *model_args, 1, 9, 1, ptr(records), None, ptr(stat),
                                                    ptr(aliased), ptr(strata)) == capi.ERR_INVALID and "null argument" in err()
    with pytest.raises(ValueError, match="strata must be"):
        cohort_mod.permanova_kr_host(np.zeros((4, 4)), np.ones(4, U64), np.zeros((4, 1), np.uint32), strata=np.zeros(3))


def test_null_strata_give_the_bytes_of_the_entries_without_them():
    """The `_strata` entries with strata == NULL against the entries that existed before, byte for byte."""
    lib = capi.load()
    mass, first, bl, labels, rng = strata_case(33)
    kr, totals = numpy_kr(mass, first, bl), cohort_mod.totals_of(mass)
    s, n, m, permutations, seed = 33, mass.shape[1], labels.shape[1], 21, 9
    ptr = lambda a: a.ctypes.data
    want = cohort_mod.permanova_host(mass, first, bl, labels, permutations, seed, True)
    got = cohort_mod.Permanova(*cohort_mod._permanova_buffers(m, permutations, True, True))
    capi.check(lib.epik_amd_cohort_permanova_strata_host(ptr(mass), s, n, ptr(first), ptr(bl), 0, ptr(labels), m, permutations, seed, 1,
                                                         ptr(got.records), ptr(got.ssw), ptr(got.group_ss), None))
    same_records(got, want)
    got = cohort_mod.Permanova(*cohort_mod._permanova_buffers(m, permutations, True, True))
    capi.check(lib.epik_amd_cohort_permanova_strata_kr_host(ptr(kr), ptr(totals), s, ptr(labels), m, permutations, seed, 1,
                                                            ptr(got.records), ptr(got.ssw), ptr(got.group_ss), None))
    same_records(got, want)
    want = cohort_mod.permdisp_host(mass, first, bl, labels, permutations, seed, True)
    got = cohort_mod._permdisp_buffers(m, s, permutations, True, True)
    capi.check(lib.epik_amd_cohort_permdisp_strata_host(ptr(mass), s, n, ptr(first), ptr(bl), 0, ptr(labels), m, permutations, seed, 1,
                                                        ptr(got.records), ptr(got.stat), ptr(got.group_mean), ptr(got.z), None))
    same_records(got, want)
    got = cohort_mod._permdisp_buffers(m, s, permutations, True, True)
    capi.check(lib.epik_amd_cohort_permdisp_strata_kr_host(ptr(kr), ptr(totals), s, ptr(labels), m, permutations, seed, 1,
                                                           ptr(got.records), ptr(got.stat), ptr(got.group_mean), ptr(got.z), None))
    same_records(got, want)
    want = cohort_mod.edgetest_host(mass, first, labels, permutations, seed)
    got = cohort_mod.Edgetest(*cohort_mod._edgetest_buffers(m, n, permutations, True, True))
    capi.check(lib.epik_amd_cohort_edgetest_strata_host(ptr(mass), s, n, ptr(first), ptr(labels), m, permutations, seed, ptr(got.records),
                                                        ptr(got.stat), ptr(got.max), None))
    same_records(got, want)
    kind, mlabels, values = model_design(labels, rng)
    want = cohort_mod.model_host(mass, first, bl, kind, mlabels, values, permutations, seed)
    for entry, head in ((lib.epik_amd_cohort_model_strata_host, (ptr(mass), s, n, ptr(first), ptr(bl), 0)),
                        (lib.epik_amd_cohort_model_strata_kr_host, (ptr(kr), ptr(totals), s))):
        records, info, stat, aliased = cohort_mod._model_buffers(len(kind), permutations, True)
        capi.check(entry(*head, ptr(kind), ptr(mlabels), ptr(values), len(kind), permutations, seed, ptr(records), ptr(info), ptr(stat),
                         ptr(aliased), None))
        same_records(cohort_mod.Model(records, info[0], stat, aliased), want)


# ---- 5. the host code stand-alone -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitized", [False, True])
def test_host_test_binary_strata_modes_are_the_library_s(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    seed = 12345678901234567890
    paths = {name: str(tmp_path / f"{name}.bin") for name in ("out", "mass", "labels", "strata", "design")}

    def run(mode, *more):
        done = subprocess.run([binary, mode, paths["out"], paths["mass"], *more], capture_output=True, text=True)
        assert done.returncode == 0 and not done.stderr, (mode, done.stderr)
        with open(paths["out"], "rb") as fh:
            return fh.read()

    for num_samples in (2, 5, 33, 65):
        mass, first, bl, labels, rng = strata_case(num_samples, seed=9)
        nova_cpu._cells_input(paths["mass"], mass, first, bl)
        labels.tofile(paths["labels"])
        kind, mlabels, values = model_design(labels, rng)
        with open(paths["design"], "wb") as fh:
            fh.write(np.array([len(kind)], dtype="<u8").tobytes() + kind.tobytes() + mlabels.tobytes() + values.tobytes())
        for name, strata in strata_layouts(num_samples).items():
            if name not in ("pairs", "interleaved", "huge"):
                continue
            strata.tofile(paths["strata"])
            permutations = str(int(rng.integers(1, 30)))
            p, what = int(permutations), (num_samples, name)
            for pairwise in (0, 1):
                want = cohort_mod.permanova_host(mass, first, bl, labels, p, seed, bool(pairwise), strata=strata)
                got = run("permanova-strata", paths["labels"], paths["strata"], permutations, str(seed), str(pairwise))
                assert got == want.records.tobytes() + want.ssw.tobytes() + want.group_ss.tobytes(), what
                want = cohort_mod.permdisp_host(mass, first, bl, labels, p, seed, bool(pairwise), strata=strata)
                got = run("permdisp-strata", paths["labels"], paths["strata"], permutations, str(seed), str(pairwise))
                assert got == want.records.tobytes() + want.stat.tobytes() + want.group_mean.tobytes() + want.z.tobytes(), what
            want = cohort_mod.edgetest_host(mass, first, labels, p, seed, strata=strata)
            got = run("edgetest-strata", paths["labels"], paths["strata"], permutations, str(seed))
            assert got == want.records.tobytes() + want.stat.tobytes() + want.max.tobytes(), what
            want = cohort_mod.model_host(mass, first, bl, kind, mlabels, values, p, seed, strata=strata)
            got = run("model-strata", paths["design"], paths["strata"], permutations, str(seed))
            assert got == want.records.tobytes() + want.info.tobytes() + want.stat.tobytes() + want.aliased.tobytes(), what
    np.zeros(3, np.uint32).tofile(paths["strata"])                              # a strata file of another length is refused
    done = subprocess.run([binary, "model-strata", paths["out"], paths["mass"], paths["design"], paths["strata"], "9", "1"],
                          capture_output=True, text=True)
    assert done.returncode == 1 and "strata file" in done.stderr


# ---- 6. the strata file, the four files' field, the drivers' flags ----------------------------------------------------------
STRATA_NAMES = ["a", "skin 3", "it's", "none", "q"]
STRATA_FILE = ("# who is who\nsample\tsubject\tbatch\n" "q\tmary\tb1\n" "a\tjohn smith\tb1\n" "other\tx\ty\n" "skin 3\tmary\tb2\n"
               "it's\t17\tb2\n" "none\tjohn smith\tNA\n")


def cpp_strata(host_bins, tmp_path, path, column, names=STRATA_NAMES):
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names))
    return subprocess.run([os.path.join(host_bins, "cohort_test"), "strata-read", str(tmp_path / "strata.bin"), str(tmp_path / "names.txt"),
                           str(path), column or "-"], capture_output=True, text=True)


def test_the_strata_reader_and_its_errors_with_line_and_column(host_bins, tmp_path):
    path = tmp_path / "strata.tsv"
    path.write_text(STRATA_FILE)
    strata, name = cohort_mod.read_strata(str(path), STRATA_NAMES, "subject")
    assert name == "subject" and list(strata) == [1, 0, 2, 1, 0] and strata.dtype == np.uint32      # mary 0, john smith 1, 17 2
    run = cpp_strata(host_bins, tmp_path, path, "subject")
    assert run.returncode == 0 and not run.stderr, run.stderr
    assert (tmp_path / "strata.bin").read_bytes() == strata.tobytes() + b"subject"
    # every error names the flag's file, the line and, where there is one, the column -- from Python and from C++
    cases = [("batch", STRATA_FILE, ("line 8", "column batch", "'none'", "no stratum")),
             (None, STRATA_FILE, ("2 columns", "--cohort-strata-column")),
             ("who", STRATA_FILE, ("--cohort-strata-column", "no column 'who'")),
             ("subject", STRATA_FILE.replace("q\tmary\tb1\n", "q\tmary\n"), ("line 3", "2 fields, not 3")),
             ("subject", STRATA_FILE + "a\tz\tb9\n", ("line 9", "'a' is given twice", "line 4")),
             ("subject", STRATA_FILE.replace("it's\t17\tb2\n", ""), ("no line for the sample 'it's'",)),
             ("subject", STRATA_FILE.replace("sample\tsubject", "name\tsubject"), ("line 2", "must begin with 'sample'"))]
    for column, text, words in cases:
        path.write_text(text)
        with pytest.raises(ValueError) as e:
            cohort_mod.read_strata(str(path), STRATA_NAMES, column)
        assert all(w in str(e.value) for w in words), (column, str(e.value))
        run = cpp_strata(host_bins, tmp_path, path, column)
        assert run.returncode == 1 and all(w in run.stderr for w in words) and "--cohort-strata" in run.stderr, (column, run.stderr)
    # no cap on the labels: 1 024 samples in 512 pairs; one column needs no name
    names = [f"s{i}" for i in range(1024)]
    path.write_text("sample\tsubject\n" + "".join(f"{n}\tsubject {i // 2}\n" for i, n in enumerate(names)))
    strata, name = cohort_mod.read_strata(str(path), names)
    assert name == "subject" and np.array_equal(strata, np.arange(1024) // 2)
    run = cpp_strata(host_bins, tmp_path, path, None, names)
    assert run.returncode == 0 and (tmp_path / "strata.bin").read_bytes() == strata.tobytes() + b"subject"


@pytest.mark.parametrize("sanitized", [False, True])
def test_the_four_files_carry_the_field_from_python_and_from_cpp_and_read_back(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    num_samples, permutations, seed = 9, 19, 3
    mass, first, bl, labels, rng = strata_case(num_samples)
    names = [f"s {i}" for i in range(num_samples)]
    totals = cohort_mod.totals_of(mass)
    strata = (np.arange(num_samples) // 3).astype(np.uint32)
    columns, label_names = ["state", "site", "arm"], [["a", "b"], ["x", "y", "z"], ["p", "q"]]
    nova = cohort_mod.permanova_host(mass, first, bl, labels, permutations, seed, True, strata=strata)
    disp = cohort_mod.permdisp_host(mass, first, bl, labels, permutations, seed, True, metric="weighted", strata=strata)
    edge = cohort_mod.edgetest_host(mass, first, labels, permutations, seed, strata=strata)
    kind, mlabels, values = model_design(labels, rng)
    model = cohort_mod.model_host(mass, first, bl, kind, mlabels, values, permutations, seed, strata=strata)
    texts = {
        "permanova": lambda s: cohort_mod.format_permanova_tsv(names, totals, columns, label_names, labels, permutations, seed, True,
                                                               nova.records, nova.group_ss, strata=s),
        "permdisp": lambda s: cohort_mod.format_permdisp_tsv(names, totals, columns, label_names, labels, permutations, seed, True,
                                                             disp.records, disp.group_mean, disp.z, distance="weighted", strata=s),
        "edgetest": lambda s: cohort_mod.format_edgetest_tsv(names, totals, columns, label_names, labels, permutations, seed, edge.records,
                                                             strata=s),
        "model": lambda s: cohort_mod.format_model_tsv(names, totals, ["site", "age", "state"], kind, [label_names[1], [], label_names[0]],
                                                       mlabels, values, permutations, seed, model, strata=s)}
    readers = {"permanova": cohort_mod.read_permanova_tsv, "permdisp": cohort_mod.read_permdisp_tsv, "edgetest": cohort_mod.read_edgetest_tsv,
               "model": cohort_mod.read_model_tsv}
    for what, text in texts.items():
        plain, named = text(None), text("the subject")
        first_line = plain.split("\n", 1)[0]
        assert named == first_line + "\tstrata=the subject\n" + plain.split("\n", 1)[1] and text("") == plain, what
        assert ("\tdistance=weighted\tstrata=the subject\n" in named) == (what == "permdisp")
        (tmp_path / "plain.tsv").write_text(plain)
        run = subprocess.run([binary, "strata-field", str(tmp_path / "cpp.tsv"), str(tmp_path / "plain.tsv"), "the subject"],
                             capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (what, run.stderr)
        assert (tmp_path / "cpp.tsv").read_bytes() == named.encode(), what
        back, back_plain = readers[what](str(tmp_path / "cpp.tsv")), readers[what](str(tmp_path / "plain.tsv"))
        assert back[-1]["strata"] == "the subject" and "strata" not in back_plain[-1], what
        assert {k: v for k, v in back[-1].items() if k != "strata"}.keys() == back_plain[-1].keys(), what
    # a nested factor is found: constant inside every stratum of its used samples
    assert cohort_mod.constant_within_strata(np.arange(num_samples) // 3 % 2, totals, strata)
    assert not cohort_mod.constant_within_strata(labels[:, 2], totals, strata)


@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_drivers_refuse_the_flags_and_read_the_strata_before_the_database(host_bins, tmp_path, binary):
    out = tmp_path / "out"
    out.mkdir()
    (tmp_path / "samples.list").write_text("".join(f"{n}\tin/{i}.fasta\n" for i, n in enumerate(STRATA_NAMES)))
    (tmp_path / "in").mkdir()
    for i in range(len(STRATA_NAMES)):
        (tmp_path / "in" / f"{i}.fasta").write_text(">r\nACGTACGTACGT\n")
    (tmp_path / "strata.tsv").write_text(STRATA_FILE)
    (tmp_path / "factors.tsv").write_text("sample\tstate\n" + "".join(f"{n}\t{'ab'[i % 2]}\n" for i, n in enumerate(STRATA_NAMES)))
    base = [os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "samples.list"), "-o", str(out)]
    strata = ["--cohort-strata", str(tmp_path / "strata.tsv")]
    test = ["--cohort", "--cohort-permanova", str(tmp_path / "factors.tsv")]

    def refused(extra, *words):
        run = subprocess.run(base + extra, capture_output=True, text=True)
        assert run.returncode == 255 and run.stderr.startswith("Error:"), (extra, run.stdout + run.stderr)
        assert all(w in run.stderr for w in words), (extra, run.stderr)
        assert "Loading database" not in run.stdout and "HIP device" not in run.stderr and not list(out.iterdir())
        return run

    refused(strata, "--cohort-strata needs --cohort-permanova, --cohort-permdisp, --cohort-edge-test or --cohort-model")
    refused(["--cohort"] + strata, "--cohort-strata needs")
    refused(["--cohort", "--cohort-pcoa", "--cohort-squash"] + strata, "--cohort-strata needs")
    refused(test + ["--cohort-strata-column", "subject"], "--cohort-strata-column needs --cohort-strata")
    refused(test + strata, "strata.tsv", "2 columns", "--cohort-strata-column")
    refused(test + strata + ["--cohort-strata-column", "who"], "no column 'who'")
    refused(test + strata + ["--cohort-strata-column", "batch"], "--cohort-strata", "line 8", "column batch", "'none'", "no stratum")
    refused(test + ["--cohort-strata", str(tmp_path / "nowhere.tsv")], "--cohort-strata", "cannot open")
    # a good strata file: read, reported, and only then the database is missed
    run = subprocess.run(base + test + strata + ["--cohort-strata-column", "subject"], capture_output=True, text=True)
    assert run.returncode == 255 and "strata" not in run.stderr, run.stderr
    assert "Cohort strata: column subject, 3 strata of 5 samples" in run.stdout
    shown = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert shown.returncode == 0 and "--cohort-strata arg" in shown.stdout and "--cohort-strata-column arg" in shown.stdout


def test_the_launcher_passes_the_strata_flags_on_and_refuses_them_alone():
    import click
    sys.path.insert(0, ROOT)
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw)
    assert epik.driver_command(**kw, cohort_strata=None, cohort_strata_column=None) == default
    for test in (dict(cohort_permanova="f.tsv"), dict(cohort_permdisp="f.tsv"), dict(cohort_edge_test="f.tsv"),
                 dict(cohort_model="f.tsv", cohort_model_terms="f:state")):
        argv = epik.driver_command(**kw, cohort=True, cohort_strata="s.tsv", cohort_strata_column="subject", **test)
        at = argv.index("--cohort-strata")
        assert argv[at:at + 4] == ["--cohort-strata", "s.tsv", "--cohort-strata-column", "subject"]
        assert "--cohort-strata-column" not in epik.driver_command(**kw, cohort=True, cohort_strata="s.tsv", **test)
    for bad in (dict(cohort=True, cohort_strata="s.tsv"), dict(cohort=True, cohort_pcoa=True, cohort_strata="s.tsv"),
                dict(cohort=True, cohort_permanova="f.tsv", cohort_strata_column="subject")):
        with pytest.raises(click.UsageError):
            epik.driver_command(**kw, **bad)
    me = os.path.join(ROOT, "epik.py")
    shown = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert shown.returncode == 0 and "--cohort-strata " in shown.stdout and "--cohort-strata-column" in shown.stdout
    for flags, word in ((["--cohort", "--cohort-strata", me], "--cohort-strata needs"),
                        (["--cohort", "--cohort-permanova", me, "--cohort-strata-column", "x"], "--cohort-strata-column needs")):
        run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, *flags, me], capture_output=True, text=True)
        assert run.returncode == 2 and word in run.stderr, (flags, run.stdout, run.stderr)


# ---- 7. the build record ----------------------------------------------------------------------------------------------------
def test_the_kernels_that_existed_keep_the_build_record_of_the_parent_commit():
    """profiles/strata_kernels.json holds, for the four analyses' files, every kernel's VGPRs, SGPRs, spills, static LDS and
    scratch of the parent commit and of this one (tools/kernel_figures.py).  Every kernel of the parent is there still, under
    its name or as the instantiation with kStrata = false, with the parent's figures; and where the library at hand was built
    by the record's compiler, its listings give the record's figures."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_figures
    with open(os.path.join(ROOT, "profiles", "strata_kernels.json")) as fh:
        record = json.load(fh)
    unstratified = lambda name: re.sub(r"^void ", "", re.sub(r"<false>\(", "(", re.sub(r", false>\(", ">(", name)))
    kept = 0
    for name, parent in record["parent"].items():
        now = {unstratified(k): v for k, v in record["this"][name].items()}
        now.update({re.sub(r"^void ", "", k): v for k, v in record["this"][name].items()})     # (a kernel that kept its name)
        for kernel, figures in parent.items():
            assert now[re.sub(r"^void ", "", kernel)] == figures, (name, kernel)
            kept += 1
        assert len(record["this"][name]) > len(parent)                          # (the kStrata instantiations and the tables' kernel)
    assert kept == 40
    with open(os.path.join(ROOT, "epik_amd", "libepik_amd.build.json")) as fh:
        built_with = json.load(fh)["hipcc"]
    if built_with == record["hipcc"]:
        for name in record["this"]:
            listing = os.path.join(ROOT, "epik_amd", "csrc", "build", "lib", f"{name}-hip-amdgcn-amd-amdhsa-gfx950.s")
            assert kernel_figures.figures(listing) == record["this"][name], name
