"""Permutations within strata on the device: the `_strata` entries of PERMANOVA, PERMDISP, the edge test and the sequential model
against the host mirror (and, for the smaller cohorts, the numpy restatement of test_strata_cpu), bit for bit, into poisoned
buffers on a stream of their own; the sizes at which the kernels take another path (a wave, PERMANOVA's counting, sort and LDS
limits with and without strata, the key tile of the stratified ranking with a stratum across its seam, the model's LDS tier),
the general paths forced, two workgroups; no side effects; the properties of test_strata_cpu on the device; and one handle
through stratified and unstratified calls of the four analyses in turn.
"""
import numpy as np
import pytest

import test_edgetest_cpu as edge_cpu
import test_model_cpu as model_cpu
import test_permanova_cpu as nova_cpu
import test_permdisp_cpu as disp_cpu
from epik_amd import capi, cohort as cohort_mod
from test_cohort_cpu import random_cells, same_bits
from test_cohort_gpu import ENV, kr_case
from test_strata_cpu import (MISSING, model_design, numpy_edgetest, numpy_model, numpy_permanova, numpy_permdisp, paired_line,
                             same_records, strata_layouts)

pytestmark = pytest.mark.gpu
U64 = np.uint64
SWITCHES = ("EPIK_AMD_PERMANOVA_LDS", "EPIK_AMD_EDGETEST_LDS", "EPIK_AMD_MODEL_LDS")
SLOTS = 1 + capi.PERMANOVA_PAIR_SLOTS
SMALL = 130                  # up to here every layout, the general paths and two workgroups are run as well
PAIRWISE = 257               # up to here the pairwise tests are run
RESTATED = 65                # up to here the restatement is computed beside the mirror

# S: over a wave; 128 | 129 (PERMANOVA's one wave, the model's LDS tier); 256 | 257 | 258 (counting | sorting); 512 | 513 (the LDS
# limit with strata); 1 024 | 1 025 | 1 026 (the LDS limit without, and the key tile: one sample is empty, so the last has 1 025
# positions).  P: 1, and 4 k - 1, 4 k, 4 k + 1.
CASES = {7: ((65, 63), (128, 64), (129, 65), (256, 1), (257, 9), (258, 5), (512, 3), (513, 3), (1024, 3), (1025, 2), (1026, 2)),
         999: ((130, 9),)}


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def layouts_of(num_samples):
    """Every layout of test_strata_cpu for the small cohorts; for the large ones pairs and blocks -- the blocks of
    (S + 3) / 4 samples put a stratum across position 1 023 | 1 024 from 1 025 samples on."""
    every = strata_layouts(num_samples)
    return every if num_samples <= SMALL else {name: every[name] for name in ("pairs", "blocks")}


def case_labels(rng, num_samples):
    i = np.arange(num_samples)
    three = np.where(rng.random(num_samples) < 0.2, MISSING, rng.integers(0, 3, num_samples))
    return np.ascontiguousarray(np.array([rng.permutation(i % 2), three, i % 2], dtype=np.uint32).T)


def poisoned(pl, nbytes):
    import torch
    return torch.full((max(nbytes, 1),), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}")


def on_a_stream(call):
    """`call(stream)` on a stream of its own, then everything drained."""
    import torch
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    call(stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()


def device_distances(pl, cohort, tree, bl):
    import torch
    s = cohort.num_samples
    d_kr = torch.full((s * s,), np.nan, dtype=torch.float64, device=f"cuda:{pl.device}")
    cohort.kr_device(tree, bl, d_kr.data_ptr())
    torch.cuda.synchronize()
    return d_kr


def raw_permanova(pl, cohort, d_kr, labels, permutations, seed, pairwise, strata):
    m, slots = labels.shape[1], SLOTS if pairwise else 1
    bufs = [poisoned(pl, n) for n in (m * slots * 56, m * slots * (permutations + 1) * 8, m * 256 * 8)]
    on_a_stream(lambda stream: cohort.permanova_device(d_kr.data_ptr(), labels, permutations, seed, pairwise, bufs[0].data_ptr(),
                                                       bufs[1].data_ptr(), bufs[2].data_ptr(), stream, strata=strata))
    out, ssw, group_ss = (b.cpu().numpy() for b in bufs)
    return cohort_mod.Permanova(out.view(capi.PERMANOVA).reshape(m, slots).copy(), ssw.view(np.float64).reshape(m, slots, permutations + 1).copy(),
                                group_ss.view(np.float64).reshape(m, 256).copy())


def raw_permdisp(pl, cohort, d_kr, labels, permutations, seed, pairwise, strata):
    s, m, slots = cohort.num_samples, labels.shape[1], SLOTS if pairwise else 1
    bufs = [poisoned(pl, n) for n in (m * slots * 48, m * slots * (permutations + 1) * 8, m * 32 * 8, m * s * 8)]
    on_a_stream(lambda stream: cohort.permdisp_device(d_kr.data_ptr(), labels, permutations, seed, pairwise, bufs[0].data_ptr(),
                                                      bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[1].data_ptr(), stream, strata=strata))
    out, stat, mean, z = (b.cpu().numpy() for b in bufs)
    return cohort_mod.Permdisp(out.view(capi.PERMDISP).reshape(m, slots).copy(), stat.view(np.float64).reshape(m, slots, permutations + 1).copy(),
                               mean.view(np.float64).reshape(m, 32).copy(), z.view(np.float64).reshape(m, s).copy())


def raw_edgetest(pl, cohort, tree, labels, permutations, seed, strata):
    n, m, row = cohort.num_branches, labels.shape[1], permutations + 1
    bufs = [poisoned(pl, nbytes) for nbytes in (m * n * 208, m * 4 * n * row * 8, m * 4 * row * 8)]
    on_a_stream(lambda stream: cohort.edgetest_device(tree, labels, permutations, seed, bufs[0].data_ptr(), bufs[1].data_ptr(),
                                                      bufs[2].data_ptr(), stream, strata=strata))
    out, stat, most = (b.cpu().numpy() for b in bufs)
    return cohort_mod.Edgetest(out.view(capi.EDGETEST).reshape(m, n).copy(), stat.view(np.float64).reshape(m, 4, n, row).copy(),
                               most.view(np.float64).reshape(m, 4, row).copy())


def raw_model(pl, cohort, d_kr, design, permutations, seed, strata):
    terms = len(design[0])
    bufs = [poisoned(pl, n) for n in ((terms + 1) * 48, 40, 64, (terms + 1) * (permutations + 1) * 8)]
    on_a_stream(lambda stream: cohort.model_device(d_kr.data_ptr(), *design, permutations, seed, bufs[0].data_ptr(), bufs[1].data_ptr(),
                                                   bufs[2].data_ptr(), bufs[3].data_ptr(), stream, strata=strata))
    out, info, aliased, stat = (b.cpu().numpy() for b in bufs)
    return cohort_mod.Model(out.view(capi.MODEL_TERM).copy(), info.view(capi.MODEL_INFO)[0].copy(),
                            stat.view(np.float64).reshape(terms + 1, permutations + 1).copy(), aliased.copy())


def mirrors(mass, first, bl, labels, design, permutations, seed, pairwise, strata, metric="kr"):
    return {"permanova": cohort_mod.permanova_host(mass, first, bl, labels, permutations, seed, pairwise, metric=metric, strata=strata),
            "permdisp": cohort_mod.permdisp_host(mass, first, bl, labels, permutations, seed, pairwise, metric=metric, strata=strata),
            "edgetest": cohort_mod.edgetest_host(mass, first, labels, permutations, seed, strata=strata),
            "model": cohort_mod.model_host(mass, first, bl, *design, permutations, seed, metric=metric, strata=strata)}


def check_device(pl, cohort, tree, bl, mass, labels, design, permutations, seed, pairwise, strata, want, what, analyses=None):
    """The four analyses into poisoned buffers: the mirror's bytes; d_kr and the cells unchanged."""
    d_kr = device_distances(pl, cohort, tree, bl)
    before = d_kr.cpu().numpy().copy()
    calls = {"permanova": lambda: raw_permanova(pl, cohort, d_kr, labels, permutations, seed, pairwise, strata),
             "permdisp": lambda: raw_permdisp(pl, cohort, d_kr, labels, permutations, seed, pairwise, strata),
             "edgetest": lambda: raw_edgetest(pl, cohort, tree, labels, permutations, seed, strata),
             "model": lambda: raw_model(pl, cohort, d_kr, design, permutations, seed, strata)}
    same = {"permanova": nova_cpu.same_permanova, "permdisp": disp_cpu.same_permdisp, "edgetest": edge_cpu.same_edgetest,
            "model": model_cpu.same_model}
    for analysis in analyses or calls:
        same[analysis](calls[analysis](), want[analysis], what + (analysis,))
    assert same_bits(before, d_kr.cpu().numpy()), what
    after = cohort.read()
    assert np.array_equal(after.mass, mass) and not after.best.any(), what


def build_cases(num_branches):
    parent, bl, first, db = kr_case(num_branches)
    rng = np.random.default_rng(7700 + num_branches)
    cases = []
    for num_samples, permutations in CASES[num_branches]:
        mass = random_cells(rng, num_samples, num_branches, empty=1, bits=42)
        labels = case_labels(rng, num_samples)
        design = model_design(labels, rng)
        for name, strata in layouts_of(num_samples).items():
            pairwise = num_samples <= PAIRWISE and name in ("pairs", "interleaved")
            seed = int(rng.integers(0, 1 << 63)) * 2 + 1
            want = mirrors(mass, first, bl, labels, design, permutations, seed, pairwise, strata)
            if num_samples <= RESTATED and name in ("pairs", "huge"):
                kr, totals = cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass)
                what = (num_samples, name, "restated")
                nova_cpu.same_permanova(want["permanova"], numpy_permanova(kr, totals, labels, permutations, seed, pairwise, strata), what)
                disp_cpu.same_permdisp(want["permdisp"], numpy_permdisp(kr, totals, labels, permutations, seed, pairwise, strata), what)
                edge_cpu.same_edgetest(want["edgetest"], numpy_edgetest(mass, first, labels, permutations, seed, strata), what)
                model_cpu.same_model(want["model"], numpy_model(kr, totals, *design, permutations, seed, strata), what)
            cases.append((num_samples, name, mass, labels, design, permutations, seed, pairwise, strata, want))
    return parent, bl, db, cases


@pytest.mark.parametrize("num_branches", sorted(CASES))
def test_the_four_analyses_equal_the_host_mirror_bit_for_bit(placer_cls, monkeypatch, num_branches):
    for var in ENV + SWITCHES:
        monkeypatch.delenv(var, raising=False)
    parent, bl, db, cases = build_cases(num_branches)
    for name, env in (("default", {}), ("the general paths", {switch: "0" for switch in SWITCHES}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for num_samples, layout, mass, labels, design, permutations, seed, pairwise, strata, want in cases:
                if name != "default" and num_samples > SMALL:
                    continue
                what = (name, num_samples, layout, permutations, pairwise)
                with pl.cohort(num_samples) as cohort:
                    cohort.add_cells(mass, None, None)
                    check_device(pl, cohort, tree, bl, mass, labels, design, permutations, seed, pairwise, strata, want, what)
                    if layout == "pairs":                                   # the synchronous entries, and the workspace used again
                        nova_cpu.same_permanova(cohort.permanova(tree, bl, labels, permutations, seed, pairwise, with_ssw=True, strata=strata),
                                                want["permanova"], what)
                        disp_cpu.same_permdisp(cohort.permdisp(tree, bl, labels, permutations, seed, pairwise, with_stat=True, strata=strata),
                                               want["permdisp"], what)
                        edge_cpu.same_edgetest(cohort.edgetest(tree, labels, permutations, seed, True, True, strata=strata), want["edgetest"], what)
                        model_cpu.same_model(cohort.model(tree, bl, *design, permutations, seed, with_stat=True, strata=strata), want["model"], what)
        for key in env:
            monkeypatch.delenv(key)


def test_strata_over_an_unweighted_unifrac(placer_cls, monkeypatch):
    for var in ENV + SWITCHES:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(7)
    rng = np.random.default_rng(31)
    num_samples, permutations, seed = 33, 21, 5
    mass = random_cells(rng, num_samples, 7, empty=1, bits=42)
    labels = case_labels(rng, num_samples)
    design = model_design(labels, rng)
    strata = strata_layouts(num_samples)["blocks"]
    want = mirrors(mass, first, bl, labels, design, permutations, seed, True, strata, metric="unweighted")
    assert not same_bits(want["permanova"].ssw, mirrors(mass, first, bl, labels, design, permutations, seed, True, strata)["permanova"].ssw)
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(num_samples) as cohort:
        cohort.add_cells(mass, None, None)
        got = cohort.permanova(tree, bl, labels, permutations, seed, True, with_ssw=True, metric="unweighted", strata=strata)
        nova_cpu.same_permanova(got, want["permanova"], "unweighted")
        got = cohort.permdisp(tree, bl, labels, permutations, seed, True, with_stat=True, metric="unweighted", strata=strata)
        disp_cpu.same_permdisp(got, want["permdisp"], "unweighted")
        got = cohort.model(tree, bl, *design, permutations, seed, with_stat=True, metric="unweighted", strata=strata)
        model_cpu.same_model(got, want["model"], "unweighted")


def test_the_properties_hold_on_the_device(placer_cls, monkeypatch):
    """(a) one stratum gives the bytes of the entries without strata, (b) singletons give p = 1 with every SSW the observed one,
    (e) the paired cohort needs its strata -- on the device, over cells whose samples lie in pairs."""
    for var in ENV + SWITCHES:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(7)
    rng = np.random.default_rng(41)
    num_samples, permutations, seed = 130, 33, 3
    mass = random_cells(rng, num_samples, 7, empty=1, bits=42)
    labels = case_labels(rng, num_samples)
    design = model_design(labels, rng)
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
        with pl.cohort(num_samples) as cohort:
            cohort.add_cells(mass, None, None)
            plain = mirrors(mass, first, bl, labels, design, permutations, seed, True, None)
            check_device(pl, cohort, tree, bl, mass, labels, design, permutations, seed, True, None, plain, ("no strata",))
            for stratum in (0, 0xFFFFFFFF):                                # (a)
                check_device(pl, cohort, tree, bl, mass, labels, design, permutations, seed, True, np.full(num_samples, stratum, np.uint32),
                             plain, ("one stratum", stratum))
        # the id 0xffffffff is a stratum like any other, also where PERMANOVA sorts (beyond 256 positions) and its padding
        # takes that very id: a third of 300 samples in it, interleaved with pairs
        many = 300
        mass300 = random_cells(rng, many, 7, empty=1, bits=42)
        labels300 = case_labels(rng, many)
        top = np.where(np.arange(many) % 3 == 0, 0xFFFFFFFF, np.arange(many) // 6).astype(np.uint32)
        with pl.cohort(many) as cohort:
            cohort.add_cells(mass300, None, None)
            for pairwise in (False, True):
                want = cohort_mod.permanova_host(mass300, first, bl, labels300, 9, 77, pairwise, strata=top)
                got = cohort.permanova(tree, bl, labels300, 9, 77, pairwise, with_ssw=True, strata=top)
                nova_cpu.same_permanova(got, want, ("the id 0xffffffff", pairwise))
            assert not same_bits(want.ssw, cohort_mod.permanova_host(mass300, first, bl, labels300, 9, 77, True).ssw)
        with pl.cohort(num_samples) as cohort:
            cohort.add_cells(mass, None, None)
            singles = (5000 - np.arange(num_samples)).astype(np.uint32)     # (b)
            got = cohort.permanova(tree, bl, labels, permutations, seed, True, with_ssw=True, strata=singles)
            defined = ~np.isnan(got.records["p"])
            assert defined[:, 0].all() and (got.ssw[defined].view(U64) == got.ssw[defined][:, :1].view(U64)).all()
            assert (got.records["at_most"][defined] == permutations).all() and (got.records["p"][defined] == 1.0).all()
            got = cohort.model(tree, bl, *design, permutations, seed, with_stat=True, strata=singles)
            tested = got.records["df"] > 0
            assert tested.any() and (got.records["at_least"][tested] == permutations).all() and (got.records["p"][tested] == 1.0).all()
            got = cohort.edgetest(tree, labels, permutations, seed, strata=singles).records["family"]
            assert (got["p"][~np.isnan(got["p"])] == 1.0).all() and (~np.isnan(got["p"])).sum() > 10
        # (e) eight subjects far apart on a ladder of masses, each sampled twice, the treatment a small shift
        subjects, num_samples = 8, 16
        mass = np.zeros((num_samples, 7), dtype=U64)
        for i in range(subjects):
            for treated in (0, 1):
                mass[2 * i + treated, 0], mass[2 * i + treated, 1] = 1000 - 100 * i - 10 * treated, 100 * i + 10 * treated + 1
        labels = np.tile([0, 1], subjects).astype(np.uint32)[:, None].copy()
        strata = np.repeat(np.arange(subjects), 2).astype(np.uint32)
        with pl.cohort(num_samples) as cohort:
            cohort.add_cells(mass, None, None)
            for seed in (1, 2, 3):
                free = cohort.permanova(tree, bl, labels, 999, seed, with_ssw=True)
                within = cohort.permanova(tree, bl, labels, 999, seed, with_ssw=True, strata=strata)
                nova_cpu.same_permanova(free, cohort_mod.permanova_host(mass, first, bl, labels, 999, seed), ("paired", seed))
                nova_cpu.same_permanova(within, cohort_mod.permanova_host(mass, first, bl, labels, 999, seed, strata=strata), ("paired", seed))
                print("paired cohort, seed", seed, "free p", free.records["p"][0, 0], "within subjects p", within.records["p"][0, 0])
                assert within.records["p"][0, 0] < 0.05 and free.records["p"][0, 0] > 0.5


def test_one_handle_through_stratified_and_unstratified_calls(placer_cls, monkeypatch):
    """The tables of a call live in the handle's workspaces: stratified, then without strata, then other strata, then thinned
    cells, then a cohort of two samples, the four analyses in a changing order -- every step the mirror's bytes."""
    for var in ENV + SWITCHES:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(7)
    rng = np.random.default_rng(51)
    num_samples, permutations = 65, 17
    mass = random_cells(rng, num_samples, 7, empty=1, bits=42)
    thinned = mass.copy()
    thinned[rng.random(mass.shape) < 0.6] = 0
    thinned[:, 0] |= (mass.sum(axis=1, dtype=U64) != 0).astype(U64)
    thinned[5] = 0
    labels = case_labels(rng, num_samples)
    design = model_design(labels, rng)
    layouts = strata_layouts(num_samples)
    order = ["permanova", "permdisp", "edgetest", "model"]
    steps = [(mass, layouts["pairs"]), (mass, None), (mass, layouts["interleaved"]), (thinned, layouts["interleaved"]), (thinned, None),
             (thinned, layouts["huge"]), (mass, layouts["blocks"])]
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
        with pl.cohort(num_samples) as cohort:
            for step, (cells, strata) in enumerate(steps):
                cohort.reset()
                cohort.add_cells(cells, None, None)
                seed = 100 + step
                want = mirrors(cells, first, bl, labels, design, permutations, seed, step % 2 == 0, strata)
                order = order[1:] + order[:1]
                check_device(pl, cohort, tree, bl, cells, labels, design, permutations, seed, step % 2 == 0, strata, want, ("step", step),
                             analyses=order)
        two = mass[[0, 2]].copy()
        for strata in (np.array([4, 4], np.uint32), None, np.array([4, 9], np.uint32)):
            with pl.cohort(2) as cohort:
                cohort.add_cells(two, None, None)
                two_labels = np.array([[0, 1], [1, 1], [0, 0]], dtype=np.uint32).T.copy()
                two_design = model_cpu.design(("f", two_labels[:, 0]))
                want = mirrors(two, first, bl, two_labels, two_design, 5, 1, True, strata)
                check_device(pl, cohort, tree, bl, two, two_labels, two_design, 5, 1, True, strata, want, ("two samples", strata is None))
