"""PERMDISP of a cohort's samples over their KR distances on the device: epik_amd_cohort_permdisp / _permdisp_device against the
host mirror and the rule restated in numpy (test_permdisp_cpu.numpy_permdisp), bit for bit, the records, every stat[p], the
group means and z; both accumulator paths (G <= 4 in registers, beyond in LDS), the chunk of labellings stepped over, two
workgroups; the star fed through d_kr; no side effects; the errors; one handle called with one column, three columns pairwise
and one column again (the workspace grows, then the larger buffer is carved for the smaller shape).  (epik-dna --cohort --cohort-pcoa --cohort-permdisp
--cohort-permanova end to end is in test_pcoa_gpu.)
"""
import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod
from test_cohort_cpu import random_cells, same_bits
from test_cohort_gpu import ENV, kr_case
from test_pcoa_cpu import STAR_KR
from test_permanova_gpu import factor_labels
from test_permdisp_cpu import MISSING, SLOTS, numpy_permdisp, same_permdisp

pytestmark = pytest.mark.gpu
U64 = np.uint64
CHUNK = 1024                 # the labellings made at a time (permdisp_place.hip: kChunk)
REGISTER_GROUPS = 4          # up to here a lane's accumulators are registers (kRegisterGroups)
PAIRWISE_UP_TO = 130


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def capped_labels(rng, num_samples, pairwise):
    """test_permanova_gpu.factor_labels with every label taken mod 32, the cap of this test: 2 groups; 3 with a fifth missing;
    5 under scattered ids; and, without pairwise, 32 groups (every sample its own up to 32 samples) and a single group."""
    labels = factor_labels(rng, num_samples, pairwise)
    return np.where(labels == MISSING, MISSING, labels % 32).astype(np.uint32)


def device_permdisp_raw(pl, cohort, d_kr, labels, permutations, seed, pairwise):
    """permdisp_device over d_kr into poisoned buffers on a stream of its own: a `Permdisp` as the device left it."""
    import torch
    s, m = labels.shape
    slots = SLOTS if pairwise else 1
    sizes = (m * slots * 48, m * slots * (permutations + 1) * 8, m * 32 * 8, m * s * 8)
    bufs = [torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}") for nbytes in sizes]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    cohort.permdisp_device(d_kr.data_ptr(), labels, permutations, seed, pairwise, bufs[0].data_ptr(), bufs[2].data_ptr(),
                           bufs[3].data_ptr(), bufs[1].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    out, stat, mean, z = (b.cpu().numpy() for b in bufs)
    return cohort_mod.Permdisp(out.view(capi.PERMDISP).reshape(m, slots).copy(),
                               stat.view(np.float64).reshape(m, slots, permutations + 1).copy(),
                               mean.view(np.float64).reshape(m, 32).copy(), z.view(np.float64).reshape(m, s).copy())


# (S, P) of the issue, one sample of each cohort empty; then the chunk of 1 024 labellings stepped over at S = 4
CASES = ((3, 1), (4, 63), (33, 64), (65, 65), (129, 200), (257, 9), (4, CHUNK + 1))
SMALL = 65                    # up to here two workgroups are run as well


def permdisp_cases(num_branches=7):
    """[(S, mass, labels, P, seed, pairwise, the host mirror's Permdisp)]: every case with all its columns (more than four groups:
    the accumulators in LDS) and with its first two alone (two and three groups: in registers)."""
    parent, bl, first, db = kr_case(num_branches)
    rng = np.random.default_rng(2300 + num_branches)
    cases = []
    for num_samples, permutations in CASES:
        mass = random_cells(rng, num_samples, num_branches, empty=1, bits=42)
        kr, totals = cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass)
        for pairwise in (False, True):
            if pairwise and (num_samples > PAIRWISE_UP_TO or permutations > CHUNK):
                continue
            wide = capped_labels(rng, num_samples, pairwise)
            seed = int(rng.integers(0, 1 << 63)) * 2 + int(pairwise)
            for labels in (wide, np.ascontiguousarray(wide[:, :2])):
                want = cohort_mod.permdisp_kr_host(kr, totals, labels, permutations, seed, pairwise)
                if num_samples <= 65 and permutations <= 65:                    # (the restatement is slow: the small cases)
                    same_permdisp(want, numpy_permdisp(kr, totals, labels, permutations, seed, pairwise), (num_samples, pairwise))
                cases.append((num_samples, mass, labels, permutations, seed, pairwise, want))
    return cases


def test_permdisp_equals_the_host_mirror_and_the_restatement_bit_for_bit(placer_cls, monkeypatch):
    import torch
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(7)
    cases = permdisp_cases(7)
    # the comparison cannot pass on NAs alone: more than half of the records are defined.  Counted among the tests that exist
    # (used > 0): a pairwise call has 496 pair slots a column and a column of G groups fills G (G - 1) / 2 of them, the rest
    # are empty by layout (used = groups = 0, NA), so over all slots no set of cases could reach a half
    exist = sum(int((c[-1].records["used"] > 0).sum()) for c in cases)
    defined = sum(int((~np.isnan(c[-1].records["p"])).sum()) for c in cases)
    assert 2 * defined > exist, (defined, exist)
    assert any(int(c[-1].records["groups"].max()) > REGISTER_GROUPS for c in cases)
    assert any(c[2].shape[1] == 2 and int(c[-1].records["groups"].max()) <= REGISTER_GROUPS for c in cases)
    assert any(int(c[-1].records["clipped"].max()) > 0 for c in cases), "the KR distance of a random cohort is not Euclidean"
    for name, env in (("default", {}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for num_samples, mass, labels, permutations, seed, pairwise, want in cases:
                if name != "default" and (num_samples > SMALL or permutations > CHUNK):
                    continue
                what = (name, num_samples, labels.shape[1], permutations, pairwise)
                with pl.cohort(num_samples) as cohort:
                    cohort.add_cells(mass, None, None)
                    same_permdisp(cohort.permdisp(tree, bl, labels, permutations, seed, pairwise, with_stat=True), want, what)
                    d_kr = torch.full((num_samples * num_samples,), np.nan, dtype=torch.float64, device=f"cuda:{pl.device}")
                    cohort.kr_device(tree, bl, d_kr.data_ptr())
                    torch.cuda.synchronize()
                    before = d_kr.cpu().numpy().copy()
                    # into poisoned buffers on a stream of its own: every cell written; the workspace used again
                    got = device_permdisp_raw(pl, cohort, d_kr, labels, permutations, seed, pairwise)
                    same_permdisp(got, want, what + ("raw",))
                    assert same_bits(d_kr.cpu().numpy(), before), what                          # d_kr is not changed
                    after = cohort.read()
                    assert np.array_equal(after.mass, mass) and not after.best.any(), what      # nor the cells
                    lean = cohort.permdisp(tree, bl, labels[:, :1].copy(), permutations, seed, pairwise)
                    assert lean.stat is None and lean.records[0].tobytes() == want.records[0].tobytes(), what
        for key in env:
            monkeypatch.delenv(key)


# the switches of the analyses around PERMDISP (test_cohort_lifecycle_gpu, test_model_lifecycle_gpu): "0" forces their general paths
SWITCHES = ("EPIK_AMD_EDGETEST_LDS", "EPIK_AMD_PERMANOVA_LDS", "EPIK_AMD_EPCA_LDS", "EPIK_AMD_CORRELATION_LDS", "EPIK_AMD_MODEL_LDS",
            "EPIK_AMD_PCOA_LDS")
GROWTH = {}


def growth_calls():
    """The KR matrix of 70 samples on the tree of 7 branches (padded to 96, one sample without mass) and three calls at P = 9 with
    the host mirror's Permdisp: one column; three columns pairwise, whose workspace is some thirty times the first call's (the
    pool of labellings alone has 32 lists for 1); and one column again."""
    if not GROWTH:
        parent, bl, first, db = kr_case(7)
        rng = np.random.default_rng(2377)
        mass = random_cells(rng, 70, 7, empty=1, bits=42)
        kr, totals = cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass)
        one, three = capped_labels(rng, 70, False)[:, 1:2].copy(), capped_labels(rng, 70, True)
        calls = [(labels, 9, int(rng.integers(0, 1 << 63)), pairwise) for labels, pairwise in ((one, False), (three, True), (one, False))]
        assert [c[0].shape for c in calls] == [(70, 1), (70, 3), (70, 1)]
        GROWTH["case"] = (parent, bl, db, mass, kr, [(c, cohort_mod.permdisp_kr_host(kr, totals, *c)) for c in calls])
    return GROWTH["case"]


@pytest.mark.parametrize("variant", ("as created", "the general paths"))
def test_the_workspace_grows_with_the_columns_and_is_carved_again_for_fewer(placer_cls, monkeypatch, variant):
    """One handle, one matrix: the second call needs a larger workspace than the first allocated, the third carves the larger
    buffer for the smaller shape.  A workspace kept too small, or parts laid out for another shape, cannot give these bytes."""
    import torch
    for var in ENV + SWITCHES:
        monkeypatch.delenv(var, raising=False)
    if variant == "the general paths":
        for switch in SWITCHES:
            monkeypatch.setenv(switch, "0")
    parent, bl, db, mass, kr, calls = growth_calls()
    # the comparison cannot pass on NAs alone, and the pairwise call has defined pairs
    assert all(not np.isnan(want.records["p"][:, 0]).any() for _, want in calls)
    assert int((~np.isnan(calls[1][1].records["p"][:, 1:])).sum()) >= 3
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(70) as cohort:
        cohort.add_cells(mass, None, None)
        d_kr = torch.full((70 * 70,), np.nan, dtype=torch.float64, device=f"cuda:{pl.device}")
        cohort.kr_device(tree, bl, d_kr.data_ptr())
        torch.cuda.synchronize()
        assert same_bits(d_kr.cpu().numpy().reshape(70, 70), kr), variant
        for k, (call, want) in enumerate(calls):
            same_permdisp(device_permdisp_raw(pl, cohort, d_kr, *call), want, (variant, "call", k + 1))
        assert same_bits(d_kr.cpu().numpy().reshape(70, 70), kr), (variant, "after")


def test_the_star_through_d_kr_and_the_errors(placer_cls, monkeypatch):
    import torch
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(7)
    forged = np.zeros((6, 6))
    forged[:4, :4] = STAR_KR
    forged[4, 5] = forged[5, 4] = 3.0
    forged[:4, 4:] = forged[4:, :4] = 7.0
    labels = np.array([[0, 0, 0, 0, 1, 1], [0, 1, 2, 3, 4, 5]], dtype=np.uint32).T.copy()
    totals = np.ones(6, U64)
    want = cohort_mod.permdisp_kr_host(forged, totals, labels, 99, 1, True)
    lib = capi.load()
    err = lambda: lib.epik_amd_last_error().decode()
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(6) as cohort:
        mass = np.zeros((6, 7), U64)
        mass[:, 0] = 1                                            # every sample has mass: T_s > 0 is all the rule takes of it
        cohort.add_cells(mass, None, None)
        device = f"cuda:{pl.device}"
        d_kr = torch.full((36,), np.nan, dtype=torch.float64, device=device)
        d_out = torch.full((2 * SLOTS * 48,), 0xA5, dtype=torch.uint8, device=device)
        d_mean = torch.full((2 * 32 * 8,), 0xA5, dtype=torch.uint8, device=device)
        d_z = torch.full((2 * 6 * 8,), 0xA5, dtype=torch.uint8, device=device)
        call = lambda c=cohort._handle, k=d_kr.data_ptr(), l=labels.ctypes.data, m=2, p=9, o=d_out.data_ptr(), g=d_mean.data_ptr(), \
            z=d_z.data_ptr(): lib.epik_amd_cohort_permdisp_device(c, k, l, m, p, 7, 1, o, None, g, z, None)
        # before any distance: T_s is not on the device yet
        assert call() == capi.ERR_INVALID and "kr_device" in err()
        cohort.kr_device(tree, bl, d_kr.data_ptr())
        torch.cuda.synchronize()
        assert call(c=None) == capi.ERR_INVALID and "null cohort" in err()
        for null in ("k", "l", "o", "g", "z"):
            assert call(**{null: None}) == capi.ERR_INVALID and "null argument" in err(), null
        for bad in (0, 65):
            assert call(m=bad) == capi.ERR_INVALID and "num_columns" in err() and "[1, 64]" in err()
        for bad in (0, 1_000_000):
            assert call(p=bad) == capi.ERR_INVALID and "num_permutations" in err() and "[1, 999999]" in err()
        wrong = labels.copy()
        wrong[3, 1] = 32
        assert call(l=wrong.ctypes.data) == capi.ERR_INVALID and "sample 3" in err() and "column 1" in err() and "32" in err()
        torch.cuda.synchronize()
        for buf in (d_out, d_mean, d_z):
            assert (buf.cpu().numpy() == 0xA5).all()                # the refused calls wrote nothing
        # the forged matrix: the star beside a pair, in the place of the cohort's own distances
        d_kr.copy_(torch.from_numpy(forged.reshape(-1)).to(device))
        torch.cuda.synchronize()
        got = device_permdisp_raw(pl, cohort, d_kr, labels, 99, 1, True)
        same_permdisp(got, want, "star")
        assert same_bits(d_kr.cpu().numpy().reshape(6, 6), forged)
    leaf = np.sqrt(1.3125)
    assert same_bits(got.z[0], [leaf, leaf, leaf, 0.0, 1.5, 1.5]) and got.records["clipped"][0, 0] == 1
    assert got.records["clipped"][0, cohort_mod.pair_slot(0, 1)] == 1 and not np.isnan(got.records["p"][0, 0])
    assert np.isnan(got.records["p"][1, 0]) and same_bits(got.z[1], np.zeros(6))            # all singletons: z is +0.0
