"""The edge model on the device (edgemodel_place.hip) against the host mirror and the numpy restatement, bit for bit: at every
edge of the hot kernel's tiling (the branch block, the permutation block, the slab of positions, the chunk of permutations),
over a wave, the workgroup's lanes, the ranking's tile and the LDS tier of the observed pass, at ranks on each side of the
register block's columns and at 63 and 64, every one of them also on the general path and with two workgroups; with strata; with and without
stat and max; and one handle through dense, thinned and two-sample cells with the edge model between its siblings.
"""
import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, synth
from test_cohort_cpu import numpy_first, random_cells
from test_cohort_gpu import ENV, kr_case
from test_edgemodel_cpu import numpy_edgemodel, same_edgemodel
from test_edgetest_cpu import same_edgetest
from test_edgetest_gpu import device_edgetest_raw, group_labels
from test_model_cpu import same_model
from test_model_gpu import device_model_raw, model_design
from test_permanova_cpu import same_permanova
from test_permanova_gpu import device_permanova_raw, sparser

pytestmark = pytest.mark.gpu
U64 = np.uint64
SWITCH = "EPIK_AMD_EDGEMODEL_LDS"
SWITCHES = (SWITCH, "EPIK_AMD_EDGETEST_LDS", "EPIK_AMD_MODEL_LDS", "EPIK_AMD_PERMANOVA_LDS")
TILE_BRANCHES = 16           # listed branches a tile of the hot kernel (edgemodel_place.hip: kTileBranches)
TILE_COLS = 128              # chains a tile: TILE_COLS // Rb whole permutations, Rb the design's columns (kTileCols)
SLAB = 32                    # positions staged at a time (kSlab)
CHUNK_TILES = 32             # tiles of chains a chunk of permutations (kChunkTiles): 4 096 permutations of one column
REG_COLS = 4                 # the columns of a lane's register block (kRegCols)
LDS_POSITIONS = 1024         # the most samples whose vectors stay in LDS in the observed pass (kLdsPositions)
BLOCK = 256                  # the lanes of a workgroup
KEY_TILE = 1024              # the keys permutation_rank ranks against at a time (cohort_device.hpp: kCohortKeyTile)
SMALL = 300                  # a size between the workgroup's lanes and the ranking's tile, for the rank of 64
TREES = {}


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def tree_of(num_branches):
    """(parent, branch_length, first, db): kr_case's trees, and two of 15 and 17 branches, one below and one above a branch tile."""
    if num_branches in (7, 999):
        return kr_case(num_branches)
    if num_branches not in TREES:
        tree = synth.make_tree((num_branches + 1) // 2, seed=30)
        parent = np.asarray(tree.parent, dtype=np.int64)
        assert len(parent) == num_branches
        TREES[num_branches] = (parent, np.array(tree.branch_length, dtype=np.float64), numpy_first(parent),
                               synth.make_db(num_branches, kmer_size=4, seed=31, p_present=0.7))
    return TREES[num_branches]


# (S, P, rank, extras) by the number of branches; one sample of each cohort is empty, so L = S - 1 where nothing is missing.
# N = 7: fewer listed branches than a tile.  L steps over the slab (31, 32, 33), a wave, the workgroup's lanes, and the ranking's
# tile and the LDS tier (1 023, 1 024, 1 025).  The rank: 1, each side of the register block's columns (3, 4, 5), 63 and 64.
# P + 1 steps over the permutations of a tile (128 of one column; 32 of four, with 3 accepted and one aliased) and over the
# chunk (4 096 of one column, 1 024 of four).  N = 15, 17: one branch below and above a tile; N = 17 with the mass of a leaf
# zeroed: 16 listed.  N = 999: many tiles of branches.
CASES = {7: ((3, 1, 1, ""), (SLAB, 1, 1, ""), (SLAB + 1, TILE_COLS - 2, 1, ""), (SLAB + 2, TILE_COLS - 1, 1, ""),
             (64, TILE_COLS, 1, "missing"), (65, CHUNK_TILES * TILE_COLS - 2, 1, ""), (66, CHUNK_TILES * TILE_COLS - 1, 1, ""),
             (40, CHUNK_TILES * TILE_COLS, 1, "missing"), (BLOCK - 1, TILE_COLS // 4 - 2, 3, "alias missing"),
             (BLOCK, TILE_COLS // 4 - 1, 3, "alias"), (BLOCK + 1, TILE_COLS // 4, REG_COLS, "na missing"),
             (90, CHUNK_TILES * TILE_COLS // 4 - 2, REG_COLS, ""), (91, CHUNK_TILES * TILE_COLS // 4 - 1, REG_COLS, ""),
             (92, CHUNK_TILES * TILE_COLS // 4, 3, "alias"), (BLOCK + 2, 8, REG_COLS + 1, "na missing"), (140, 7, 63, "alias"),
             (SMALL, 5, 64, ""), (KEY_TILE, 5, 9, "alias"), (KEY_TILE + 1, 3, 3, "na"), (KEY_TILE + 2, 2, 2, "")),
         15: ((40, 33, 2, ""),),
         17: ((40, 33, 2, ""), (41, 33, 2, "zeroed")),
         999: ((5, 9, 1, "na"), (33, 8, 4, "missing"), (65, TILE_COLS, 5, "alias missing"), (130, 9, 64, ""), (200, 8, 5, "alias na missing"))}


def device_edgemodel_raw(pl, cohort, tree, kind, labels, values, permutations, seed, num_branches, with_stat=True, with_max=True,
                         strata=None):
    """edgemodel_device into poisoned buffers on a stream of its own: `cohort_mod.Edgemodel`."""
    import torch
    t, row = labels.shape[1], permutations + 1
    sizes = (t * num_branches * 144, 152, t * 2 * num_branches * row * 8 if with_stat else 8, t * 2 * row * 8 if with_max else 8, 64)
    bufs = [torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}") for nbytes in sizes]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    cohort.edgemodel_device(tree, kind, labels, values, permutations, seed, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[4].data_ptr(),
                            bufs[2].data_ptr() if with_stat else 0, bufs[3].data_ptr() if with_max else 0, stream.cuda_stream, strata=strata)
    stream.synchronize()
    torch.cuda.synchronize()
    out, info, stat, most, aliased = (b.cpu().numpy() for b in bufs)
    if not with_stat:
        assert (stat == 0xA5).all()
    if not with_max:
        assert (most == 0xA5).all()
    return cohort_mod.Edgemodel(out.view(capi.EDGEMODEL).reshape(t, num_branches).copy(), info.view(capi.EDGEMODEL_INFO)[0].copy(),
                                stat.view(np.float64).reshape(t, 2, num_branches, row).copy() if with_stat else None,
                                most.view(np.float64).reshape(t, 2, row).copy() if with_max else None, aliased.copy())


@pytest.mark.parametrize("num_branches", sorted(CASES))
def test_edgemodel_equals_the_host_mirror_and_the_restatement_bit_for_bit(placer_cls, monkeypatch, num_branches):
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = tree_of(num_branches)
    rng = np.random.default_rng(2800 + num_branches)
    cases = []
    for num_samples, permutations, rank, extras in CASES[num_branches]:
        mass = random_cells(rng, num_samples, num_branches, empty=1, bits=42)
        if "zeroed" in extras:
            mass[:, int(np.flatnonzero(first == np.arange(num_branches))[0])] = 0        # a leaf without mass: the list skips it
        kind, labels, values = model_design(rng, num_samples, rank, extras)
        seed = int(rng.integers(0, 1 << 63))
        want = cohort_mod.edgemodel_host(mass, first, kind, labels, values, permutations, seed)
        if num_branches == 7:
            same_edgemodel(want, numpy_edgemodel(mass, first, kind, labels, values, permutations, seed), (num_samples, "the restatement"))
        if num_samples > 2 * rank + 4:
            assert want.info["rank"] == rank and want.aliased.sum() == ("alias" in extras), (num_samples, want.info)
            listed = int((~np.isnan(want.records["family"]["ss"])).any(axis=(0, 2)).sum())
            assert listed == num_branches - ("zeroed" in extras), (num_samples, listed)
        cases.append((num_samples, mass, kind, labels, values, permutations, seed, want))
    for name, env in (("default", {}), ("the general path", {SWITCH: "0"}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for num_samples, mass, kind, labels, values, permutations, seed, want in cases:
                what = (name, num_samples, permutations)
                with pl.cohort(num_samples) as cohort:
                    cohort.add_cells(mass, None, None)
                    same_edgemodel(cohort.edgemodel(tree, kind, labels, values, permutations, seed, with_stat=True, with_max=True), want, what)
                    # into poisoned buffers on a stream of its own: every cell written; the workspace used again
                    got = device_edgemodel_raw(pl, cohort, tree, kind, labels, values, permutations, seed, num_branches)
                    same_edgemodel(got, want, what + ("raw",))
                    after = cohort.read()
                    assert np.array_equal(after.mass, mass) and not after.best.any(), what      # the cells are not changed
                    fewer = cohort.edgemodel(tree, kind[:1], labels[:, :1].copy(), values[:, :1].copy(), min(permutations, 9), seed)
                    lone = cohort_mod.edgemodel_host(mass, first, kind[:1], labels[:, :1].copy(), values[:, :1].copy(), min(permutations, 9),
                                                     seed)
                    assert fewer.stat is None and fewer.max is None and same_edgemodel(fewer, lone, what + ("the first term alone",))
        for key in env:
            monkeypatch.delenv(key)


@pytest.mark.parametrize("variant", ("default", "the general path"))
def test_strata_and_the_optional_outputs(placer_cls, monkeypatch, variant):
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    if variant != "default":
        monkeypatch.setenv(SWITCH, "0")
    parent, bl, first, db = tree_of(999)
    rng = np.random.default_rng(66)
    num_samples, permutations, seed = 70, 40, 11
    mass = sparser(rng, random_cells(rng, num_samples, 999, empty=2, bits=42))
    kind, labels, values = model_design(rng, num_samples, 3, "alias missing")
    i = np.arange(num_samples)
    strata = np.where(i == 5, 77, np.minimum(i * 7 // num_samples, 2) * 1000000007 % (1 << 32)).astype(np.uint32)  # 3 unequal and a singleton
    want = cohort_mod.edgemodel_host(mass, first, kind, labels, values, permutations, seed, strata=strata)
    plain = cohort_mod.edgemodel_host(mass, first, kind, labels, values, permutations, seed)
    assert want.stat.tobytes() != plain.stat.tobytes()
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(num_samples) as cohort:
        cohort.add_cells(mass, None, None)
        same_edgemodel(device_edgemodel_raw(pl, cohort, tree, kind, labels, values, permutations, seed, 999, strata=strata), want, "strata")
        same_edgemodel(cohort.edgemodel(tree, kind, labels, values, permutations, seed, True, True, strata=strata), want, "strata, sync")
        for with_stat, with_max in ((False, False), (True, False), (False, True)):
            got = device_edgemodel_raw(pl, cohort, tree, kind, labels, values, permutations, seed, 999, with_stat, with_max)
            same_edgemodel(got, plain, (with_stat, with_max))
        lib = capi.load()
        err = lambda: lib.epik_amd_last_error().decode()
        out = np.zeros((len(kind), 999), dtype=capi.EDGEMODEL)
        info, aliased = np.zeros(1, dtype=capi.EDGEMODEL_INFO), np.zeros(64, dtype=np.uint8)
        args = (kind.ctypes.data, labels.ctypes.data, values.ctypes.data, len(kind), permutations, seed, out.ctypes.data, info.ctypes.data, None,
                None, aliased.ctypes.data)
        assert lib.epik_amd_cohort_edgemodel(None, tree._handle, *args) == capi.ERR_INVALID and "null cohort" in err()
        assert lib.epik_amd_cohort_edgemodel(cohort._handle, None, *args) == capi.ERR_INVALID and "null argument" in err()
        assert lib.epik_amd_cohort_edgemodel(cohort._handle, tree._handle, *args[:4], 0, *args[5:]) == capi.ERR_INVALID and "num_permutations" in err()
        assert not out.view(np.uint8).any()                                                     # nothing was written
        assert np.array_equal(cohort.read().mass, mass)


# ---- one handle, changing cells, the siblings in between ---------------------------------------------------------------------
STAGES = ("dense", "thin", "two")
RANKS = (9, 3, 2)
EXTRAS = ("alias missing", "na", "alias")
PERMUTATIONS = (9, 140, 4)                                                                       # (the workspace grows at the second stage)
ORDERS = (("edgetest", "edgemodel", "permanova", "model"), ("edgemodel", "model", "edgetest", "permanova"),
          ("permanova", "edgetest", "model", "edgemodel"))


@pytest.mark.parametrize("variant", ("as created", "the general paths"))
def test_the_edge_model_between_its_siblings_after_the_cells_change(placer_cls, monkeypatch, variant):
    for var in ENV + SWITCHES:
        monkeypatch.delenv(var, raising=False)
    num_branches, s = 999, 70
    parent, bl, first, db = tree_of(num_branches)
    rng = np.random.default_rng(5400)
    dense = random_cells(rng, s, num_branches, empty=1, bits=42)
    thin = sparser(rng, dense)
    with_mass = np.flatnonzero(thin.any(axis=1))
    thin[rng.choice(with_mass, size=(len(with_mass) * 4 + 5) // 10, replace=False)] = 0
    two = np.zeros_like(dense)
    two[[3, s - 2]] = dense[[3, s - 2]]
    stages = []
    for k, (name, mass) in enumerate(zip(STAGES, (dense, thin, two))):
        design, p, seed = model_design(rng, s, RANKS[k], EXTRAS[k]), PERMUTATIONS[k], int(rng.integers(0, 1 << 63))
        factors = group_labels(rng, s, 3)
        kr, totals = cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass)
        want = {"edgemodel": cohort_mod.edgemodel_host(mass, first, *design, p, seed),
                "edgetest": cohort_mod.edgetest_host(mass, first, factors, p, seed),
                "permanova": cohort_mod.permanova_kr_host(kr, totals, factors, p, seed),
                "model": cohort_mod.model_kr_host(kr, totals, *design, p, seed)}
        stages.append((name, mass, design, factors, p, seed, want))
    used = [int(st[-1]["edgemodel"].info["used"]) for st in stages]
    assert used[0] > used[1] > used[2] == 2 and np.isnan(stages[2][-1]["edgemodel"].records["family"]["ss"]).all()
    assert not np.isnan(stages[0][-1]["edgemodel"].records["family"]["p"][0, :, 0]).all()
    if variant != "as created":
        for switch in SWITCHES:
            monkeypatch.setenv(switch, "0")
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(s) as cohort:
        for (name, mass, design, factors, p, seed, want), order in zip(stages, ORDERS):
            cohort.reset()
            cohort.add_cells(mass, None, None)
            for analysis in order:
                what = (variant, name, analysis)
                if analysis == "edgemodel":
                    same_edgemodel(device_edgemodel_raw(pl, cohort, tree, *design, p, seed, num_branches), want["edgemodel"], what)
                elif analysis == "edgetest":
                    same_edgetest(device_edgetest_raw(pl, cohort, tree, factors, p, seed, num_branches), want["edgetest"], what)
                elif analysis == "permanova":
                    got, _, _ = device_permanova_raw(pl, cohort, tree, bl, factors, p, seed, False)
                    same_permanova(got, want["permanova"], what)
                else:
                    got, _, _ = device_model_raw(pl, cohort, tree, bl, *design, p, seed)
                    same_model(got, want["model"], what)
            assert np.array_equal(cohort.read().mass, mass), (variant, name)
