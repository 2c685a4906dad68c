"""The sequential model of a cohort's samples over their distances on the device: epik_amd_cohort_model / _model_device
against the host mirror and the rule restated in numpy (test_model_cpu), bit for bit: the records, the info block, the aliased
bytes and every F of every permutation; a wave, a workgroup, the ranking's tile and the LDS limit stepped over, both register
tiers and every number of passes over B, the general path forced; no side effects; the errors; a UniFrac distance.
"""
import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod
from test_cohort_cpu import random_cells, same_bits
from test_cohort_gpu import ENV, kr_case
from test_model_cpu import MISSING, design, numpy_model, same_model

pytestmark = pytest.mark.gpu
U64 = np.uint64
SWITCH = "EPIK_AMD_MODEL_LDS"
PERMS = 4                    # the permutations a workgroup carries through one pass over B (model_place.hip: kPerms)
CHUNK = 8                    # the columns a lane accumulates at a time (kChunk) ...
SMALL_COLUMNS = 4            # ... and in a design of up to this many columns (kSmallColumns)
LDS_POSITIONS = 128          # the most samples whose row sums stay in LDS (kLdsPositions)
BLOCK = 256                  # the lanes of a workgroup: beyond, a lane owns more than one row
KEY_TILE = 1024              # the keys permutation_rank ranks against at a time (cohort_device.hpp: kCohortKeyTile)
SMALL = 130                  # up to here the general path and two workgroups are run as well


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def model_design(rng, num_samples, rank, extras):
    """A design whose rank is `rank` when there are more used samples than that: covariates, one a term, up to 12; beyond, two
    factors of 32 labels and covariates.  "alias": the first covariate again, last (one column more, dropped); "na": a factor
    of one group, first (no column, an NA record); "missing": a value and a label missing somewhere."""
    s = num_samples
    covariates = rank if rank <= 12 else rank - 62
    terms = [("n", rng.normal(size=s)) for _ in range(covariates)]
    if rank > 12:
        terms = [("f", rng.permutation(np.arange(s) % 32).astype(np.uint32)), ("f", rng.permutation(np.arange(s) % 32).astype(np.uint32))] + terms
    if "alias" in extras:
        terms.append(("n", terms[-1][1].copy()))
    if "na" in extras:
        terms.insert(0, ("f", np.full(s, 9, dtype=np.uint32)))
    kind, labels, values = design(*terms)
    if "missing" in extras and s > 8:
        values[s // 2, kind.argmax()] = np.nan
        if not kind.all():
            labels[s // 3, kind.argmin()] = MISSING
    return kind, labels, values


# (S, P, rank, extras).  S: a wave, the workgroup's lanes, the LDS limit and the ranking's tile stepped over (one sample of each
# cohort is empty; the designs at the two largest sizes miss nothing, so L = S - 1 sits on each side of the tile).  The rank: 1,
# each side of the small tier (a design of 4 and of 5 columns), 8 and 9 (one pass over B and two), 63 and 64 (eight).
# P: 1, and 4 k - 1, 4 k, 4 k + 1 permutations for the workgroups' four; small where S is large.
CASES = {7: ((3, 1, 1, ""), (64, 7, 4, "missing"), (65, 8, 4, "alias missing"), (66, 9, 5, "na missing"), (67, 8, 8, "missing"),
             (LDS_POSITIONS, 7, 9, "alias missing"), (LDS_POSITIONS + 1, 9, 9, "na"), (SMALL, 8, 63, "alias"),
             (BLOCK + 1, 5, 2, "na missing"), (BLOCK + 2, 5, 64, ""), (KEY_TILE + 1, 5, 9, "alias"), (KEY_TILE + 2, 3, 3, "na")),
         999: ((5, 9, 1, "na"), (33, 8, 4, "missing"), (65, 7, 12, "alias missing"), (SMALL, 9, 64, ""), (200, 8, 5, "alias na missing"))}


def device_model_raw(pl, cohort, tree, bl, kind, labels, values, permutations, seed):
    """kr_device, then model_device into poisoned buffers on a stream of its own: (Model, kr before, kr after)."""
    import torch
    s, t = labels.shape
    d_kr = torch.full((s * s,), np.nan, dtype=torch.float64, device=f"cuda:{pl.device}")
    cohort.kr_device(tree, bl, d_kr.data_ptr())
    torch.cuda.synchronize()
    before = d_kr.cpu().numpy().copy()
    sizes = ((t + 1) * 48, 40, (t + 1) * (permutations + 1) * 8, 64)
    bufs = [torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}") for nbytes in sizes]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    cohort.model_device(d_kr.data_ptr(), kind, labels, values, permutations, seed, bufs[0].data_ptr(), bufs[1].data_ptr(),
                        bufs[3].data_ptr(), bufs[2].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    out, info, stat, aliased = (b.cpu().numpy() for b in bufs)
    got = cohort_mod.Model(out.view(capi.MODEL_TERM).copy(), info.view(capi.MODEL_INFO)[0].copy(),
                           stat.view(np.float64).reshape(t + 1, permutations + 1).copy(), aliased.copy())
    return got, before, d_kr.cpu().numpy()


@pytest.mark.parametrize("num_branches", sorted(CASES))
def test_model_equals_the_host_mirror_and_the_restatement_bit_for_bit(placer_cls, monkeypatch, num_branches):
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(num_branches)
    rng = np.random.default_rng(2100 + num_branches)
    cases = []
    for num_samples, permutations, rank, extras in CASES[num_branches]:
        mass = random_cells(rng, num_samples, num_branches, empty=1, bits=42)
        kind, labels, values = model_design(rng, num_samples, rank, extras)
        seed = int(rng.integers(0, 1 << 63))
        kr, totals = cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass)
        want = cohort_mod.model_kr_host(kr, totals, kind, labels, values, permutations, seed)
        same_model(want, numpy_model(kr, totals, kind, labels, values, permutations, seed), (num_samples, "the restatement"))
        if num_samples > 2 * rank + 4:
            assert want.info["rank"] == rank and want.aliased.sum() == ("alias" in extras), (num_samples, want.info)
            # (a term of no accepted column is an NA record: the factor of one group and the covariate given again)
            assert np.isnan(want.records["p"]).sum() == ("na" in extras) + ("alias" in extras), (num_samples, want.records)
        if "missing" not in extras:
            assert want.info["used"] == num_samples - (num_samples > 1)
        cases.append((num_samples, mass, kind, labels, values, permutations, seed, want))
    records = sum(len(c[-1].records) for c in cases)
    defined = sum(int((~np.isnan(c[-1].records["p"])).sum()) for c in cases)
    assert 2 * defined > records, (defined, records)
    assert any(c[-1].aliased.any() for c in cases) and any(np.isnan(c[-1].records["p"]).any() for c in cases)
    for name, env in (("default", {}), ("the general path", {SWITCH: "0"}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for num_samples, mass, kind, labels, values, permutations, seed, want in cases:
                if name != "default" and num_samples > SMALL:
                    continue
                what = (name, num_samples, permutations)
                with pl.cohort(num_samples) as cohort:
                    cohort.add_cells(mass, None, None)
                    same_model(cohort.model(tree, bl, kind, labels, values, permutations, seed, with_stat=True), want, what)
                    # into poisoned buffers on a stream of its own: every cell written; the workspace used again
                    got, kr_before, kr_after = device_model_raw(pl, cohort, tree, bl, kind, labels, values, permutations, seed)
                    same_model(got, want, what + ("raw",))
                    assert same_bits(kr_before, kr_after), what                                  # d_kr is not changed
                    after = cohort.read()
                    assert np.array_equal(after.mass, mass) and not after.best.any(), what      # nor the cells
                    fewer = cohort.model(tree, bl, kind[:1], labels[:, :1].copy(), values[:, :1].copy(), permutations, seed)
                    lone = cohort_mod.model_host(mass, first, bl, kind[:1], labels[:, :1].copy(), values[:, :1].copy(), permutations, seed)
                    assert fewer.stat is None and same_model(fewer, lone, what + ("the first term alone",))
        for key in env:
            monkeypatch.delenv(key)


def test_model_over_a_unifrac_distance_and_the_errors_of_the_device_entry(placer_cls, monkeypatch):
    import torch
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(999)
    rng = np.random.default_rng(8)
    num_samples, permutations, seed = 41, 9, 7
    mass = random_cells(rng, num_samples, 999, empty=4, bits=42)
    kind, labels, values = model_design(rng, num_samples, 3, "alias na missing")
    terms = len(kind)
    lib = capi.load()
    err = lambda: lib.epik_amd_last_error().decode()
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(num_samples) as cohort:
        cohort.add_cells(mass, None, None)
        device = f"cuda:{pl.device}"
        d_kr = torch.full((num_samples * num_samples,), np.nan, dtype=torch.float64, device=device)
        sizes = ((terms + 1) * 48, 40, (terms + 1) * (permutations + 1) * 8, 64)
        d_out, d_info, d_stat, d_aliased = (torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=device) for nbytes in sizes)

        def call(c=cohort._handle, k=d_kr.data_ptr(), kd=kind, la=labels, va=values, t=terms, p=permutations, o=d_out.data_ptr(),
                 i=d_info.data_ptr(), a=d_aliased.data_ptr()):
            kd, la, va = (None if v is None else np.ascontiguousarray(v) for v in (kd, la, va))
            return lib.epik_amd_cohort_model_device(c, k, *(None if v is None else v.ctypes.data for v in (kd, la, va)), t, p, seed, o, i,
                                                    d_stat.data_ptr(), a, None)

        # before any distance: T_s is not on the device yet
        assert call() == capi.ERR_INVALID and "kr_device" in err()
        cohort.unifrac_device(tree, bl, "unweighted", d_kr.data_ptr())
        torch.cuda.synchronize()
        assert call(c=None) == capi.ERR_INVALID and "null cohort" in err()
        for null in ("k", "kd", "la", "va", "o", "i", "a"):
            assert call(**{null: None}) == capi.ERR_INVALID and "null argument" in err(), null
        for bad in (0, 17):
            assert call(t=bad) == capi.ERR_INVALID and "num_terms" in err() and "[1, 16]" in err()
        for bad in (0, 1_000_000):
            assert call(p=bad) == capi.ERR_INVALID and "num_permutations" in err() and "[1, 999999]" in err()
        wrong = labels.copy()
        wrong[17, 0] = 32
        assert call(la=wrong) == capi.ERR_INVALID and "sample 17" in err() and "term 0" in err() and "32" in err()
        wrong = values.copy()
        wrong[23, 1] = np.inf
        assert call(va=wrong) == capi.ERR_INVALID and "sample 23" in err() and "infinite" in err()
        wide = design(*[("f", (np.arange(num_samples) * (t + 1)) % 23) for t in range(terms)])
        assert call(kd=wide[0], la=wide[1], va=wide[2]) == capi.ERR_INVALID and "columns" in err() and "64" in err()
        # the poisoned buffers of the refused calls, read back: nothing was written
        torch.cuda.synchronize()
        for buf in (d_out, d_info, d_stat, d_aliased):
            assert (buf.cpu().numpy() == 0xA5).all()
        # model_device over the matrix of a UniFrac distance is model_metric with that distance, and the host mirror's
        assert call() == capi.OK
        torch.cuda.synchronize()
        got = cohort_mod.Model(d_out.cpu().numpy().view(capi.MODEL_TERM).copy(), d_info.cpu().numpy().view(capi.MODEL_INFO)[0].copy(),
                               d_stat.cpu().numpy().view(np.float64).reshape(terms + 1, permutations + 1).copy(), d_aliased.cpu().numpy().copy())
        want = cohort_mod.model_host(mass, first, bl, kind, labels, values, permutations, seed, metric="unweighted")
        same_model(got, want, "model_device over unweighted UniFrac")
        same_model(cohort.model(tree, bl, kind, labels, values, permutations, seed, with_stat=True, metric="unweighted"), want, "model_metric")
        assert not same_bits(want.records["ss"], cohort_mod.model_host(mass, first, bl, kind, labels, values, permutations, seed).records["ss"])
        after = cohort.read()
    assert np.array_equal(after.mass, mass)
