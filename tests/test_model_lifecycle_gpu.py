"""One cohort handle, three sets of cells (dense, thinned, two samples), and at every stage the sequential model between the
principal coordinates, PERMANOVA and PERMDISP -- the analyses that form the squared distances and the Gower centring of the
same matrix -- in an order that changes from stage to stage, with T, R, P and L moving against the stage before: stale state
in the model's workspace (rows of Q beyond L, columns beyond R, the lists of a longer design, the slices of more
permutations) shows only here.  Every byte is compared against the host mirrors, which are computed once per shape.
"""
import numpy as np
import pytest

from epik_amd import cohort as cohort_mod
from test_cohort_cpu import random_cells, same_bits
from test_cohort_gpu import ENV, kr_case, placer_cls  # noqa: F401 (placer_cls: a fixture)
from test_model_cpu import same_model
from test_model_gpu import SWITCH, device_model_raw, model_design
from test_pcoa_cpu import assert_pcoa
from test_pcoa_gpu import device_pcoa_raw
from test_permanova_cpu import same_permanova
from test_permanova_gpu import device_permanova_raw, sparser
from test_permdisp_cpu import same_permdisp
from test_permdisp_gpu import capped_labels, device_permdisp_raw

pytestmark = pytest.mark.gpu
SWITCHES = (SWITCH, "EPIK_AMD_PERMANOVA_LDS", "EPIK_AMD_PCOA_LDS")
ANALYSES = ("pcoa", "permanova", "permdisp", "model")
STAGES = ("dense", "thin", "two")
# the model of the three stages: the rank, the extras and P move against the stage before
RANKS = (9, 3, 2)
EXTRAS = ("alias missing", "na", "alias")
PERMUTATIONS = (9, 21, 4)
COMPONENTS = (5, 2, 5)
ORDERS = (("pcoa", "model", "permanova", "permdisp"), ("model", "permdisp", "pcoa", "permanova"), ("permanova", "pcoa", "permdisp", "model"))
WALK = {}


def walk_of(num_branches, num_samples):
    """[(name, mass, parameters, mirrors)] of a shape, and what keeps the walk from passing vacuously."""
    key = (num_branches, num_samples)
    if key in WALK:
        return WALK[key]
    WALK.clear()
    parent, bl, first, db = kr_case(num_branches)
    rng = np.random.default_rng(5300 + num_branches + num_samples)
    s = num_samples
    dense = random_cells(rng, s, num_branches, empty=1, bits=42)
    thin = sparser(rng, dense)
    with_mass = np.flatnonzero(thin.any(axis=1))
    thin[rng.choice(with_mass, size=(len(with_mass) * 4 + 5) // 10, replace=False)] = 0
    two = np.zeros_like(dense)
    two[[3, s - 2]] = dense[[3, s - 2]]
    stages = []
    for k, (name, mass) in enumerate(zip(STAGES, (dense, thin, two))):
        p = {"design": model_design(rng, s, RANKS[k], EXTRAS[k]), "permutations": PERMUTATIONS[k], "seed": int(rng.integers(0, 1 << 63)),
             "components": COMPONENTS[k], "factors": capped_labels(rng, s, False)}
        kr, totals = cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass)
        want = {"kr": kr, "pcoa": cohort_mod.pcoa_kr_host(kr, totals, p["components"]),
                "permanova": cohort_mod.permanova_kr_host(kr, totals, p["factors"], p["permutations"], p["seed"]),
                "permdisp": cohort_mod.permdisp_kr_host(kr, totals, p["factors"], p["permutations"], p["seed"]),
                "model": cohort_mod.model_kr_host(kr, totals, *p["design"], p["permutations"], p["seed"])}
        stages.append((name, mass, p, want))
    models = [st[3]["model"] for st in stages]
    assert [int(m.info["rank"]) for m in models] == [9, 3, 1] and [len(m.records) for m in models] == [11, 5, 4]
    assert models[0].info["used"] > models[1].info["used"] > models[2].info["used"] == 2
    assert not np.isnan(models[0].records["p"][:9]).any() and not np.isnan(models[1].records["p"][1:]).any()
    assert np.isnan(models[2].records["f"]).all() and models[2].info["df_res"] == 0      # two samples: nothing is left to test with
    WALK[key] = (parent, bl, db, stages)
    return WALK[key]


SHAPES = ((7, 70), (999, 130))
VARIANTS = {"as created": {}, "the general paths": {switch: "0" for switch in SWITCHES}}
WALKS = [(n, s, v) for n, s in SHAPES for v in VARIANTS]


@pytest.mark.parametrize("num_branches, num_samples, variant", WALKS, ids=[f"{n}-{s}-{v.replace(' ', '_')}" for n, s, v in WALKS])
def test_the_model_between_its_siblings_after_the_cells_change(placer_cls, monkeypatch, num_branches, num_samples, variant):
    for var in ENV + SWITCHES:
        monkeypatch.delenv(var, raising=False)
    parent, bl, db, stages = walk_of(num_branches, num_samples)
    for key, value in VARIANTS[variant].items():
        monkeypatch.setenv(key, value)
    import torch
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(num_samples) as cohort:
        for (name, mass, p, want), order in zip(stages, ORDERS):
            cohort.reset()
            cohort.add_cells(mass, None, None)
            d_kr = torch.full((num_samples * num_samples,), np.nan, dtype=torch.float64, device=f"cuda:{pl.device}")
            cohort.kr_device(tree, bl, d_kr.data_ptr())
            torch.cuda.synchronize()
            assert same_bits(d_kr.cpu().numpy().reshape(num_samples, num_samples), want["kr"]), (variant, name)
            for analysis in order:
                what = (variant, name, analysis)
                if analysis == "pcoa":
                    assert_pcoa(device_pcoa_raw(pl, cohort, d_kr, p["components"]), want["pcoa"], what)
                elif analysis == "permanova":
                    got, _, _ = device_permanova_raw(pl, cohort, tree, bl, p["factors"], p["permutations"], p["seed"], False)
                    same_permanova(got, want["permanova"], what)
                elif analysis == "permdisp":
                    same_permdisp(device_permdisp_raw(pl, cohort, d_kr, p["factors"], p["permutations"], p["seed"], False), want["permdisp"], what)
                else:
                    got, kr_before, kr_after = device_model_raw(pl, cohort, tree, bl, *p["design"], p["permutations"], p["seed"])
                    same_model(got, want["model"], what)
                    assert same_bits(kr_before, kr_after), what
            assert same_bits(d_kr.cpu().numpy().reshape(num_samples, num_samples), want["kr"]), (variant, name, "after")
            assert np.array_equal(cohort.read().mass, mass), (variant, name)
