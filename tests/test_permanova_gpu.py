"""PERMANOVA of a cohort's samples over their KR distances on the device: epik_amd_cohort_permanova / _permanova_device against
the host mirror and the rule restated in numpy (test_permanova_cpu), bit for bit, the records and every SSW of every
permutation; a wave, a workgroup and both limits of the ranking stepped over, the general path forced; no side effects; the
errors; and epik-dna --cohort --cohort-permanova end to end.
"""
import os
import subprocess

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, dbfile, synth
from test_cohort_cpu import numpy_first, random_cells, same_bits
from test_cohort_gpu import ENV, _cohort_files, _run, kr_case
from test_profile_gpu import _write_fasta
from test_permanova_cpu import MISSING, numpy_labellings, numpy_permanova, same_permanova

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
SWITCH = "EPIK_AMD_PERMANOVA_LDS"
WAVE_SAMPLES = 128           # up to here a workgroup is one wave (permanova_place.hip: kSmallSamples)
COUNT_POSITIONS = 256        # the most positions the LDS path ranks by counting (kCountPositions); beyond, it sorts
LDS_POSITIONS = 1024         # the most positions of a test whose vectors stay in LDS (kLdsPositions)
SLOTS = 1 + capi.PERMANOVA_PAIR_SLOTS


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def device_permanova_raw(pl, cohort, tree, bl, labels, permutations, seed, pairwise):
    """kr_device, then permanova_device into poisoned buffers on a stream of its own: (Permanova, kr before, kr after)."""
    import torch
    s, m = labels.shape
    slots = SLOTS if pairwise else 1
    d_kr = torch.full((s * s,), np.nan, dtype=torch.float64, device=f"cuda:{pl.device}")
    cohort.kr_device(tree, bl, d_kr.data_ptr())
    torch.cuda.synchronize()
    before = d_kr.cpu().numpy().copy()
    sizes = (m * slots * 56, m * slots * (permutations + 1) * 8, m * 256 * 8)
    bufs = [torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}") for nbytes in sizes]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    cohort.permanova_device(d_kr.data_ptr(), labels, permutations, seed, pairwise, bufs[0].data_ptr(), bufs[1].data_ptr(),
                            bufs[2].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    out, ssw, group_ss = (b.cpu().numpy() for b in bufs)
    got = cohort_mod.Permanova(out.view(capi.PERMANOVA).reshape(m, slots).copy(),
                               ssw.view(np.float64).reshape(m, slots, permutations + 1).copy(),
                               group_ss.view(np.float64).reshape(m, 256).copy())
    return got, before, d_kr.cpu().numpy()


def sparser(rng, mass):
    """`mass` with another 0.9 share zeroed, every sample but the empty ones keeping some mass."""
    out = mass.copy()
    out[rng.random(out.shape) < 0.9] = 0
    out[:, 0] |= (mass.sum(axis=1, dtype=U64) != 0).astype(U64)
    return out


def factor_labels(rng, num_samples, pairwise):
    """labels [S][M]: 2 groups; 3 unbalanced groups with a fifth missing; 7 groups under scattered ids, some of one sample;
    and, without pairwise, a column near 256 groups (every sample its own group up to 250 samples: undefined; beyond, 250
    groups, some of two samples) and one of a single group."""
    s = num_samples
    cols = [rng.integers(0, 2, size=s), np.where(rng.random(s) < 0.2, MISSING, rng.choice(3, size=s, p=[0.6, 0.3, 0.1])),
            np.array([255, 200, 3, 77, 0, 31, 128])[np.minimum(rng.geometric(0.35, size=s) - 1, 6)]]
    if not pairwise:
        cols += [(np.arange(s) * 7 + 5) % 250, np.full(s, 17)]
    return np.ascontiguousarray(np.array(cols, dtype=np.uint32).T)


# S: a wave and a workgroup stepped over, and one size on each side of every limit (one sample of each cohort is empty, so the
# whole column has S - 1 positions at the most); P: 1, and 4 k - 1, 4 k, 4 k + 1 labellings for the workgroups' four
CASES = {7: ((3, 1), (4, 63), (33, 64), (65, 65), (WAVE_SAMPLES, 200), (WAVE_SAMPLES + 1, 63), (130, 1), (COUNT_POSITIONS + 1, 64),
             (COUNT_POSITIONS + 2, 65), (LDS_POSITIONS, 5), (LDS_POSITIONS + 1, 5)),
         999: ((3, 200), (4, 1), (33, 65), (65, 64), (130, 63), (257, 9))}
SMALL = 130                   # up to here the general path and two workgroups are run as well


@pytest.mark.parametrize("num_branches", sorted(CASES))
def test_permanova_equals_the_host_mirror_and_the_restatement_bit_for_bit(placer_cls, monkeypatch, num_branches):
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(num_branches)
    rng = np.random.default_rng(1200 + num_branches)
    cases = []
    for num_samples, permutations in CASES[num_branches]:
        dense = random_cells(rng, num_samples, num_branches, empty=1, bits=42)
        for kind, mass in (("random_cells", dense), ("nine in ten more zeroed", sparser(rng, dense))):
            if kind != "random_cells" and num_samples > SMALL:
                continue
            for pairwise in (False, True):
                if pairwise and num_samples > COUNT_POSITIONS + 1:
                    continue
                labels = factor_labels(rng, num_samples, pairwise)
                seed = int(rng.integers(0, 1 << 63)) * 2 + int(pairwise)
                want = cohort_mod.permanova_host(mass, first, bl, labels, permutations, seed, pairwise)
                restated = numpy_permanova(cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass), labels, permutations,
                                           seed, pairwise)
                same_permanova(want, restated, (num_samples, kind, pairwise))
                cases.append((num_samples, kind, mass, labels, permutations, seed, pairwise, want))
    defined = sum(int((~np.isnan(c[-1].records["p"])).sum()) for c in cases)
    assert defined > 3 * len(cases)
    for name, env in (("default", {}), ("the general path", {SWITCH: "0"}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for num_samples, kind, mass, labels, permutations, seed, pairwise, want in cases:
                if name != "default" and num_samples > SMALL:
                    continue
                what = (name, num_samples, kind, permutations, pairwise)
                with pl.cohort(num_samples) as cohort:
                    cohort.add_cells(mass, None, None)
                    same_permanova(cohort.permanova(tree, bl, labels, permutations, seed, pairwise, with_ssw=True), want, what)
                    # into poisoned buffers on a stream of its own: every cell written; the workspace used again
                    got, kr_before, kr_after = device_permanova_raw(pl, cohort, tree, bl, labels, permutations, seed, pairwise)
                    same_permanova(got, want, what + ("raw",))
                    assert same_bits(kr_before, kr_after), what                                  # d_kr is not changed
                    after = cohort.read()
                    assert np.array_equal(after.mass, mass) and not after.best.any(), what      # nor the cells
                    fewer = cohort.permanova(tree, bl, labels[:, :1].copy(), permutations, seed, pairwise)
                    assert fewer.ssw is None and fewer.records[0].tobytes() == want.records[0].tobytes(), what
        for key in env:
            monkeypatch.delenv(key)


def test_the_errors_of_the_device_entries(placer_cls, monkeypatch):
    import torch
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(999)
    rng = np.random.default_rng(5)
    num_samples = 33
    mass = random_cells(rng, num_samples, 999, empty=4, bits=42)
    labels = factor_labels(rng, num_samples, True)
    lib = capi.load()
    err = lambda: lib.epik_amd_last_error().decode()
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(num_samples) as cohort:
        cohort.add_cells(mass, None, None)
        device = f"cuda:{pl.device}"
        d_kr = torch.full((num_samples * num_samples,), np.nan, dtype=torch.float64, device=device)
        d_out = torch.full((3 * SLOTS * 56,), 0xA5, dtype=torch.uint8, device=device)
        d_ssw = torch.full((3 * SLOTS * 10 * 8,), 0xA5, dtype=torch.uint8, device=device)
        d_group = torch.full((3 * 256 * 8,), 0xA5, dtype=torch.uint8, device=device)
        call = lambda c=cohort._handle, k=d_kr.data_ptr(), l=labels.ctypes.data, m=3, p=9, pw=1, o=d_out.data_ptr(): \
            lib.epik_amd_cohort_permanova_device(c, k, l, m, p, 7, pw, o, d_ssw.data_ptr(), d_group.data_ptr(), None)
        # before any distance: T_s is not on the device yet
        assert call() == capi.ERR_INVALID and "kr_device" in err()
        cohort.kr_device(tree, bl, d_kr.data_ptr())
        torch.cuda.synchronize()
        assert call(c=None) == capi.ERR_INVALID and "null cohort" in err()
        for null in ("k", "l", "o"):
            assert call(**{null: None}) == capi.ERR_INVALID and "null argument" in err(), null
        for bad in (0, 65):
            assert call(m=bad) == capi.ERR_INVALID and "num_columns" in err() and "[1, 64]" in err()
        for bad in (0, 1_000_000):
            assert call(p=bad) == capi.ERR_INVALID and "num_permutations" in err() and "[1, 999999]" in err()
        wrong = labels.copy()
        wrong[17, 2] = 256
        assert call(l=wrong.ctypes.data) == capi.ERR_INVALID and "sample 17" in err() and "column 2" in err() and "256" in err()
        wide = np.arange(num_samples, dtype=np.uint32)[:, None].copy()
        assert call(l=wide.ctypes.data, m=1) == capi.ERR_INVALID and "33 distinct labels" in err()
        from epik_amd.confidence import Tree
        with Tree(pl.device, *kr_case(7)[:2]) as small_tree:
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.permanova(small_tree, bl, labels, 9, 7, True)
            assert e.value.code == capi.ERR_INVALID and "tree" in str(e.value)
        for bad in (dict(labels=labels[:, :0].copy()), dict(permutations=0), dict(permutations=1_000_000)):
            kw = dict(labels=labels, permutations=9)
            kw.update(bad)
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.permanova(tree, bl, kw["labels"], kw["permutations"], 7, True)
            assert e.value.code == capi.ERR_INVALID
        # the poisoned buffers of the refused calls, read back: nothing was written
        torch.cuda.synchronize()
        for buf in (d_out, d_ssw, d_group):
            assert (buf.cpu().numpy() == 0xA5).all()
        # without the optional outputs; then everything, the same records
        assert lib.epik_amd_cohort_permanova_device(cohort._handle, d_kr.data_ptr(), labels.ctypes.data, 3, 9, 7, 1, d_out.data_ptr(),
                                                    None, None, None) == capi.OK
        torch.cuda.synchronize()
        lean = d_out.cpu().numpy().view(capi.PERMANOVA).reshape(3, SLOTS).copy()
        assert call() == capi.OK
        torch.cuda.synchronize()
        want = cohort_mod.permanova_host(mass, first, bl, labels, 9, 7, True)
        got = cohort_mod.Permanova(d_out.cpu().numpy().view(capi.PERMANOVA).reshape(3, SLOTS).copy(),
                                   d_ssw.cpu().numpy().view(np.float64).reshape(3, SLOTS, 10).copy(),
                                   d_group.cpu().numpy().view(np.float64).reshape(3, 256).copy())
        same_permanova(got, want, "after the refusals")
        assert lean.tobytes() == want.records.tobytes()
        after = cohort.read()
    assert np.array_equal(after.mass, mass)


E2E_PERMUTATIONS, E2E_SEED = 99, 2


def test_epik_dna_cohort_permanova_end_to_end(placer_cls, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-dna")
    tree = synth.make_tree(500, seed=13)
    assert tree.num_nodes == 999
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=30, ref_length=500, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    # two groups of six samples, each drawn from its own eight references, a blank sample and one without a label
    plan = [("gut_1", 0), ("skin 1", 1), ("gut_2", 0), ("blank", None), ("skin 2", 1), ("gut_3", 0), ("it's", 1), ("gut_4", 0),
            ("skin 4", 1), ("gut_5", 0), ("skin 5", 1), ("nobody", 0), ("gut_6", 0), ("skin 6", 1)]
    lines, rows = [], []
    (tmp_path / "in").mkdir()
    for i, (name, group) in enumerate(plan):
        if group is None:                                 # no placeable read: the sample is not used
            reads = ["ACG", "AC", "A"] * 15
        else:
            data, offs = synth.make_clade_reads(refs[group * 14:group * 14 + 8], 60, 150, seed=40 + i)
            reads = [bytes(data[int(offs[j]):int(offs[j + 1])]).decode() for j in range(60)]
        _write_fasta(str(tmp_path / "in" / f"s{i}.fasta"), [(f"s{i}_{j}", s) for j, s in enumerate(reads)])
        lines.append(f"{name}\tin/s{i}.fasta")
        state = "NA" if name == "nobody" else "sick" if group in (1, None) else "healthy"
        rows.append(f"{name}\t{state}\t{'abc'[i % 3]}")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    names = [name for name, _ in plan]
    factors_path = tmp_path / "factors.tsv"
    factors_path.write_text("# the design\nsample\tstate\tbatch\nelsewhere\tx\ty\n" + "\n".join(rows) + "\n")
    # that no permutation gives the observed split of the twelve back is a matter of the keys alone: checked here first
    lam = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1])
    mu = numpy_labellings(lam, E2E_SEED, E2E_PERMUTATIONS)[1:]
    assert not ((mu == lam).all(axis=1) | (mu == 1 - lam).all(axis=1)).any()
    flags = ["--cohort-permanova", str(factors_path), "--cohort-permanova-permutations", str(E2E_PERMUTATIONS), "--cohort-permanova-seed",
             str(E2E_SEED), "--cohort-permanova-pairwise"]
    variants = {"plain": ["-j", "1"], "j1": ["-j", "1"] + flags, "j16": ["-j", "16"] + flags,
                "batch50": ["--batch-size", "50", "-j", "16"] + flags, "batch7": ["--batch-size", "7", "-j", "1"] + flags,
                "with the others": ["-j", "4"] + flags + ["--cohort-squash", "--cohort-alpha", "--cohort-dispersion"],
                "others alone": ["-j", "1", "--cohort-squash", "--cohort-alpha", "--cohort-dispersion"]}
    new_name = "cohort_permanova_samples.list.tsv"
    other_names = ["cohort_alpha_samples.list.tsv", "cohort_dispersion_samples.list.tsv", "cohort_squash_samples.list.nwk",
                   "cohort_squash_samples.list.tsv"]
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant.replace(" ", "_"))
        outs[variant].mkdir()
        run = _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + extra)
        older = sorted(p.name for p in _cohort_files(outs[variant]).values())
        new = ([new_name] if "--cohort-permanova" in extra else []) + (other_names if "--cohort-squash" in extra else [])
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(older + new), variant
        assert ("Cohort PERMANOVA: " in run.stdout) == ("--cohort-permanova" in extra)
        assert ("Cohort factors: 2 columns, 1 lines of samples that are not in the list skipped" in run.stdout) == ("--cohort-permanova" in extra)
        for what, path in _cohort_files(outs[variant]).items():                # the three older files: unchanged by the flags
            assert path.read_bytes() == _cohort_files(outs["plain"])[what].read_bytes(), (variant, what)
    permanova_bytes = (outs["j1"] / new_name).read_bytes()
    for variant in ("j16", "batch50", "batch7", "with the others"):
        assert (outs[variant] / new_name).read_bytes() == permanova_bytes, variant
    for name in other_names:                                                   # the other analyses' files: unchanged too
        assert (outs["with the others"] / name).read_bytes() == (outs["others alone"] / name).read_bytes(), name
    # the file is the formatter over the mirror's results for the profile file's cells, and over the device's
    mass, best = cohort_mod.read_profile_tsv(str(_cohort_files(outs["j1"])["profile"]), names, tree.num_nodes)
    totals = cohort_mod.totals_of(mass)
    assert [t > 0 for t in totals] == [name != "blank" for name in names]
    columns, labels, label_names, skipped = cohort_mod.read_factors(str(factors_path), names, True)
    assert columns == ["state", "batch"] and skipped == 1 and label_names[0] == ["healthy", "sick"]
    parent = np.asarray(tree.parent, dtype=np.int64)
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    mirror = cohort_mod.permanova_host(mass, numpy_first(parent), bl, labels, E2E_PERMUTATIONS, E2E_SEED, True)
    state = mirror.records[0, 0]
    assert state["used"] == 12 and state["groups"] == 2 and state["at_most"] == 0 and same_bits(state["p"], 1.0 / (E2E_PERMUTATIONS + 1))
    assert mirror.records[0, 1].tobytes() == state.tobytes()                   # (the two clades separate; the one pair is the whole test)
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as device_tree, pl.cohort(len(names)) as cohort:
        cohort.add_cells(mass, best, None)
        device = cohort.permanova(device_tree, bl, labels, E2E_PERMUTATIONS, E2E_SEED, True, with_ssw=True)
    same_permanova(device, mirror, "end to end")
    text = cohort_mod.format_permanova_tsv(names, totals, columns, label_names, labels, E2E_PERMUTATIONS, E2E_SEED, True, mirror.records,
                                           mirror.group_ss)
    assert permanova_bytes.decode() == text
    assert text.startswith("# epik_amd permanova v1  samples=14 used=13 columns=2 permutations=99 seed=2 pairwise=1\n# unused\tblank\n"
                           "# column\t0\tstate\t12\t2\n# column\t1\tbatch\t13\t3\n# group\t0\t0\thealthy\t6\t")
    back_columns, rows_back, groups, info = cohort_mod.read_permanova_tsv(str(outs["j1"] / new_name))
    assert back_columns == columns and info["unused"] == ["blank"] and info["pairwise"] and len(rows_back) == 2 + 4
    assert rows_back[0][3].tobytes() == state.tobytes() and rows_back[1][1:3] == ("healthy", "sick")
