"""The Mantel and partial Mantel tests and ANOSIM of a cohort's samples on the device: epik_amd_cohort_mantel / _mantel_device and
_anosim / _anosim_device against the host mirror bit for bit, the records and every stat[p], and against the rule restated in numpy
(test_mantel_cpu) where that is fast enough; both methods, with and without a control, column and matrix sides, with and without
strata; the seams named by the kernels' constants (the tiers of the key ranking, the LDS tile of the triangle sort, the LDS tiers
of the permutations' vectors, two workgroups); no side effects; one handle called with one side, three sides and a control, one
side again, a PERMANOVA in between; another metric; the errors; and epik-dna and epik.py end to end with the new flags.
"""
import os

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod
from test_cohort_cpu import random_cells, same_bits
from test_cohort_gpu import ENV, kr_case
from test_mantel_cpu import anosim_labels, mantel_sides, numpy_anosim, numpy_mantel, same_anosim, same_mantel
from test_permanova_cpu import same_permanova

pytestmark = pytest.mark.gpu
U64 = np.uint64
SWITCH = "EPIK_AMD_MANTEL_LDS"
PERMS = 4                     # the permutations of a workgroup's pass (mantel_place.hip: kPerms)
COUNT_POSITIONS = 256         # up to here the LDS path ranks the keys by counting; beyond, it sorts (kCountPositions)
SORT_TILE = 4096              # the values of the triangle sort that are sorted in LDS (kSortTile)
LDS_CONTROL_POSITIONS = 512   # the most samples whose vectors stay in LDS with a control (kLdsControlPositions)
LDS_POSITIONS = 1024          # ... and without (kLdsPositions)
BOTH = ("pearson", "spearman")


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


# (S, P) of the issue, one sample of each cohort empty; the chunk of four permutations stepped over at S = 4; then a list beyond
# the counting tier of the keys, and a cohort on each side of the two LDS tiers (there with the first two sides only)
CASES = ((3, 1), (4, 63), (33, 64), (65, 65), (129, 200), (257, 9), (4, 4 * PERMS + 1), (COUNT_POSITIONS + 3, 5),
         (LDS_CONTROL_POSITIONS + 2, 2), (LDS_POSITIONS + 2, 2))
SMALL = 65                    # up to here the general path and two workgroups are run as well, and the restatement
LEAN_FROM = 400               # from here a case has two columns and a matrix, pearson and spearman, one control
CASE_DATA = {}


def strata_of(num_samples):
    """Three strata of unequal size and a singleton."""
    strata = np.minimum(np.arange(num_samples) * 7 % 10, 4).astype(np.uint32) // 2 * 5      # a fifth, a fifth and three fifths
    strata[num_samples // 3] = 1000
    return strata


def case_data(num_samples, permutations):
    """(mass, kr, totals, values, matrices, present, labels, seed, [(control, strata, Mantel)], [(strata, Anosim)]) by the host mirror."""
    key = (num_samples, permutations)
    if key not in CASE_DATA:
        parent, bl, first, db = kr_case(7)
        rng = np.random.default_rng(3100 + num_samples + permutations)
        mass = random_cells(rng, num_samples, 7, empty=1, bits=42)
        kr, totals = cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass)
        values, matrices, present = mantel_sides(rng, kr)
        labels = anosim_labels(rng, num_samples)
        if num_samples >= LEAN_FROM:
            values, matrices, present, labels = values[:2].copy(), matrices[:1].copy(), present[:1].copy(), labels[:, :2].copy()
        seed = int(rng.integers(0, 1 << 63))
        strata = strata_of(num_samples)
        matrix = len(values)                                        # the first matrix's side
        variants = ((0, None),) if num_samples >= LEAN_FROM else ((None, None), (0, None), (matrix, strata), (None, strata))
        mantel = [(control, layers, cohort_mod.mantel_kr_host(kr, totals, values, matrices, present, BOTH, control, permutations, seed,
                                                               strata=layers)) for control, layers in variants]
        anosim = [(layers, cohort_mod.anosim_kr_host(kr, totals, labels, permutations, seed, strata=layers)) for layers in (None, strata)]
        if num_samples <= SMALL and permutations <= 65:             # (the restatement is slow: the small cases)
            for control, layers, want in mantel[1:3]:
                same_mantel(want, numpy_mantel(kr, totals, values, matrices, present, BOTH, control, permutations, seed, layers), key)
            for layers, want in anosim:
                same_anosim(want, numpy_anosim(kr, totals, labels, permutations, seed, layers), key)
        CASE_DATA[key] = (mass, kr, totals, values, matrices, present, labels, seed, mantel, anosim)
    return CASE_DATA[key]


def poisoned(pl, nbytes):
    import torch
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}")


def device_mantel_raw(pl, cohort, d_dist, values, matrices, present, methods, control, permutations, seed, strata=None):
    """mantel_device over d_dist into poisoned buffers on a stream of its own: a `Mantel` as the device left it."""
    import torch
    tests = sum(len(side) for side in (values, matrices) if side is not None) * len(methods)
    out, stat = poisoned(pl, tests * 64), poisoned(pl, tests * (permutations + 1) * 8)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    cohort.mantel_device(d_dist.data_ptr(), values, matrices, present, methods, control, permutations, seed, out.data_ptr(),
                         stat.data_ptr(), stream.cuda_stream, strata)
    stream.synchronize()
    torch.cuda.synchronize()
    return cohort_mod.Mantel(out.cpu().numpy().view(capi.MANTEL).copy(),
                             stat.cpu().numpy().view(np.float64).reshape(tests, permutations + 1).copy())


def device_anosim_raw(pl, cohort, d_dist, labels, permutations, seed, strata=None):
    import torch
    m = labels.shape[1]
    out, stat = poisoned(pl, m * 48), poisoned(pl, m * (permutations + 1) * 8)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    cohort.anosim_device(d_dist.data_ptr(), labels, permutations, seed, out.data_ptr(), stat.data_ptr(), stream.cuda_stream, strata)
    stream.synchronize()
    torch.cuda.synchronize()
    return cohort_mod.Anosim(out.cpu().numpy().view(capi.ANOSIM).copy(), stat.cpu().numpy().view(np.float64).reshape(m, permutations + 1).copy())


def test_the_cases_cross_every_seam_and_cannot_pass_on_na_alone():
    """Counted on the host mirror's output: more than half of the records with used >= 3 are defined; a list on each side of the
    counting tier of the keys; a triangle above the sort's LDS tile and one below it; a cohort on each side of both LDS tiers."""
    exist = defined = 0
    used = {}
    for num_samples, permutations in CASES:
        data = case_data(num_samples, permutations)
        for _, _, want in data[8]:
            exist += int((want.records["used"] >= 3).sum())
            defined += int((~np.isnan(want.records["p"])).sum())
        used[num_samples] = int(max(want.records["used"].max() for _, _, want in data[8]))
    assert 2 * defined > exist > 200, (defined, exist)
    pairs = {s: n * (n - 1) // 2 for s, n in used.items()}
    assert used[257] <= COUNT_POSITIONS < used[COUNT_POSITIONS + 3]
    assert pairs[65] < SORT_TILE < pairs[129] and pairs[129] == 8128
    assert 257 <= LDS_CONTROL_POSITIONS < CASES[-2][0] <= LDS_POSITIONS < CASES[-1][0]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"S{c[0]}-P{c[1]}")
def test_mantel_and_anosim_equal_the_host_mirror_bit_for_bit(placer_cls, monkeypatch, case):
    import torch
    num_samples, permutations = case
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(7)
    mass, kr, totals, values, matrices, present, labels, seed, mantel, anosim = case_data(num_samples, permutations)
    paths = (("default", {}),)
    if num_samples <= SMALL:
        paths += (("the general path", {SWITCH: "0"}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"}))
    for name, env in paths:
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(num_samples) as cohort:
            cohort.add_cells(mass, None, None)
            d_dist = torch.full((num_samples * num_samples,), np.nan, dtype=torch.float64, device=f"cuda:{pl.device}")
            cohort.kr_device(tree, bl, d_dist.data_ptr())
            torch.cuda.synchronize()
            before = d_dist.cpu().numpy().copy()
            assert same_bits(before.reshape(num_samples, num_samples), kr)
            for control, strata, want in mantel:
                what = (name, num_samples, permutations, control, strata is not None)
                got = cohort.mantel(tree, bl, values, matrices, present, BOTH, control, permutations, seed, strata=strata, with_stat=True)
                same_mantel(got, want, what)
                # into poisoned buffers on a stream of its own: every cell written; the workspace used again
                same_mantel(device_mantel_raw(pl, cohort, d_dist, values, matrices, present, BOTH, control, permutations, seed, strata),
                            want, what + ("raw",))
            lean = cohort.mantel(tree, bl, values[:1], None, None, ("spearman",), None, permutations, seed)
            assert lean.stat is None and lean.records[0].tobytes() == mantel[0][2].records[1].tobytes()   # (side 0 is tested plainly)
            for strata, want in anosim:
                what = (name, num_samples, permutations, "anosim", strata is not None)
                same_anosim(cohort.anosim(tree, bl, labels, permutations, seed, strata=strata, with_stat=True), want, what)
                same_anosim(device_anosim_raw(pl, cohort, d_dist, labels, permutations, seed, strata), want, what + ("raw",))
            assert same_bits(d_dist.cpu().numpy(), before), name                            # d_dist is not changed
            after = cohort.read()
            assert np.array_equal(after.mass, mass) and not after.best.any(), name          # nor the cells
        for key in env:
            monkeypatch.delenv(key)


def test_one_handle_grows_its_workspace_and_a_permanova_runs_in_between(placer_cls, monkeypatch):
    """One side; three sides, both methods and a control, whose workspace is larger (a third table, the sort's buffer, a matrix);
    one side again, carved from the larger buffer; a PERMANOVA on the same handle in between."""
    import torch
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(7)
    rng = np.random.default_rng(3177)
    mass = random_cells(rng, 70, 7, empty=1, bits=42)
    kr, totals = cohort_mod.kr_host(mass, first, bl), cohort_mod.totals_of(mass)
    values, matrices, present = mantel_sides(rng, kr)
    factors = anosim_labels(rng, 70)[:, :2].copy()
    one = (values[:1], None, None, ("pearson",), None, 9, 5)
    three = (values[:2], matrices[:1], present[:1], BOTH, 1, 9, 6)
    nova = cohort_mod.permanova_kr_host(kr, totals, factors, 9, 7)
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(70) as cohort:
        cohort.add_cells(mass, None, None)
        d_dist = torch.full((70 * 70,), np.nan, dtype=torch.float64, device=f"cuda:{pl.device}")
        cohort.kr_device(tree, bl, d_dist.data_ptr())
        torch.cuda.synchronize()
        for k, call in enumerate((one, three, one)):
            want = cohort_mod.mantel_kr_host(kr, totals, *call)
            assert not np.isnan(want.records["p"]).any()
            same_mantel(device_mantel_raw(pl, cohort, d_dist, *call), want, ("call", k + 1))
            same_permanova(cohort.permanova(tree, bl, factors, 9, 7, with_ssw=True), nova, ("permanova after call", k + 1))
            same_anosim(device_anosim_raw(pl, cohort, d_dist, factors, 9, 7), cohort_mod.anosim_kr_host(kr, totals, factors, 9, 7), k)
        assert same_bits(d_dist.cpu().numpy().reshape(70, 70), kr)


def test_another_metric_is_the_host_mirror_fed_that_matrix(placer_cls, monkeypatch):
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(7)
    rng = np.random.default_rng(3188)
    mass = random_cells(rng, 33, 7, empty=1, bits=42)
    matrix, totals = cohort_mod.unifrac_host(mass, first, bl, "unweighted"), cohort_mod.totals_of(mass)
    values, matrices, present = mantel_sides(rng, cohort_mod.kr_host(mass, first, bl))
    labels = anosim_labels(rng, 33)
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(33) as cohort:
        cohort.add_cells(mass, None, None)
        got = cohort.mantel(tree, bl, values, matrices, present, BOTH, 0, 20, 3, metric="unweighted", with_stat=True)
        same_mantel(got, cohort_mod.mantel_kr_host(matrix, totals, values, matrices, present, BOTH, 0, 20, 3), "unweighted")
        assert not np.isnan(got.records["p"][:4]).any()
        same_anosim(cohort.anosim(tree, bl, labels, 20, 3, metric="unweighted", with_stat=True),
                    cohort_mod.anosim_kr_host(matrix, totals, labels, 20, 3), "unweighted")
        same_mantel(cohort_mod.mantel_host(mass, first, bl, values, matrices, present, BOTH, 0, 20, 3, metric="unweighted"), got)


def test_the_errors(placer_cls, monkeypatch):
    import torch
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(7)
    lib = capi.load()
    err = lambda: lib.epik_amd_last_error().decode()
    s = 6
    values, matrices, present = np.zeros((65, s)), np.zeros((9, s, s)), np.ones((9, s), np.uint8)
    values[:, :] = np.arange(s)
    labels = np.array([[0, 0, 0, 1, 1, 1]], np.uint32).T.copy()
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(s) as cohort:
        mass = np.zeros((s, 7), U64)
        mass[:, 0] = 1
        cohort.add_cells(mass, None, None)
        d_dist = torch.full((s * s,), np.nan, dtype=torch.float64, device=f"cuda:{pl.device}")
        d_out, d_rank = poisoned(pl, 130 * 64), poisoned(pl, 48)
        call = lambda c=cohort._handle, k=d_dist.data_ptr(), v=values.ctypes.data, mv=1, m=matrices.ctypes.data, pr=present.ctypes.data, \
            mm=1, methods=3, control=capi.MANTEL_NO_CONTROL, p=9, o=d_out.data_ptr(): lib.epik_amd_cohort_mantel_device(
                c, k, v, mv, m, pr, mm, methods, control, p, 7, None, o, None, None)
        again = lambda c=cohort._handle, k=d_dist.data_ptr(), l=labels.ctypes.data, m=1, p=9, o=d_rank.data_ptr(): \
            lib.epik_amd_cohort_anosim_device(c, k, l, m, p, 7, None, o, None, None)
        # before any distance: T_s is not on the device yet
        assert call() == capi.ERR_INVALID and "kr_device" in err()
        assert again() == capi.ERR_INVALID and "kr_device" in err()
        cohort.kr_device(tree, bl, d_dist.data_ptr())
        torch.cuda.synchronize()
        assert call(c=None) == capi.ERR_INVALID and "null cohort" in err()
        assert again(c=None) == capi.ERR_INVALID and "null cohort" in err()
        for null in ("k", "o", "v", "m", "pr"):
            assert call(**{null: None}) == capi.ERR_INVALID and "null argument" in err(), null
        for null in ("k", "l", "o"):
            assert again(**{null: None}) == capi.ERR_INVALID and "null argument" in err(), null
        for bad, words in ((dict(mv=65), ("num_columns", "[0, 64]")), (dict(mm=9), ("num_matrices", "[0, 8]")), (dict(mv=0, mm=0), ("side",)),
                           (dict(control=2), ("control = 2", "no side")), (dict(methods=0), ("methods",)), (dict(p=0), ("num_permutations",)),
                           (dict(p=1_000_000), ("[1, 999999]",))):
            assert call(**bad) == capi.ERR_INVALID and all(w in err() for w in words), (bad, err())
        for bad in (dict(m=0), dict(m=65), dict(p=0)):
            assert again(**bad) == capi.ERR_INVALID, bad
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0xA5).all() and (d_rank.cpu().numpy() == 0xA5).all()  # the refused calls wrote nothing
        assert call() == capi.OK and again() == capi.OK
        torch.cuda.synchronize()
        closed = cohort
    with pytest.raises(capi.EpikAmdError, match="null cohort"):
        closed.mantel_device(1, values[:1], d_out=1)
    with pytest.raises(capi.EpikAmdError, match="null cohort"):
        closed.anosim_device(1, labels, 9, 1, 1)
    # more than 8 192 samples: refused by the argument check alone, ahead of the check that the cohort has distances, which itself
    # comes ahead of the workspace: nothing of that size is allocated, and the pointers are never followed
    with placer_cls.from_synth(db) as pl, pl.cohort(capi.MANTEL_MAX_SAMPLES + 1) as wide:
        big = capi.MANTEL_MAX_SAMPLES + 1
        column, factor = np.zeros((1, big)), np.zeros((big, 1), np.uint32)
        assert lib.epik_amd_cohort_mantel_device(wide._handle, 1, column.ctypes.data, 1, None, None, 0, 1, capi.MANTEL_NO_CONTROL, 9, 1,
                                                 None, 1, None, None) == capi.ERR_INVALID and "8192" in err()
        assert lib.epik_amd_cohort_anosim_device(wide._handle, 1, factor.ctypes.data, 1, 9, 1, None, 1, None, None) == capi.ERR_INVALID
        assert "8192" in err()


# ---- the drivers, end to end ------------------------------------------------------------------------------------------------
def test_the_drivers_end_to_end(placer_cls, tmp_path):
    """epik-dna and epik.py --cohort with the Mantel flags (a metadata file, a matrix file, both methods, a side held fixed),
    --cohort-anosim and --cohort-strata on 13 samples: the two files are the same bytes at -j 1 and -j 4 and two batch sizes and
    from the launcher, are the formatters over the host mirror's and the device's records for the profile file's cells, and read
    back; over another distance the first line says so; every other cohort file of the run is unchanged by the flags."""
    import subprocess
    import sys
    from epik_amd import dbfile, synth
    from test_cohort_cpu import numpy_first
    from test_cohort_gpu import _cohort_files, _run
    from test_mantel_cpu import matrix_text
    from test_profile_gpu import _write_fasta
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    driver = os.path.join(root, "epik_amd", "bin", "epik-dna")
    tree = synth.make_tree(500, seed=13)
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=30, ref_length=500, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    plan = [("gut_1", 0), ("skin 1", 1), ("gut_2", 0), ("blank", None), ("skin 2", 1), ("gut_3", 0), ("it's", 1), ("gut_4", 0),
            ("skin 4", 1), ("gut_5", 0), ("skin 5", 1), ("gut_6", 0), ("skin 6", 1)]
    names = [name for name, _ in plan]
    rng = np.random.default_rng(77)
    lines, meta_rows, factor_rows = [], [], []
    (tmp_path / "in").mkdir()
    for i, (name, group) in enumerate(plan):
        if group is None:                                 # no placeable read: the sample is not used
            reads = ["ACG", "AC", "A"] * 15
        else:
            data, offs = synth.make_clade_reads(refs[group * 14:group * 14 + 8], 60, 150, seed=40 + i)
            reads = [bytes(data[int(offs[j]):int(offs[j + 1])]).decode() for j in range(60)]
        _write_fasta(str(tmp_path / "in" / f"s{i}.fasta"), [(f"s{i}_{j}", s) for j, s in enumerate(reads)])
        lines.append(f"{name}\tin/s{i}.fasta")
        ph = "NA" if name == "gut_5" else f"{5 + 2 * (group or 0) + (3 * i) % 7 / 8}"
        meta_rows.append(f"{name}\t{ph}\t{(5 * i) % 4}")
        factor_rows.append(f"{name}\t{'sick' if group in (1, None) else 'healthy'}\tperson {i % 4}")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    meta_path, factor_path, geo_path = tmp_path / "meta.tsv", tmp_path / "factors.tsv", tmp_path / "geo.tsv"
    meta_path.write_text("# the metadata\nsample\tph\tdepth\nelsewhere\t1\t2\n" + "\n".join(meta_rows) + "\n")
    factor_path.write_text("sample\tstate\tsubject\n" + "\n".join(factor_rows) + "\n")
    noise = rng.random((13, 13))
    geo = np.where(np.eye(13, dtype=bool), 0.0, noise + noise.T)
    in_file = [i for i, name in enumerate(names) if name != "skin 4"][::-1]         # the file lacks a sample and has its own order
    geo_path.write_text(matrix_text([names[i] for i in in_file], geo[np.ix_(in_file, in_file)]))
    present = np.array([[name != "skin 4" for name in names]], np.uint8)
    flags = ["--cohort-mantel", str(meta_path), "--cohort-mantel-matrix", f"geo={geo_path}", "--cohort-mantel-method", "both",
             "--cohort-mantel-partial", "depth", "--cohort-mantel-permutations", "99", "--cohort-mantel-seed", "3",
             "--cohort-anosim", str(factor_path), "--cohort-anosim-permutations", "99", "--cohort-anosim-seed", "4",
             "--cohort-strata", str(factor_path), "--cohort-strata-column", "subject"]
    variants = {"plain": ["-j", "1"], "j1": ["-j", "1"] + flags, "j4": ["-j", "4"] + flags,
                "batch50": ["--batch-size", "50", "-j", "4"] + flags, "batch7": ["--batch-size", "7", "-j", "1"] + flags,
                "with the others": ["-j", "4"] + flags + ["--cohort-squash", "--cohort-alpha"],
                "others alone": ["-j", "1", "--cohort-squash", "--cohort-alpha"],
                "unweighted": ["-j", "4"] + flags + ["--cohort-distance", "unweighted"]}
    new_names = ["cohort_anosim_samples.list.tsv", "cohort_mantel_samples.list.tsv"]
    other_names = ["cohort_alpha_samples.list.tsv", "cohort_squash_samples.list.nwk", "cohort_squash_samples.list.tsv"]
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant.replace(" ", "_"))
        outs[variant].mkdir()
        run = _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + extra)
        older = sorted(p.name for p in _cohort_files(outs[variant]).values())
        new = (new_names if "--cohort-mantel" in extra else []) + (other_names if "--cohort-squash" in extra else [])
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(older + new), variant
        assert ("Cohort Mantel sides: 2 columns, 1 matrices, 1 lines of samples that are not in the list skipped" in run.stdout) == \
            ("--cohort-mantel" in extra), run.stdout
        assert ("Cohort ANOSIM: " in run.stdout) == ("--cohort-anosim" in extra)
        for what, path in _cohort_files(outs[variant]).items():                # the three older files: unchanged by the flags
            assert path.read_bytes() == _cohort_files(outs["plain"])[what].read_bytes(), (variant, what)
    for name in new_names:
        for variant in ("j4", "batch50", "batch7", "with the others"):
            assert (outs[variant] / name).read_bytes() == (outs["j1"] / name).read_bytes(), (variant, name)
    for name in other_names:                                                   # the other analyses' files: unchanged too
        assert (outs["with the others"] / name).read_bytes() == (outs["others alone"] / name).read_bytes(), name
    # the launcher passes the flags on: the same bytes
    launched = tmp_path / "launcher"
    launched.mkdir()
    _run([sys.executable, os.path.join(root, "epik.py"), "place", "-i", db_path, "-o", str(launched), "--cohort"] + flags +
         [str(tmp_path / "samples.list")])
    for name in new_names:
        assert (launched / name).read_bytes() == (outs["j1"] / name).read_bytes(), name
    # the files are the formatters over the mirror's records for the profile file's cells, and over the device's
    mass, best = cohort_mod.read_profile_tsv(str(_cohort_files(outs["j1"])["profile"]), names, tree.num_nodes)
    totals = cohort_mod.totals_of(mass)
    assert [t > 0 for t in totals] == [name != "blank" for name in names]
    columns, meta, skipped = cohort_mod.read_metadata(str(meta_path), names)
    values = np.ascontiguousarray(np.asarray(meta, dtype=np.float64).T)
    factor_columns, labels, label_names, _ = cohort_mod.read_factors(str(factor_path), names)
    strata = np.ascontiguousarray(labels[:, 1])
    geo_list = geo.copy()
    geo_list[~present[0].astype(bool)] = 0.0
    geo_list[:, ~present[0].astype(bool)] = 0.0
    parent, bl = np.asarray(tree.parent, dtype=np.int64), np.asarray(tree.branch_length, dtype=np.float64)
    first = numpy_first(parent)
    sides = list(columns) + ["geo"]
    assert sides == ["ph", "depth", "geo"] and skipped == 1
    mantel = cohort_mod.mantel_host(mass, first, bl, values, geo_list[None], present, BOTH, 1, 99, 3, strata=strata)
    anosim = cohort_mod.anosim_host(mass, first, bl, labels, 99, 4, strata=strata)
    assert not np.isnan(mantel.records["p"]).any() and mantel.records["used"].tolist() == [11, 11, 12, 12, 11, 11]
    assert not np.isnan(anosim.records["p"][0]) and anosim.records["r"][0] > 0.3                 # the two clades separate
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as device_tree, pl.cohort(len(names)) as cohort:
        cohort.add_cells(mass, best, None)
        same_mantel(cohort.mantel(device_tree, bl, values, geo_list[None], present, BOTH, 1, 99, 3, strata=strata, with_stat=True), mantel)
        same_anosim(cohort.anosim(device_tree, bl, labels, 99, 4, strata=strata, with_stat=True), anosim)
        wide = cohort.mantel(device_tree, bl, values, geo_list[None], present, BOTH, 1, 99, 3, metric="unweighted", strata=strata)
        ranked = cohort.anosim(device_tree, bl, labels, 99, 4, metric="unweighted", strata=strata)
    text = cohort_mod.format_mantel_tsv(names, totals, sides, 2, "both", 1, 99, 3, mantel.records, strata="subject")
    assert (outs["j1"] / new_names[1]).read_text() == text
    assert text.startswith("# epik_amd mantel v1  samples=13 used=12 sides=3 permutations=99 seed=3 method=both partial=depth\tstrata=subject\n"
                           "# unused\tblank\n# side\t0\tcolumn\tph\t11\n# side\t1\tcolumn\tdepth\t12\n# side\t2\tmatrix\tgeo\t11\n")
    back_sides, kinds, records, info = cohort_mod.read_mantel_tsv(str(outs["j1"] / new_names[1]))
    assert back_sides == sides and records.tobytes() == mantel.records.tobytes() and info["strata"] == "subject" and info["partial"] == "depth"
    text = cohort_mod.format_anosim_tsv(names, totals, factor_columns, label_names, labels, 99, 4, anosim.records, strata="subject")
    assert (outs["j1"] / new_names[0]).read_text() == text
    assert cohort_mod.read_anosim_tsv(str(outs["j1"] / new_names[0]))[2].tobytes() == anosim.records.tobytes()
    # over unweighted UniFrac: the field on the first line, and the device's records for that distance
    text = cohort_mod.format_mantel_tsv(names, totals, sides, 2, "both", 1, 99, 3, wide.records, "unweighted", "subject")
    assert (outs["unweighted"] / new_names[1]).read_text() == text and text.split("\n")[0].endswith("\tdistance=unweighted\tstrata=subject")
    text = cohort_mod.format_anosim_tsv(names, totals, factor_columns, label_names, labels, 99, 4, ranked.records, "unweighted", "subject")
    assert (outs["unweighted"] / new_names[0]).read_text() == text and text != (outs["j1"] / new_names[0]).read_text()
    # the flags are refused without what they need, before anything is opened
    for extra, word in ((["--cohort-mantel-seed", "3"], "--cohort-mantel-seed needs"), (["--cohort-anosim-seed", "3"], "needs --cohort-anosim"),
                        (["--cohort-mantel", str(meta_path), "--cohort-mantel-partial", "nobody"], "'nobody'"),
                        (["--cohort-mantel-matrix", "geo"], "NAME=FILE"), (["--cohort-mantel", str(meta_path), "--cohort-mantel-method", "kendall"], "kendall")):
        run = subprocess.run([driver, "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "samples.list"), "-o", str(tmp_path), "--cohort"] + extra,
                             capture_output=True, text=True)
        assert run.returncode == 255 and word in run.stderr and "Loading database" not in run.stdout, (extra, run.stdout, run.stderr)
