"""The edge test on the device: epik_amd_cohort_edgetest / _edgetest_device against the host mirror (which test_edgetest_cpu
holds to the rule restated in numpy), bit for bit on the records, on every eta of every labelling and on the maxima; a wave, a
workgroup and both sides of every limit of the kernels stepped over, the general path forced, two workgroups; no side effects;
the errors; and epik-dna --cohort --cohort-edge-test end to end on a planted clade.
"""
import os
import subprocess

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, dbfile, synth
from test_cohort_cpu import numpy_first, random_cells
from test_cohort_gpu import ENV, _cohort_files, _run, kr_case
from test_profile_gpu import _write_fasta
from test_permanova_cpu import MISSING, numpy_labellings
from test_edgetest_cpu import same_edgetest, sparser

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
SWITCH = "EPIK_AMD_EDGETEST_LDS"
PAIR_GROUPS = 2              # up to here a lane's accumulators are two registers a family (edgetest_place.hip: the kG = 2 kernel)
REGISTER_GROUPS = 4          # up to here they are registers (kRegisterGroups); beyond, LDS [g][lane] of kLdsLanes = 128 lanes
COUNT_SAMPLES = 128          # the most positions whose midranks the LDS path counts (cohort_device.hpp: kCohortCountSamples)
LDS_POSITIONS = 1024         # the most samples whose vectors stay in LDS (kLdsPositions), and the keys of a tile (kKeyTile)
CHUNK = 1024                 # the labellings made at a time (kChunk): P + 1 of them in all
BLOCK = 256                  # the labellings of a workgroup (kBlock)


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def device_edgetest_raw(pl, cohort, tree, labels, permutations, seed, num_branches):
    """edgetest_device into poisoned buffers on a stream of its own."""
    import torch
    m, row = labels.shape[1], permutations + 1
    sizes = (m * num_branches * 208, m * 4 * num_branches * row * 8, m * 4 * row * 8)
    bufs = [torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}") for nbytes in sizes]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    cohort.edgetest_device(tree, labels, permutations, seed, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    out, stat, most = (b.cpu().numpy() for b in bufs)
    return cohort_mod.Edgetest(out.view(capi.EDGETEST).reshape(m, num_branches).copy(),
                               stat.view(np.float64).reshape(m, 4, num_branches, row).copy(),
                               most.view(np.float64).reshape(m, 4, row).copy())


def group_labels(rng, num_samples, most_groups):
    """labels [S][M] whose largest G is `most_groups` (the kernel is chosen by it): that many groups under scattered ids below
    32, some of one sample; two groups; three unbalanced groups with a fifth missing where they fit; one single group."""
    s = num_samples
    ids = np.array([31, 20, 3, 7, 0, 30, 12, 1, 2, 4, 5, 6, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 21, 22, 23, 24, 25, 26, 27, 28, 29])
    if most_groups <= 7:
        many = ids[np.minimum(rng.geometric(0.35, size=s) - 1, most_groups - 1)]
        many[:most_groups] = ids[:most_groups][:s]
    else:
        many = ids[np.arange(s) % most_groups]
    cols = [many, rng.integers(0, 2, size=s), np.full(s, 17)]
    if most_groups >= 3:
        cols.insert(2, np.where(rng.random(s) < 0.2, MISSING, rng.choice(3, size=s, p=[0.6, 0.3, 0.1])))
    return np.ascontiguousarray(np.array(cols, dtype=np.uint32).T)


# (S, P, the largest G).  S: a wave and a workgroup stepped over, and one size on each side of every limit in S (one sample of
# each cohort is empty, so a column has S - 1 positions at the most: S = 129 and 130 are 128 and 129 positions; the LDS switch
# is taken by S itself); G on both sides of both accumulator switches; P + 1 on both sides of a workgroup's labellings and of
# the chunk
G2, G3, G4, G5 = PAIR_GROUPS, PAIR_GROUPS + 1, REGISTER_GROUPS, REGISTER_GROUPS + 1
CASES = {7: ((3, 1, G2), (4, 63, G2), (33, 64, G3), (65, 65, G4), (64, 9, G5), (COUNT_SAMPLES + 1, BLOCK - 2, G2),
             (COUNT_SAMPLES + 2, BLOCK - 1, G5), (130, BLOCK, 7), (33, CHUNK - 2, G4), (33, CHUNK - 1, G2), (34, CHUNK, G5), (257, 5, 32),
             (LDS_POSITIONS, 5, G2), (LDS_POSITIONS + 1, 5, G4), (LDS_POSITIONS + 2, 3, G5)),
         999: ((3, 65, G2), (4, 1, G2), (33, 65, G5), (65, 64, G4), (130, 63, G2), (257, 9, G3))}
SMALL = 130                   # up to here the general path and two workgroups are run as well


@pytest.mark.parametrize("num_branches", sorted(CASES))
def test_edgetest_equals_the_host_mirror_bit_for_bit(placer_cls, monkeypatch, num_branches):
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(num_branches)
    rng = np.random.default_rng(1600 + num_branches)
    cases = []
    for num_samples, permutations, most_groups in CASES[num_branches]:
        dense = random_cells(rng, num_samples, num_branches, empty=1, bits=42)
        for kind, mass in (("random_cells", dense), ("nine in ten zeroed", sparser(rng, dense))):
            if kind != "random_cells" and num_samples > SMALL:
                continue
            labels = group_labels(rng, num_samples, most_groups)
            seed = int(rng.integers(0, 1 << 63)) * 2 + 1
            want = cohort_mod.edgetest_host(mass, first, labels, permutations, seed)
            assert len(set(labels[:, 0].tolist())) == min(most_groups, num_samples)       # (what chooses the kernel)
            cases.append((num_samples, kind, mass, labels, permutations, seed, want))
    defined = sum(int((~np.isnan(c[-1].records["family"]["p"])).sum()) for c in cases)
    assert defined > 3 * len(cases)
    for name, env in (("default", {}), ("the general path", {SWITCH: "0"}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for num_samples, kind, mass, labels, permutations, seed, want in cases:
                if name != "default" and num_samples > SMALL:
                    continue
                what = (name, num_samples, kind, permutations, int(want.records["groups"].max()))
                with pl.cohort(num_samples) as cohort:
                    cohort.add_cells(mass, None, None)
                    same_edgetest(cohort.edgetest(tree, labels, permutations, seed, with_stat=True, with_max=True), want, what)
                    # into poisoned buffers on a stream of its own: every cell written; the workspace used again
                    same_edgetest(device_edgetest_raw(pl, cohort, tree, labels, permutations, seed, num_branches), want, what + ("raw",))
                    after = cohort.read()
                    assert np.array_equal(after.mass, mass) and not after.best.any(), what      # the cells are not changed
                    fewer = cohort.edgetest(tree, labels[:, :1].copy(), permutations, seed)
                    assert fewer.stat is None and fewer.max is None and fewer.records[0].tobytes() == want.records[0].tobytes(), what
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
    labels = group_labels(rng, num_samples, 5)
    m = labels.shape[1]
    lib = capi.load()
    err = lambda: lib.epik_amd_last_error().decode()
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(num_samples) as cohort:
        cohort.add_cells(mass, None, None)
        device = f"cuda:{pl.device}"
        d_out = torch.full((m * 999 * 208,), 0xA5, dtype=torch.uint8, device=device)
        d_stat = torch.full((m * 4 * 999 * 10 * 8,), 0xA5, dtype=torch.uint8, device=device)
        d_max = torch.full((m * 4 * 10 * 8,), 0xA5, dtype=torch.uint8, device=device)
        call = lambda c=cohort._handle, t=tree._handle, l=labels.ctypes.data, cols=m, p=9, o=d_out.data_ptr(): \
            lib.epik_amd_cohort_edgetest_device(c, t, l, cols, p, 7, o, d_stat.data_ptr(), d_max.data_ptr(), None)
        assert call(c=None) == capi.ERR_INVALID and "null cohort" in err()
        for null in ("t", "l", "o"):
            assert call(**{null: None}) == capi.ERR_INVALID and "null argument" in err(), null
        for bad in (0, 65):
            assert call(cols=bad) == capi.ERR_INVALID and "num_columns" in err() and "[1, 64]" in err()
        for bad in (0, 1_000_000):
            assert call(p=bad) == capi.ERR_INVALID and "num_permutations" in err() and "[1, 999999]" in err()
        for bad in (32, 255):
            wrong = labels.copy()
            wrong[17, 2] = bad
            assert call(l=wrong.ctypes.data) == capi.ERR_INVALID and "sample 17" in err() and "column 2" in err() and "32" in err()
        from epik_amd.confidence import Tree
        with Tree(pl.device, *kr_case(7)[:2]) as small_tree:
            assert call(t=small_tree._handle) == capi.ERR_INVALID and "tree" in err()
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.edgetest(small_tree, labels, 9, 7)
            assert e.value.code == capi.ERR_INVALID and "tree" in str(e.value)
        if capi.device_count() > 1:
            with Tree(1 - pl.device, parent, bl) as far_tree:
                assert call(t=far_tree._handle) == capi.ERR_INVALID and "device" in err()
        for bad in (dict(labels=labels[:, :0].copy()), dict(permutations=0), dict(permutations=1_000_000)):
            kw = dict(labels=labels, permutations=9)
            kw.update(bad)
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.edgetest(tree, kw["labels"], kw["permutations"], 7)
            assert e.value.code == capi.ERR_INVALID
        # the poisoned buffers of the refused calls, read back: nothing was written
        torch.cuda.synchronize()
        for buf in (d_out, d_stat, d_max):
            assert (buf.cpu().numpy() == 0xA5).all()
        # without the optional outputs; then everything, the same records
        assert lib.epik_amd_cohort_edgetest_device(cohort._handle, tree._handle, labels.ctypes.data, m, 9, 7, d_out.data_ptr(), None, None,
                                                   None) == capi.OK
        torch.cuda.synchronize()
        lean = d_out.cpu().numpy().view(capi.EDGETEST).reshape(m, 999).copy()
        assert call() == capi.OK
        torch.cuda.synchronize()
        want = cohort_mod.edgetest_host(mass, first, labels, 9, 7)
        got = cohort_mod.Edgetest(d_out.cpu().numpy().view(capi.EDGETEST).reshape(m, 999).copy(),
                                  d_stat.cpu().numpy().view(np.float64).reshape(m, 4, 999, 10).copy(),
                                  d_max.cpu().numpy().view(np.float64).reshape(m, 4, 10).copy())
        same_edgetest(got, want, "after the refusals")
        assert lean.tobytes() == want.records.tobytes()
        after = cohort.read()
    assert np.array_equal(after.mass, mass)


E2E_PERMUTATIONS, E2E_SEED = 99, 2


def test_epik_dna_cohort_edge_test_end_to_end(placer_cls, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-dna")
    tree = synth.make_tree(500, seed=13)
    assert tree.num_nodes == 999
    db, refs, centres = synth.make_clade_db(tree.num_nodes, n_refs=30, ref_length=500, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    parent = np.asarray(tree.parent, dtype=np.int64)
    first = numpy_first(parent)
    # the planted clade: the inner branch of 60 to 300 branches with the most references at home well inside it; the sick
    # samples' reads come from those references, the healthy samples' from references well outside it
    best = (0, None)
    for b in range(999):
        lo = int(first[b])
        if 60 <= b - lo + 1 <= 300:
            count = int(((centres >= lo + 25) & (centres <= b - 25)).sum())
            if count > best[0]:
                best = (count, b)
    root = best[1]
    inside = refs[(centres >= int(first[root]) + 25) & (centres <= root - 25)]
    outside = refs[(centres < int(first[root]) - 40) | (centres > root + 40)]
    assert len(inside) >= 4 and len(outside) >= 4
    plan = [("gut_1", 0), ("skin 1", 1), ("gut_2", 0), ("blank", None), ("skin 2", 1), ("gut_3", 0), ("it's", 1), ("gut_4", 0),
            ("skin 4", 1), ("gut_5", 0), ("skin 5", 1), ("nobody", 0), ("gut_6", 0), ("skin 6", 1)]
    lines, rows = [], []
    (tmp_path / "in").mkdir()
    for i, (name, group) in enumerate(plan):
        if group is None:                                 # no placeable read: the sample is not used
            reads = ["ACG", "AC", "A"] * 15
        else:
            data, offs = synth.make_clade_reads(inside if group else outside, 60, 150, seed=40 + i)
            reads = [bytes(data[int(offs[j]):int(offs[j + 1])]).decode() for j in range(60)]
        _write_fasta(str(tmp_path / "in" / f"s{i}.fasta"), [(f"s{i}_{j}", s) for j, s in enumerate(reads)])
        lines.append(f"{name}\tin/s{i}.fasta")
        state = "NA" if name == "nobody" else "sick" if group in (1, None) else "healthy"
        rows.append(f"{name}\t{state}\t{'abc'[i % 3]}")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    names = [name for name, _ in plan]
    design = tmp_path / "design.tsv"
    design.write_text("# the design\nsample\tstate\tbatch\nelsewhere\tx\ty\n" + "\n".join(rows) + "\n")
    # that no permutation gives the observed split of the twelve back is a matter of the keys alone: checked here first
    lam = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1])
    mu = numpy_labellings(lam, E2E_SEED, E2E_PERMUTATIONS)[1:]
    assert not ((mu == lam).all(axis=1) | (mu == 1 - lam).all(axis=1)).any()
    flags = ["--cohort-edge-test", str(design), "--cohort-edge-test-permutations", str(E2E_PERMUTATIONS), "--cohort-edge-test-seed",
             str(E2E_SEED)]
    variants = {"plain": ["-j", "1"], "j1": ["-j", "1"] + flags, "j4": ["-j", "4"] + flags,
                "batch50": ["--batch-size", "50", "-j", "4"] + flags, "batch7": ["--batch-size", "7", "-j", "1"] + flags,
                "with the others": ["-j", "4"] + flags + ["--cohort-permanova", str(design), "--cohort-dispersion"],
                "others alone": ["-j", "1", "--cohort-permanova", str(design), "--cohort-dispersion"]}
    new_name = "cohort_edgetest_samples.list.tsv"
    other_names = ["cohort_permanova_samples.list.tsv", "cohort_dispersion_samples.list.tsv"]
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant.replace(" ", "_"))
        outs[variant].mkdir()
        run = _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + extra)
        older = sorted(p.name for p in _cohort_files(outs[variant]).values())
        new = ([new_name] if "--cohort-edge-test" in extra else []) + (other_names if "--cohort-dispersion" in extra else [])
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(older + new), variant
        assert ("Cohort edge test: " in run.stdout) == ("--cohort-edge-test" in extra)
        assert ("Cohort edge-test factors: 2 columns, 1 lines of samples that are not in the list skipped" in run.stdout) == \
            ("--cohort-edge-test" in extra)
        for what, path in _cohort_files(outs[variant]).items():                # the three older files: unchanged by the flags
            assert path.read_bytes() == _cohort_files(outs["plain"])[what].read_bytes(), (variant, what)
    edgetest_bytes = (outs["j1"] / new_name).read_bytes()
    for variant in ("j4", "batch50", "batch7", "with the others"):
        assert (outs[variant] / new_name).read_bytes() == edgetest_bytes, variant
    for name in other_names:                                                   # the other analyses' files: unchanged too
        assert (outs["with the others"] / name).read_bytes() == (outs["others alone"] / name).read_bytes(), name
    # the file is the formatter over the mirror's results for the profile file's cells, and over the device's
    mass, best_cells = cohort_mod.read_profile_tsv(str(_cohort_files(outs["j1"])["profile"]), names, tree.num_nodes)
    totals = cohort_mod.totals_of(mass)
    assert [t > 0 for t in totals] == [name != "blank" for name in names]
    columns, labels, label_names, skipped = cohort_mod.read_factors(str(design), names, most=capi.EDGETEST_MAX_GROUPS)
    assert columns == ["state", "batch"] and skipped == 1 and label_names[0] == ["healthy", "sick"]
    mirror = cohort_mod.edgetest_host(mass, first, labels, E2E_PERMUTATIONS, E2E_SEED)
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as device_tree, pl.cohort(len(names)) as cohort:
        cohort.add_cells(mass, best_cells, None)
        device = cohort.edgetest(device_tree, labels, E2E_PERMUTATIONS, E2E_SEED, with_stat=True, with_max=True)
    same_edgetest(device, mirror, "end to end")
    text = cohort_mod.format_edgetest_tsv(names, totals, columns, label_names, labels, E2E_PERMUTATIONS, E2E_SEED, mirror.records)
    assert edgetest_bytes.decode() == text
    assert text.startswith("# epik_amd edgetest v1  samples=14 used=13 columns=2 permutations=99 seed=2\n# unused\tblank\n"
                           "# column\t0\tstate\t12\t2\n# column\t1\tbatch\t13\t3\n# group\t0\t0\thealthy\t6\n")
    back_columns, rows_back, groups, info = cohort_mod.read_edgetest_tsv(str(outs["j1"] / new_name))
    assert back_columns == columns and info["unused"] == ["blank"] and info["permutations"] == E2E_PERMUTATIONS
    # the planted clade's root: the smallest adjusted p of the imbalance in the column that was planted, and the sick on top
    state_rows = [r for r in rows_back if r["column"] == "state"]
    planted = [r for r in state_rows if r["edge_num"] == root]
    smallest = min(r["imbalance_p_adj"] for r in state_rows if r["imbalance_p_adj"] == r["imbalance_p_adj"])
    print("root", root, planted[0], "smallest", smallest)
    assert len(planted) == 1 and planted[0]["imbalance_p_adj"] == smallest == 1.0 / (E2E_PERMUTATIONS + 1)
    assert planted[0]["imbalance_top"] == "sick"
