"""Edge correlation with per-sample metadata and edge dispersion of a cohort's samples on the device:
epik_amd_cohort_correlation / _correlation_device and epik_amd_cohort_dispersion / _dispersion_device against the host mirror
and the rule restated in numpy (test_correlation_cpu), bit for bit; a tile and a wave stepped over, two workgroups, cells
that are mostly zeros; both sides of every limit of the ranking and the general path forced; no side effects; the errors;
and epik-dna --cohort --cohort-correlation --cohort-dispersion end to end.
"""
import os
import subprocess

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, dbfile, synth
from test_cohort_cpu import numpy_first, random_cells, same_bits
from test_cohort_gpu import ENV, _cohort_files, _run, kr_case
from test_profile_gpu import _reads, _write_fasta  # noqa: F401
from test_correlation_cpu import is_na, numpy_correlation, numpy_dispersion, only_na_or_numbers, same_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
SWITCH = "EPIK_AMD_CORRELATION_LDS"
LDS_SAMPLES = 1024           # the most samples of the LDS path (correlation_place.hip: kLdsSamples)
COUNT_SAMPLES = 128          # ... and the most it ranks by counting (kCountSamples)


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def _poisoned(pl, sizes, call):
    """`call(pointers..., stream)` into poisoned device buffers on a stream of its own: the bytes it left in each."""
    import torch
    bufs = [torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}") for nbytes in sizes]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    call(*[b.data_ptr() for b in bufs], stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    return [b.cpu().numpy() for b in bufs]


def device_correlation_raw(pl, cohort, tree, meta):
    m, n = meta.shape[1], cohort.num_branches
    out, used = _poisoned(pl, (m * n * 32, m * 4), lambda d_out, d_used, stream: cohort.correlation_device(tree, meta, d_out, d_used, stream))
    return out.view(capi.CORRELATION).reshape(m, n).copy(), used.view(np.uint32).copy()


def device_dispersion_raw(pl, cohort, tree):
    out, = _poisoned(pl, (cohort.num_branches * 64,), lambda d_out, stream: cohort.dispersion_device(tree, d_out, stream))
    return out.view(capi.DISPERSION).copy()


def wide_metadata(rng, num_samples):
    """[S][64]: continuous, rounded to integers (ties), a third missing; then columns that share four patterns of missing
    values with those and with each other, a constant column and one without any value."""
    meta = rng.normal(size=(num_samples, 64)) * 3.0 + 7.0
    meta[:, 1] = np.round(rng.normal(size=num_samples) * 1.5)
    patterns = [rng.random(num_samples) < share for share in (1 / 3, 1 / 3, 0.1, 0.6)]
    meta[patterns[0], 2] = np.nan
    for c in range(3, 64):
        if c % 3:
            meta[patterns[c % 4], c] = np.nan
        if c % 5 == 0:
            meta[:, c] = np.round(meta[:, c])
    meta[~np.isnan(meta[:, 40]), 40] = 2.5
    meta[:, 50] = np.nan
    return meta


def sparser(rng, mass):
    """`mass` with another 0.9 share zeroed: ties dominate the ranks."""
    out = mass.copy()
    out[rng.random(out.shape) < 0.9] = 0
    return out


def assert_correlation(got, want, what):
    records, used = got
    assert np.array_equal(used, want[1]), (what, used, want[1])
    for f in capi.CORRELATION.names:
        assert same_bits(records[f], want[0][f]), (what, f, np.argwhere(records[f].view(U64) != want[0][f].view(U64))[:10])
    assert only_na_or_numbers(records), what


CASES = {7: (1, 2, 3, 33, 65), 999: (1, 2, 3, 33, 65), 5199: (3, 34)}


@pytest.mark.parametrize("num_branches", sorted(CASES))
def test_correlation_and_dispersion_equal_the_host_mirror_and_the_restatement_bit_for_bit(placer_cls, monkeypatch, num_branches):
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(num_branches)
    rng = np.random.default_rng(900 + num_branches)
    cases = []
    for num_samples in CASES[num_branches]:
        dense = random_cells(rng, num_samples, num_branches, empty=1, bits=42)
        meta = wide_metadata(rng, num_samples)
        for kind, mass in (("random_cells", dense), ("nine in ten more zeroed", sparser(rng, dense))):
            want = cohort_mod.correlation_host(mass, first, meta)
            # the restatement: all 64 columns on the small tree, the first three on the others (a column's records do not
            # depend on the other columns, in the restatement as in the rule)
            some = 64 if num_branches == 7 else 3
            restated = numpy_correlation(mass, first, meta[:, :some])
            assert same_records(want[0][:some], restated[0]) and np.array_equal(want[1][:some], restated[1]), (num_samples, kind)
            want_disp = cohort_mod.dispersion_host(mass, first)
            assert same_records(want_disp, numpy_dispersion(mass, first)), (num_samples, kind)
            cases.append((num_samples, kind, mass, meta, want, want_disp))
    for name, env in (("default", {}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"}), ("the general path", {SWITCH: "0"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for num_samples, kind, mass, meta, want, want_disp in cases:
                what = (name, num_samples, kind)
                with pl.cohort(num_samples) as cohort:
                    cohort.add_cells(mass, None, None)
                    others = name == "default" and num_samples in (33, 34) and kind == "random_cells"
                    if others:
                        older = (cohort.kr(tree, bl), cohort.squash(tree, bl), cohort.epca(tree, 5), cohort.kmeans(tree, bl, 3),
                                 cohort.alpha(tree, bl), cohort.rarefy(tree, bl, 2, 8))
                    assert_correlation(cohort.correlation(tree, meta), want, what)
                    assert same_records(cohort.dispersion(tree), want_disp), what
                    # into poisoned buffers on a stream of their own: every cell written; the workspace used again; fewer columns
                    for m in (1, 3, 64):
                        got = device_correlation_raw(pl, cohort, tree, np.ascontiguousarray(meta[:, :m]))
                        assert_correlation(got, (want[0][:m], want[1][:m]), what + (m,))
                    assert same_records(device_dispersion_raw(pl, cohort, tree), want_disp), what
                    after = cohort.read()
                    assert np.array_equal(after.mass, mass) and not after.best.any(), what      # the cells are not changed
                    if others:
                        newer = (cohort.kr(tree, bl), cohort.squash(tree, bl), cohort.epca(tree, 5), cohort.kmeans(tree, bl, 3),
                                 cohort.alpha(tree, bl), cohort.rarefy(tree, bl, 2, 8))
                        assert same_records(newer[0], older[0]) and same_records(newer[1], older[1]), what
                        assert all(same_records(getattr(newer[2], f), getattr(older[2], f)) for f in ("mu", "proj", "edge", "info"))
                        assert all(same_records(getattr(newer[3], f), getattr(older[3], f)) for f in ("samples", "clusters", "centroids", "info"))
                        assert same_records(newer[4], older[4]) and same_records(newer[5], older[5]), what
                        assert_correlation(cohort.correlation(tree, meta), want, what + ("again",))
                        assert same_records(cohort.dispersion(tree), want_disp), what
        for key in env:
            monkeypatch.delenv(key)


def test_both_sides_of_every_limit_of_the_ranking_give_the_bits_of_the_general_path(placer_cls, monkeypatch):
    """The ranking keeps a branch's vectors in LDS up to 1 024 samples and in global memory beyond; in LDS it counts up to
    128 samples and sorts beyond.  A cohort with 128 and with 129 used samples, one that sorts 512 values, one on each side
    of 1 024, and the general path forced on all of them."""
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(7)
    rng = np.random.default_rng(77)
    cases = []
    for num_samples in (COUNT_SAMPLES + 1, COUNT_SAMPLES + 2, 300, LDS_SAMPLES, LDS_SAMPLES + 1):       # (one sample is empty)
        mass = sparser(rng, random_cells(rng, num_samples, 7, empty=1, bits=42))
        mass[:, 0] |= U64(1)                                                  # (every other sample keeps some mass)
        mass[1] = 0
        meta = wide_metadata(rng, num_samples)[:, :3].copy()
        want = cohort_mod.correlation_host(mass, first, meta)
        restated = numpy_correlation(mass, first, meta)
        assert same_records(want[0], restated[0]) and np.array_equal(want[1], restated[1]) and want[1][0] == num_samples - 1
        want_disp = cohort_mod.dispersion_host(mass, first)
        assert same_records(want_disp, numpy_dispersion(mass, first))
        assert not is_na(want[0]["mass_spearman"][0, 0]) and not is_na(want[0]["imbalance_spearman"][0]).all()
        cases.append((num_samples, mass, meta, want, want_disp))
    for name, env in (("default", {}), ("the general path", {SWITCH: "0"}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for num_samples, mass, meta, want, want_disp in cases:
                with pl.cohort(num_samples) as cohort:
                    cohort.add_cells(mass, None, None)
                    assert_correlation(device_correlation_raw(pl, cohort, tree, meta), want, (name, num_samples))
                    assert same_records(device_dispersion_raw(pl, cohort, tree), want_disp), (name, num_samples)
        for key in env:
            monkeypatch.delenv(key)


def test_the_errors_of_the_device_entries_and_a_placed_cohort(placer_cls, monkeypatch):
    for var in ENV + (SWITCH,):
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(999)
    reads = _reads(db.kmer_size, np.random.default_rng(9))
    num_samples = 33
    samples = (np.arange(len(reads)) * (num_samples - 1) // len(reads)).astype(np.uint32)
    samples = np.where(samples >= 4, samples + 1, samples).astype(np.uint32)        # sample 4 stays empty
    data, offs = synth.pack_reads(reads)
    meta = wide_metadata(np.random.default_rng(10), num_samples)[:, :3].copy()
    lib = capi.load()
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(num_samples) as cohort:
        pl.cohort_packed(cohort, data, offs, samples)
        cells = cohort.read()
        got = device_correlation_raw(pl, cohort, tree, meta)
        disp = device_dispersion_raw(pl, cohort, tree)
        from epik_amd.confidence import Tree

        def refused(call, *words):
            """ERR_INVALID with the cause, from the entry that writes into device buffers on a stream of its own"""
            with pytest.raises(capi.EpikAmdError) as e:
                _poisoned(pl, (999 * 64 * 32, 64 * 4), call)
            assert e.value.code == capi.ERR_INVALID and all(w in str(e.value) for w in words), str(e.value)

        with Tree(pl.device, *kr_case(7)[:2]) as small_tree:
            refused(lambda d_out, d_used, stream: cohort.correlation_device(small_tree, meta, d_out, d_used, stream), "tree")
            refused(lambda d_out, d_used, stream: cohort.dispersion_device(small_tree, d_out, stream), "tree")
            for call in (lambda: cohort.correlation(small_tree, meta), lambda: cohort.dispersion(small_tree)):
                with pytest.raises(capi.EpikAmdError) as e:
                    call()
                assert e.value.code == capi.ERR_INVALID and "tree" in str(e.value)
        for columns in (0, 65):
            bad = np.zeros((num_samples, columns))
            refused(lambda d_out, d_used, stream: cohort.correlation_device(tree, bad, d_out, d_used, stream), "num_columns", "[1, 64]")
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.correlation(tree, bad)
            assert e.value.code == capi.ERR_INVALID and "num_columns" in str(e.value)
        for value in (np.inf, -np.inf):
            bad = meta.copy()
            bad[17, 2] = value
            refused(lambda d_out, d_used, stream: cohort.correlation_device(tree, bad, d_out, d_used, stream), "sample 17", "column 2", "infinite")
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.correlation(tree, bad)
            assert e.value.code == capi.ERR_INVALID and "infinite" in str(e.value)
        # the poisoned buffers of a refused call, read back: nothing was written
        import torch
        d_out = torch.full((999 * 3 * 32,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}")
        d_used = torch.full((12,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}")
        bad = meta.copy()
        bad[0, 0] = np.inf
        for args in ((cohort._handle, tree._handle, bad.ctypes.data, 3, d_out.data_ptr(), d_used.data_ptr(), None),
                     (cohort._handle, tree._handle, meta.ctypes.data, 65, d_out.data_ptr(), d_used.data_ptr(), None),
                     (cohort._handle, tree._handle, meta.ctypes.data, 0, d_out.data_ptr(), d_used.data_ptr(), None),
                     (cohort._handle, None, meta.ctypes.data, 3, d_out.data_ptr(), d_used.data_ptr(), None)):
            assert lib.epik_amd_cohort_correlation_device(*args) == capi.ERR_INVALID
        for args, word in (((cohort._handle, tree._handle, None, 3, d_out.data_ptr(), d_used.data_ptr(), None), b"null argument"),
                           ((cohort._handle, tree._handle, meta.ctypes.data, 3, None, d_used.data_ptr(), None), b"null argument"),
                           ((cohort._handle, tree._handle, meta.ctypes.data, 3, d_out.data_ptr(), None, None), b"null argument"),
                           ((None, tree._handle, meta.ctypes.data, 3, d_out.data_ptr(), d_used.data_ptr(), None), b"null cohort")):
            assert lib.epik_amd_cohort_correlation_device(*args) == capi.ERR_INVALID and word in lib.epik_amd_last_error()
        assert lib.epik_amd_cohort_dispersion_device(cohort._handle, tree._handle, None, None) == capi.ERR_INVALID
        assert b"null argument" in lib.epik_amd_last_error()
        assert lib.epik_amd_cohort_dispersion_device(None, tree._handle, d_out.data_ptr(), None) == capi.ERR_INVALID
        assert b"null cohort" in lib.epik_amd_last_error()
        assert lib.epik_amd_cohort_correlation(cohort._handle, tree._handle, meta.ctypes.data, 3, None, None) == capi.ERR_INVALID
        assert lib.epik_amd_cohort_dispersion(cohort._handle, tree._handle, None) == capi.ERR_INVALID
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0xA5).all() and (d_used.cpu().numpy() == 0xA5).all()
        again = (cohort.correlation(tree, meta), cohort.dispersion(tree))
        after = cohort.read()
    assert np.array_equal(after.mass, cells.mass) and np.array_equal(after.best, cells.best)
    assert cells.mass.any(axis=1).sum() >= 30 and not cells.mass[4].any()
    want = numpy_correlation(cells.mass, first, meta)
    assert_correlation(got, want, "placed")
    assert_correlation(again[0], want, "placed again")
    host = cohort_mod.correlation_host(cells.mass, first, meta)
    assert same_records(host[0], want[0]) and np.array_equal(host[1], want[1])
    want_disp = numpy_dispersion(cells.mass, first)
    assert same_records(disp, want_disp) and same_records(again[1], want_disp)
    assert same_records(cohort_mod.dispersion_host(cells.mass, first), want_disp)
    assert got[1][0] == cells.mass.any(axis=1).sum() and not is_na(got[0]["mass_pearson"][0]).all()


def test_epik_dna_cohort_correlation_and_dispersion_end_to_end(placer_cls, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-dna")
    tree = synth.make_tree(500, seed=13)
    assert tree.num_nodes == 999
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=30, ref_length=500, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    sizes = {"gut_1": 120, "blank": 45, "skin 3": 90, "it's": 60}
    lines = []
    (tmp_path / "in").mkdir()
    for i, (name, size) in enumerate(sizes.items()):
        if name == "blank":                               # no placeable read: the sample is not used
            reads = ["ACG", "AC", "A"] * 15
        else:
            data, offs = synth.make_clade_reads(refs[(i * 5) % 22:(i * 5) % 22 + 8], size, 150, seed=20 + i)
            reads = [bytes(data[int(offs[j]):int(offs[j + 1])]).decode() for j in range(size)]
        _write_fasta(str(tmp_path / "in" / f"s{i}.fasta"), [(f"s{i}_{j}", s) for j, s in enumerate(reads)])
        lines.append(f"{name}\tin/s{i}.fasta")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    names = list(sizes)
    meta_path = tmp_path / "meta.tsv"
    meta_path.write_text("# the cohort's metadata\nsample\tpH\tdepth m\tcase\n"
                         "it's\t6.5\t\t1\nelsewhere\t1\t2\t3\ngut_1\t7.25\t1e2\t0\nblank\t3\t3\t3\nskin 3\t5.125\t30\t1\n")
    both = ["--cohort-correlation", str(meta_path), "--cohort-dispersion"]
    variants = {"plain": ["-j", "1"], "j1": ["-j", "1"] + both, "j4": ["-j", "4"] + both,
                "batch50": ["--batch-size", "50", "-j", "4"] + both, "batch7": ["--batch-size", "7", "-j", "1"] + both,
                "two handles": ["--devices", "0,0", "-j", "4"] + both,
                "with the others": ["-j", "4"] + both + ["--cohort-kmeans", "2", "--cohort-squash", "--cohort-epca", "--cohort-alpha"],
                "others alone": ["-j", "1", "--cohort-kmeans", "2", "--cohort-squash", "--cohort-epca", "--cohort-alpha"],
                "dispersion alone": ["-j", "1", "--cohort-dispersion"]}
    new_names = ["cohort_correlation_samples.list.tsv", "cohort_dispersion_samples.list.tsv"]
    other_names = ["cohort_alpha_samples.list.tsv", "cohort_epca_edges_samples.list.tsv", "cohort_epca_samples.list.tsv",
                   "cohort_kmeans_centroids_samples.list.tsv", "cohort_kmeans_samples.list.tsv", "cohort_squash_samples.list.nwk",
                   "cohort_squash_samples.list.tsv"]
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant.replace(" ", "_"))
        outs[variant].mkdir()
        run = _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + extra)
        older = sorted(p.name for p in _cohort_files(outs[variant]).values())
        new = ([new_names[0]] if "--cohort-correlation" in extra else []) + ([new_names[1]] if "--cohort-dispersion" in extra else []) + \
            (other_names if "--cohort-squash" in extra else [])
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(older + new), variant
        assert ("Cohort edge correlation: " in run.stdout) == ("--cohort-correlation" in extra)
        assert ("Cohort edge dispersion: " in run.stdout) == ("--cohort-dispersion" in extra)
        assert ("3 columns, 1 lines of samples that are not in the list skipped" in run.stdout) == ("--cohort-correlation" in extra)
        for what, path in _cohort_files(outs[variant]).items():                # the three older files: unchanged by the flags
            assert path.read_bytes() == _cohort_files(outs["plain"])[what].read_bytes(), (variant, what)
    correlation_bytes, dispersion_bytes = ((outs["j1"] / name).read_bytes() for name in new_names)
    for variant in ("j4", "batch50", "batch7", "two handles", "with the others"):
        assert (outs[variant] / new_names[0]).read_bytes() == correlation_bytes, variant
        assert (outs[variant] / new_names[1]).read_bytes() == dispersion_bytes, variant
    assert (outs["dispersion alone"] / new_names[1]).read_bytes() == dispersion_bytes
    for name in other_names:                                                   # the other analyses' files: unchanged too
        assert (outs["with the others"] / name).read_bytes() == (outs["others alone"] / name).read_bytes(), name
    # the files are the formatters over the device's results for the profile file's cells
    mass, best = cohort_mod.read_profile_tsv(str(_cohort_files(outs["j1"])["profile"]), names, tree.num_nodes)
    assert list(mass.sum(axis=1, dtype=U64) > 0) == [True, False, True, True]
    columns, meta, skipped = cohort_mod.read_metadata(str(meta_path), names)
    assert columns == ["pH", "depth m", "case"] and skipped == 1 and np.isnan(meta[3, 1]) and same_bits(meta[0], [7.25, 100.0, 0.0])
    parent = np.asarray(tree.parent, dtype=np.int64)
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as device_tree, pl.cohort(4) as cohort:
        cohort.add_cells(mass, best, None)
        records, used = cohort.correlation(device_tree, meta)
        dispersion = cohort.dispersion(device_tree)
    totals = cohort_mod.totals_of(mass)
    assert correlation_bytes.decode() == cohort_mod.format_correlation_tsv(names, totals, columns, records, used)
    assert dispersion_bytes.decode() == cohort_mod.format_dispersion_tsv(names, totals, dispersion)
    first = numpy_first(parent)
    want = numpy_correlation(mass, first, meta)
    assert same_records(records, want[0]) and list(used) == [3, 2, 3] and same_records(dispersion, numpy_dispersion(mass, first))
    assert is_na(records[1].view(np.float64)).all() and not is_na(records["mass_pearson"][0]).all()
    text = correlation_bytes.decode()
    assert text.startswith("# epik_amd correlation v1  samples=4 used=3 columns=3\n# unused\tblank\n# column\t0\tpH\t3\n# column\t1\tdepth m\t2\n")
    back_columns, back, back_used, info = cohort_mod.read_correlation_tsv(str(outs["j1"] / new_names[0]))
    assert back_columns == columns and same_records(back, records) and info["unused"] == ["blank"]
    back, info = cohort_mod.read_dispersion_tsv(str(outs["j1"] / new_names[1]))
    assert same_records(back, dispersion) and info == {"samples": 4, "used": 3, "unused": ["blank"]}
