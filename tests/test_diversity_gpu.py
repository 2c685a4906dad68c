"""Alpha diversity and rarefaction curves of a cohort's samples on the device: epik_amd_cohort_alpha / _alpha_device and
epik_amd_cohort_rarefy / _rarefy_device against the host mirror and the rule restated in numpy (test_diversity_cpu), bit for
bit; the block edge, several blocks, two workgroups; one deep curve; the forged cohorts; a placed cohort; the errors; and
epik-dna --cohort --cohort-alpha --cohort-rarefy end to end.
"""
import os
import subprocess

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, dbfile, synth
from test_cohort_cpu import numpy_first, random_cells, same_bits
from test_cohort_gpu import ENV, _cohort_files, _run, kr_case
from test_profile_gpu import _reads, _write_fasta
from test_diversity_cpu import DEPTHS, draw_best, forged_diversity_cohorts, numpy_alpha, numpy_rarefy, same_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def _poisoned(pl, nbytes, call):
    """`call(pointer, stream)` into a poisoned device buffer on a stream of its own: the bytes it left."""
    import torch
    d_out = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    call(d_out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def device_alpha_raw(pl, cohort, tree, bl):
    raw = _poisoned(pl, cohort.num_samples * 40, lambda ptr, stream: cohort.alpha_device(tree, bl, ptr, stream))
    return raw.view(capi.ALPHA).copy()


def device_rarefy_raw(pl, cohort, tree, bl, depth_step, num_depths):
    raw = _poisoned(pl, cohort.num_samples * num_depths * 16,
                    lambda ptr, stream: cohort.rarefy_device(tree, bl, depth_step, num_depths, ptr, stream))
    return raw.view(np.float64).reshape(cohort.num_samples, num_depths, 2).copy()


EDGE_CASES = {}


def tree_of(num_branches):
    """(parent, branch_length, first, db): the trees of the KR tests, and for 255, 256 and 257 branches -- one block of the
    blocked sum short of a branch, full, and a second block of one branch -- a random tree of 128 or 129 leaves, for 256
    with a third child under the root."""
    if num_branches in (7, 999, 5199):
        return kr_case(num_branches)
    if num_branches not in EDGE_CASES:
        tree = synth.make_tree({255: 128, 256: 128, 257: 129}[num_branches], seed=33)
        parent = np.asarray(tree.parent, dtype=np.int64)
        bl = np.array(tree.branch_length, dtype=np.float64)
        if num_branches == 256:      # post-order: the new leaf takes the root's id, the root the one after
            root = len(parent) - 1
            parent = np.concatenate([np.where(parent == root, root + 1, parent)[:root], [root + 1, -1]])
            bl = np.concatenate([bl[:root], [0.375, bl[root]]])
        bl[::5] = 0.0
        assert len(parent) == num_branches
        EDGE_CASES[num_branches] = (parent, bl, numpy_first(parent), synth.make_db(num_branches, kmer_size=4, seed=31, p_present=0.7))
    return EDGE_CASES[num_branches]


CASES = {7: (1, 2, 3, 33, 65), 999: (1, 2, 3, 33, 65), 5199: (3, 34), 255: (3,), 256: (3,), 257: (3,)}


@pytest.mark.parametrize("num_branches", sorted(CASES))
def test_alpha_and_rarefy_equal_the_host_mirror_and_the_restatement_bit_for_bit(placer_cls, monkeypatch, num_branches):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = tree_of(num_branches)
    rng = np.random.default_rng(700 + num_branches)
    cases = {}
    for num_samples in CASES[num_branches]:
        mass = random_cells(rng, num_samples, num_branches, empty=1, bits=42)
        want_alpha = numpy_alpha(mass, first, bl)
        assert same_records(cohort_mod.alpha_host(mass, first, bl), want_alpha)
        curves = {}
        for step, depths in DEPTHS:
            best = draw_best(rng, num_samples, num_branches, step, depths)
            curves[step, depths] = (best, numpy_rarefy(best, first, bl, step, depths))
            assert same_bits(cohort_mod.rarefy_host(best, first, bl, step, depths), curves[step, depths][1])
        cases[num_samples] = (mass, want_alpha, curves)
    for name, env in (("default", {}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for num_samples, (mass, want_alpha, curves) in cases.items():
                for (step, depths), (best, want_curve) in curves.items():
                    what = (name, num_samples, step, depths)
                    with pl.cohort(num_samples) as cohort:
                        cohort.add_cells(mass, best, None)
                        before = cohort.read()
                        others = name == "default" and (step, depths) == (7, 40)
                        if others:
                            older = (cohort.kr(tree, bl), cohort.squash(tree, bl), cohort.epca(tree, 5), cohort.kmeans(tree, bl, 3))
                        assert same_records(cohort.alpha(tree, bl), want_alpha), what
                        assert same_bits(cohort.rarefy(tree, bl, step, depths), want_curve), what
                        # into poisoned buffers on a stream of their own: every cell written; the workspace used again
                        assert same_records(device_alpha_raw(pl, cohort, tree, bl), want_alpha), what
                        got = device_rarefy_raw(pl, cohort, tree, bl, step, depths)
                        assert same_bits(got, want_curve), (what, np.argwhere(got.view(U64) != want_curve.view(U64))[:10])
                        after = cohort.read()
                        assert np.array_equal(after.mass, mass) and np.array_equal(after.best, best)
                        assert np.array_equal(after.mass, before.mass) and np.array_equal(after.best, before.best)
                        if others:
                            kr, merges, epca, kmeans = cohort.kr(tree, bl), cohort.squash(tree, bl), cohort.epca(tree, 5), cohort.kmeans(tree, bl, 3)
                            assert same_records(kr, older[0]) and same_records(merges, older[1]), what
                            assert all(same_records(getattr(epca, f), getattr(older[2], f)) for f in ("mu", "proj", "edge", "info"))
                            assert all(same_records(getattr(kmeans, f), getattr(older[3], f)) for f in ("samples", "clusters", "centroids", "info"))
                            # fewer depths after more: the partials allocated for 40 serve 1
                            assert same_bits(cohort.rarefy(tree, bl, 7, 1), want_curve[:, :1]), what
        for key in env:
            monkeypatch.delenv(key)


def test_one_deep_curve_against_the_host_mirror(placer_cls, monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = tree_of(7)
    rng = np.random.default_rng(71)
    best = np.stack([rng.multinomial(n, rng.dirichlet(np.full(7, 0.7))) for n in ((1 << 20) + 11, 1 << 20, 3 << 20)]).astype(U64)
    want = cohort_mod.rarefy_host(best, first, bl, 4096, 256)
    assert (want >= 0.0).all() and (np.diff(want[:, :, 1], axis=1) >= -1e-9).all()
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(3) as cohort:
        cohort.add_cells(None, best, None)
        got = device_rarefy_raw(pl, cohort, tree, bl, 4096, 256)
    assert same_bits(got, want), np.argwhere(got.view(U64) != want.view(U64))[:10]
    # the curve of n_s = 2^20 ends on all of its reads: the diversity of the sample itself
    assert same_bits(got[1, 255], [cohort_mod.alpha_host(best, first, bl)[f][1] for f in ("pd", "rooted_pd")])


def test_forged_cohorts_on_the_device(placer_cls, monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    cases = forged_diversity_cohorts()
    by_tree = {}
    for name, (_, _, parent, bl) in cases.items():
        by_tree.setdefault((tuple(int(x) for x in parent), tuple(float(x) for x in bl)), []).append(name)
    for (parent, bl), names in by_tree.items():
        parent, bl = np.array(parent), np.array(bl)
        first = numpy_first(parent)
        db = synth.make_db(len(parent), kmer_size=4, seed=31, p_present=0.7)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for name in names:
                mass, best = cases[name][:2]
                with pl.cohort(len(mass)) as cohort:
                    cohort.add_cells(mass, best, None)
                    assert same_records(device_alpha_raw(pl, cohort, tree, bl), numpy_alpha(mass, first, bl)), name
                    for step, depths in DEPTHS:
                        got = device_rarefy_raw(pl, cohort, tree, bl, step, depths)
                        assert same_bits(got, numpy_rarefy(best, first, bl, step, depths)), (name, step, depths)
                        assert same_bits(got, cohort_mod.rarefy_host(best, first, bl, step, depths)), (name, step, depths)


def test_diversity_of_a_placed_cohort_and_the_errors(placer_cls, monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(999)
    reads = _reads(db.kmer_size, np.random.default_rng(9))
    num_samples = 33
    samples = (np.arange(len(reads)) * (num_samples - 1) // len(reads)).astype(np.uint32)
    samples = np.where(samples >= 4, samples + 1, samples).astype(np.uint32)        # sample 4 stays empty
    data, offs = synth.pack_reads(reads)
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(num_samples) as cohort:
        pl.cohort_packed(cohort, data, offs, samples)
        cells = cohort.read()
        alpha = device_alpha_raw(pl, cohort, tree, bl)
        curve = device_rarefy_raw(pl, cohort, tree, bl, 2, 64)
        from epik_amd.confidence import Tree
        for call in (lambda t, l: cohort.alpha(t, l), lambda t, l: cohort.rarefy(t, l, 2, 64)):
            with Tree(pl.device, *kr_case(7)[:2]) as small_tree, pytest.raises(capi.EpikAmdError) as e:
                call(small_tree, bl)
            assert e.value.code == capi.ERR_INVALID and "tree" in str(e.value)
            for bad in (-1.0, np.inf, np.nan):
                length = bl.copy()
                length[17] = bad
                with pytest.raises(capi.EpikAmdError) as e:
                    call(tree, length)
                assert e.value.code == capi.ERR_INVALID and "branch 17" in str(e.value)
        for step, depths, word in ((0, 4, "depth_step"), ((1 << 20) + 1, 1, "depth_step"), (1, 0, "num_depths"), (1, 257, "num_depths"),
                                   (4097, 256, "num_depths * depth_step")):
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.rarefy(tree, bl, step, depths)
            assert e.value.code == capi.ERR_INVALID and word in str(e.value)
        lib = capi.load()
        assert lib.epik_amd_cohort_alpha_device(cohort._handle, tree._handle, bl.ctypes.data, None, None) == capi.ERR_INVALID
        assert b"null argument" in lib.epik_amd_last_error()
        assert lib.epik_amd_cohort_rarefy_device(cohort._handle, tree._handle, bl.ctypes.data, 2, 64, None, None) == capi.ERR_INVALID
        assert b"null argument" in lib.epik_amd_last_error()
        again = (cohort.alpha(tree, bl), cohort.rarefy(tree, bl, 2, 64))
        after = cohort.read()
    assert np.array_equal(after.mass, cells.mass) and np.array_equal(after.best, cells.best)
    assert cells.mass.any(axis=1).sum() >= 30 and not cells.mass[4].any() and not cells.best[4].any()
    want_alpha, want_curve = numpy_alpha(cells.mass, first, bl), numpy_rarefy(cells.best, first, bl, 2, 64)
    assert same_records(alpha, want_alpha) and same_records(again[0], want_alpha)
    assert same_bits(curve, want_curve) and same_bits(again[1], want_curve)
    assert same_records(cohort_mod.alpha_host(cells.mass, first, bl), want_alpha)
    assert same_bits(cohort_mod.rarefy_host(cells.best, first, bl, 2, 64), want_curve)
    assert alpha["pd"][4] == -1.0 and (curve[4] == -1.0).all() and alpha["pd"][0] > 0 and curve[0, 0, 1] > 0


def test_epik_dna_cohort_alpha_and_rarefy_end_to_end(placer_cls, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-dna")
    tree = synth.make_tree(60, seed=13)
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=30, ref_length=500, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    sizes = {"gut_1": 300, "gut_2": 120, "soil": 40, "blank": 45, "skin 3": 210, "it's": 90}
    lines = []
    (tmp_path / "in").mkdir()
    for i, (name, size) in enumerate(sizes.items()):
        if name == "blank":                               # no placeable read: the sample has no diversity and no curve
            reads = ["ACG", "AC", "A"] * 15
        else:
            data, offs = synth.make_clade_reads(refs[(i * 5) % 22:(i * 5) % 22 + 8], size, 150, seed=20 + i)
            reads = [bytes(data[int(offs[j]):int(offs[j + 1])]).decode() for j in range(size)]
        _write_fasta(str(tmp_path / "in" / f"s{i}.fasta"), [(f"s{i}_{j}", s) for j, s in enumerate(reads)])
        lines.append(f"{name}\tin/s{i}.fasta")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    names = list(sizes)
    both = ["--cohort-alpha", "--cohort-rarefy", "64", "--cohort-rarefy-step", "4"]
    variants = {"plain": ["-j", "1"], "j1": ["-j", "1"] + both, "batch50": ["--batch-size", "50", "-j", "4"] + both,
                "batch7": ["--batch-size", "7", "-j", "1"] + both,
                "with the others": ["-j", "4"] + both + ["--cohort-kmeans", "3", "--cohort-squash", "--cohort-epca"],
                "others alone": ["-j", "1", "--cohort-kmeans", "3", "--cohort-squash", "--cohort-epca"],
                "alpha alone": ["-j", "1", "--cohort-alpha"], "default step": ["-j", "1", "--cohort-rarefy", "130"]}
    new_names = ["cohort_alpha_samples.list.tsv", "cohort_rarefy_samples.list.tsv"]
    other_names = ["cohort_epca_edges_samples.list.tsv", "cohort_epca_samples.list.tsv", "cohort_kmeans_centroids_samples.list.tsv",
                   "cohort_kmeans_samples.list.tsv", "cohort_squash_samples.list.nwk", "cohort_squash_samples.list.tsv"]
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant.replace(" ", "_"))
        outs[variant].mkdir()
        run = _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + extra)
        older = sorted(p.name for p in _cohort_files(outs[variant]).values())
        new = ([new_names[0]] if "--cohort-alpha" in extra else []) + ([new_names[1]] if "--cohort-rarefy" in extra else []) + \
            (other_names if "--cohort-squash" in extra else [])
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(older + new), variant
        assert ("Cohort alpha diversity: " in run.stdout) == ("--cohort-alpha" in extra)
        assert ("Cohort rarefaction curves: " in run.stdout) == ("--cohort-rarefy" in extra)
        for what, path in _cohort_files(outs[variant]).items():                # the three older files: unchanged by the flags
            assert path.read_bytes() == _cohort_files(outs["plain"])[what].read_bytes(), (variant, what)
    alpha_bytes, rarefy_bytes = ((outs["j1"] / name).read_bytes() for name in new_names)
    for variant in ("batch50", "batch7", "with the others"):
        assert (outs[variant] / new_names[0]).read_bytes() == alpha_bytes, variant
        assert (outs[variant] / new_names[1]).read_bytes() == rarefy_bytes, variant
    assert (outs["alpha alone"] / new_names[0]).read_bytes() == alpha_bytes
    for name in other_names:                                                   # the other analyses' files: unchanged too
        assert (outs["with the others"] / name).read_bytes() == (outs["others alone"] / name).read_bytes(), name
    # the files computed from the profile file's cells
    mass, best = cohort_mod.read_profile_tsv(str(_cohort_files(outs["j1"])["profile"]), names, tree.num_nodes)
    assert list(mass.sum(axis=1, dtype=U64) > 0) == [True, True, True, False, True, True]
    first = numpy_first(tree.parent)
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    alpha = cohort_mod.alpha_host(mass, first, bl)
    assert same_records(alpha, numpy_alpha(mass, first, bl))
    assert alpha_bytes.decode() == cohort_mod.format_alpha_tsv(names, alpha)
    reads = cohort_mod.reads_of(best)
    assert 0 < int(reads[2]) <= 40 and int(reads[3]) == 0 and int(reads[0]) > 64
    curve = cohort_mod.rarefy_host(best, first, bl, 4, 16)
    assert same_bits(curve, numpy_rarefy(best, first, bl, 4, 16))
    assert rarefy_bytes.decode() == cohort_mod.format_rarefy_tsv(names, reads, 4, curve)
    assert (outs["default step"] / new_names[1]).read_bytes().decode() == \
        cohort_mod.format_rarefy_tsv(names, reads, 3, cohort_mod.rarefy_host(best, first, bl, 3, 43))    # ceil(130 / 64) = 3
    text = rarefy_bytes.decode()
    assert "# unused\tblank\n" in text and "\nskin 3\t4\t" in text and "\ngut_1\t64\t" in text and "\nit's\t4\t" in text and "\nsoil\t64\t" not in text
    rows, info = cohort_mod.read_rarefy_tsv(str(outs["j1"] / new_names[1]))
    assert (info["samples"], info["used"], info["step"], info["depths"], info["unused"]) == (6, 5, 4, 16, ["blank"])
    assert len(rows) == sum(min(16, int(n) // 4) for n in reads)
    back_names, back, info = cohort_mod.read_alpha_tsv(str(outs["j1"] / new_names[0]))
    assert back_names == [n for n in names if n != "blank"] and info["unused"] == ["blank"]
    assert same_records(back, alpha[alpha["pd"] != -1.0])
