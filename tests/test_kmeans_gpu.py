"""Phylogenetic k-means of a cohort's samples on the device: epik_amd_cohort_kmeans / _kmeans_device against the host
mirror and the rule restated in numpy (test_kmeans_cpu.numpy_kmeans), bit for bit, every byte of the sample records, the
cluster records, the centroids and the info block; sample and centroid tiles crossed, two workgroups; the forged cohorts;
one iteration; a placed cohort; the errors; and epik-dna --cohort --cohort-kmeans end to end.
"""
import os
import subprocess

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, dbfile, synth
from test_cohort_cpu import numpy_first, random_cells
from test_cohort_gpu import ENV, _cohort_files, _run, kr_case
from test_profile_gpu import _reads, _write_fasta
from test_kmeans_cpu import NONE, assert_kmeans, forged_kmeans_cohorts, numpy_kmeans, planted_cells

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def device_kmeans_raw(pl, cohort, tree, bl, k, max_iterations=100, stream=None):
    """kmeans_device into poisoned buffers: (samples, clusters, centroids, info) as the device left them."""
    import torch
    s, n = cohort.num_samples, cohort.num_branches
    sizes = [s * 16, k * 24, k * n * 8, 16]
    at = np.concatenate([[0], np.cumsum(sizes)])
    d_out = torch.full((int(at[-1]),), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}")
    torch.cuda.synchronize()
    base = d_out.data_ptr()
    cohort.kmeans_device(tree, bl, k, max_iterations, base + int(at[0]), base + int(at[1]), base + int(at[2]), base + int(at[3]),
                         stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    part = lambda i, dtype: raw[int(at[i]):int(at[i + 1])].view(dtype).copy()
    return (part(0, capi.KMEANS_SAMPLE), part(1, capi.KMEANS_CLUSTER), part(2, np.float64).reshape(k, n), part(3, capi.KMEANS_INFO)[0])


# 17 and 33 used samples cross a sample tile of 16 (S = 34, 65, 66 and 70 have 33, 64, 65 and 69), 65 a wave of the
# one-column pass; K = 33 crosses two centroid tiles of 16
CASES = {7: (1, 2, 3, 4, 33, 34, 65, 66, 70), 999: (1, 2, 3, 4, 33, 34, 65, 66, 70), 5199: (3, 34, 66)}
CLUSTERS = (1, 5, 33, 64)


def same_records(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("cells", ["random", "planted"])
@pytest.mark.parametrize("num_branches", sorted(CASES))
def test_kmeans_equals_the_host_mirror_and_the_restatement_bit_for_bit(placer_cls, monkeypatch, num_branches, cells):
    import torch
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(num_branches)
    rng = np.random.default_rng(500 + num_branches)
    cases = {}
    for num_samples in CASES[num_branches]:
        if cells == "random":
            mass = random_cells(rng, num_samples, num_branches, empty=1, bits=42)
        else:
            mass = planted_cells(num_samples, 3, num_branches)
        wants = {}
        for k in CLUSTERS:
            wants[k] = numpy_kmeans(mass, first, bl, k, 100)[:4]
            assert_kmeans(cohort_mod.kmeans_host(mass, first, bl, k, 100), wants[k], ("host", num_samples, k))
            assert int(wants[k][3]["converged"]) == 1 or not mass.any()
        cases[num_samples] = (mass, wants)
    for name, env in (("default", {}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for num_samples, (mass, wants) in cases.items():
                if name == "two workgroups" and num_samples not in (34, 66, 70):
                    continue
                with pl.cohort(num_samples) as cohort:
                    cohort.add_cells(mass, None, None)
                    before = cohort.read()
                    if name == "default":
                        older = (cohort.kr(tree, bl), cohort.squash(tree, bl), cohort.epca(tree, 5))
                    assert_kmeans(cohort.kmeans(tree, bl, 5), wants[5], (name, num_samples, "synchronous"))
                    # into poisoned buffers on a stream of its own: every cell written; and every call after the first
                    # on this cohort uses the workspace again
                    for k in CLUSTERS:
                        got = device_kmeans_raw(pl, cohort, tree, bl, k, 100, torch.cuda.Stream())
                        assert_kmeans(got, wants[k], (name, num_samples, k))
                    after = cohort.read()
                    assert np.array_equal(after.mass, before.mass) and np.array_equal(after.best, before.best)
                    assert np.array_equal(after.mass, mass)
                    if name == "default":
                        kr, merges, epca = cohort.kr(tree, bl), cohort.squash(tree, bl), cohort.epca(tree, 5)
                        assert same_records(kr, older[0]) and same_records(merges, older[1]), (name, num_samples)
                        assert all(same_records(np.asarray(x), np.asarray(y)) for x, y in
                                   zip((epca.mu, epca.proj, epca.edge, epca.info), (older[2].mu, older[2].proj, older[2].edge, older[2].info)))
        for key in env:
            monkeypatch.delenv(key)


def test_forged_cohorts_and_one_iteration_on_the_device(placer_cls, monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    cases = forged_kmeans_cohorts()
    by_tree = {}
    for name, (mass, parent, bl, k) in cases.items():
        by_tree.setdefault((tuple(int(x) for x in parent), tuple(float(x) for x in bl)), []).append(name)
    assert sorted(len(p) for p, _ in by_tree) == [1, 7, 15]
    for (parent, bl), names in by_tree.items():
        parent, bl = np.array(parent), np.array(bl)
        first = numpy_first(parent)
        db = synth.make_db(len(parent), kmer_size=4, seed=31, p_present=0.7)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for name in names:
                mass, _, _, k = cases[name]
                for max_iterations in (100, 1):
                    host = cohort_mod.kmeans_host(mass, first, bl, k, max_iterations)
                    assert_kmeans(host, numpy_kmeans(mass, first, bl, k, max_iterations), (name, max_iterations))
                    assert int(host.info["converged"]) == (1 if max_iterations == 100 or not mass.any() else 0)
                    with pl.cohort(len(mass)) as cohort:
                        cohort.add_cells(mass, None, None)
                        assert_kmeans(device_kmeans_raw(pl, cohort, tree, bl, k, max_iterations), host, (name, max_iterations))


def test_kmeans_of_a_placed_cohort_and_the_errors(placer_cls, monkeypatch):
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
        got = device_kmeans_raw(pl, cohort, tree, bl, 4)
        one = device_kmeans_raw(pl, cohort, tree, bl, 4, 1)
        from epik_amd.confidence import Tree
        with Tree(pl.device, *kr_case(7)[:2]) as small_tree, pytest.raises(capi.EpikAmdError) as e:
            cohort.kmeans(small_tree, bl, 4)
        assert e.value.code == capi.ERR_INVALID and "tree" in str(e.value)
        for bad in (0, 65):
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.kmeans(tree, bl, bad)
            assert e.value.code == capi.ERR_INVALID and "num_clusters" in str(e.value)
        for bad in (0, 1001):
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.kmeans(tree, bl, 4, bad)
            assert e.value.code == capi.ERR_INVALID and "max_iterations" in str(e.value)
        for bad in (-1.0, np.inf, np.nan):
            length = bl.copy()
            length[17] = bad
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.kmeans(tree, length, 4)
            assert e.value.code == capi.ERR_INVALID and "branch 17" in str(e.value)
        lib = capi.load()
        assert lib.epik_amd_cohort_kmeans_device(cohort._handle, tree._handle, bl.ctypes.data, 4, 100, None, None, None, None,
                                                 None) == capi.ERR_INVALID and b"null argument" in lib.epik_amd_last_error()
        again = cohort.kmeans(tree, bl, 4)
    assert cells.mass.any(axis=1).sum() >= 30 and not cells.mass[4].any()
    want = numpy_kmeans(cells.mass, first, bl, 4, 100)
    assert int(got[3]["used"]) == int(cells.mass.any(axis=1).sum()) and int(got[3]["converged"]) == 1
    assert_kmeans(got, want)
    assert_kmeans(again, want)
    assert_kmeans(cohort_mod.kmeans_host(cells.mass, first, bl, 4), want)
    assert_kmeans(one, numpy_kmeans(cells.mass, first, bl, 4, 1))
    assert tuple(one[3].tolist())[2:] == (1, 0)
    assert got[0]["cluster"][4] == NONE and got[0]["dist"][4] == -1.0 and got[0]["cluster"][0] != NONE


def test_epik_dna_cohort_kmeans_end_to_end(placer_cls, tmp_path):
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
        if name == "blank":                               # no placeable read: the sample stays out of the clusters
            reads = ["ACG", "AC", "A"] * 15
        else:
            data, offs = synth.make_clade_reads(refs[(i * 5) % 22:(i * 5) % 22 + 8], size, 150, seed=20 + i)
            reads = [bytes(data[int(offs[j]):int(offs[j + 1])]).decode() for j in range(size)]
        _write_fasta(str(tmp_path / "in" / f"s{i}.fasta"), [(f"s{i}_{j}", s) for j, s in enumerate(reads)])
        lines.append(f"{name}\tin/s{i}.fasta")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    names = list(sizes)
    variants = {"plain": ["-j", "1"], "j1": ["-j", "1", "--cohort-kmeans", "3"],
                "batch50": ["--batch-size", "50", "--cohort-kmeans", "3", "-j", "4"],
                "with the others": ["-j", "1", "--cohort-kmeans", "3", "--cohort-squash", "--cohort-epca"],
                "one iteration": ["-j", "1", "--cohort-kmeans", "3", "--cohort-kmeans-iterations", "1"]}
    new_names = ["cohort_kmeans_centroids_samples.list.tsv", "cohort_kmeans_samples.list.tsv"]
    other_names = ["cohort_epca_edges_samples.list.tsv", "cohort_epca_samples.list.tsv", "cohort_squash_samples.list.nwk",
                   "cohort_squash_samples.list.tsv"]
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant.replace(" ", "_"))
        outs[variant].mkdir()
        run = _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + extra)
        older = sorted(p.name for p in _cohort_files(outs[variant]).values())
        new = (new_names if "--cohort-kmeans" in extra else []) + (other_names if "--cohort-squash" in extra else [])
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(older + new), variant
        assert ("Cohort k-means: " in run.stdout) == ("--cohort-kmeans" in extra)
        assert ("Warning" in run.stdout and "converged=0" in run.stdout) == (variant == "one iteration"), run.stdout
        for what, path in _cohort_files(outs[variant]).items():                # the three older files: unchanged by the flag
            assert path.read_bytes() == _cohort_files(outs["plain"])[what].read_bytes(), (variant, what)
    centroids, tsv = ((outs["j1"] / name).read_bytes() for name in new_names)
    for variant in ("batch50", "with the others"):
        assert (outs[variant] / new_names[1]).read_bytes() == tsv, variant
        assert (outs[variant] / new_names[0]).read_bytes() == centroids, variant
    # the clusters computed from the profile file's cells
    mass, _ = cohort_mod.read_profile_tsv(str(_cohort_files(outs["j1"])["profile"]), names, tree.num_nodes)
    assert list(mass.sum(axis=1, dtype=U64) > 0) == [True, True, True, False, True, True]
    first = numpy_first(tree.parent)
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    for variant, iterations in (("j1", 100), ("one iteration", 1)):
        kmeans = cohort_mod.kmeans_host(mass, first, bl, 3, iterations)
        assert_kmeans(kmeans, numpy_kmeans(mass, first, bl, 3, iterations))
        assert tuple(kmeans.info.tolist())[:2] == (5, 3) and int(kmeans.info["converged"]) == (1 if iterations == 100 else 0)
        assert (outs[variant] / new_names[1]).read_bytes().decode() == cohort_mod.format_kmeans_tsv(names, kmeans), variant
        assert (outs[variant] / new_names[0]).read_bytes().decode() == cohort_mod.format_kmeans_centroids_tsv(kmeans), variant
    text = tsv.decode()
    assert "# unused\tblank\n" in text and "\nskin 3\t" in text and "\nit's\t" in text
    back_names, cluster, dist, info = cohort_mod.read_kmeans_tsv(str(outs["j1"] / new_names[1]))
    kmeans = cohort_mod.kmeans_host(mass, first, bl, 3)
    used = kmeans.samples["cluster"] != NONE
    assert back_names == [n for n in names if n != "blank"] and info["unused"] == ["blank"]
    assert list(cluster) == list(kmeans.samples["cluster"][used]) and dist.tobytes() == kmeans.samples["dist"][used].tobytes()
    back = cohort_mod.read_kmeans_centroids_tsv(str(outs["j1"] / new_names[0]), 3, tree.num_nodes)
    assert back.tobytes() == kmeans.centroids.tobytes()
