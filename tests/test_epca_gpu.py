"""Edge principal components of a cohort's samples on the device: epik_amd_cohort_epca / _epca_device against the host
mirror and the rule restated in numpy (test_epca_cpu.numpy_epca), bit for bit, every byte of mu, proj, edge and the info
block; the eigensolver's LDS and global paths and two workgroups; the forged cohorts; a placed cohort; the errors; and
epik-dna --cohort --cohort-epca end to end.
"""
import os
import subprocess

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, dbfile, synth
from test_cohort_cpu import numpy_first, numpy_kr, random_cells, same_bits
from test_cohort_gpu import ENV, _cohort_files, _run, kr_case
from test_profile_gpu import _reads, _write_fasta
from test_epca_cpu import assert_epca, forged_epca_cohorts, host_epca_raw, numpy_epca
from test_squash_cpu import assert_records, numpy_squash

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
EPCA_ENV = ENV + ("EPIK_AMD_EPCA_LDS",)


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def device_epca_raw(pl, cohort, tree, k, stream=None):
    """epca_device into poisoned buffers: (mu, proj, edge, info) as the device left them."""
    import torch
    s, n = cohort.num_samples, cohort.num_branches
    sizes = [k * 8, s * k * 8, k * n * 8, 32]
    at = np.concatenate([[0], np.cumsum(sizes)])
    d_out = torch.full((int(at[-1]),), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}")
    torch.cuda.synchronize()
    base = d_out.data_ptr()
    cohort.epca_device(tree, k, base + int(at[0]), base + int(at[1]), base + int(at[2]), base + int(at[3]),
                       stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    part = lambda i, dtype: raw[int(at[i]):int(at[i + 1])].view(dtype).copy()
    return part(0, np.float64), part(1, np.float64).reshape(s, k), part(2, np.float64).reshape(k, n), part(3, capi.EPCA_INFO)[0]


def fewer_components(want, k):
    """The first k components of a restatement of more: the components do not depend on how many are asked for."""
    mu, proj, edge, info = want
    info = info.copy()
    info["components"] = min(k, int(info["used"]))
    return mu[:k].copy(), proj[:, :k].copy(), edge[:k].copy(), info


CASES = {7: (1, 2, 3, 4, 33, 34, 65, 66, 70), 999: (1, 2, 3, 4, 33, 34, 65, 66, 70), 5199: (3, 34, 66)}
USED = {1: 1, 2: 1, 3: 2, 4: 3, 33: 32, 34: 33, 65: 64, 66: 65, 70: 69}     # 32 fills a tile, 64 the LDS bound, 65 the global path


@pytest.mark.parametrize("num_branches", sorted(CASES))
def test_epca_equals_the_host_mirror_and_the_restatement_bit_for_bit(placer_cls, monkeypatch, num_branches):
    import torch
    for var in EPCA_ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(num_branches)
    rng = np.random.default_rng(300 + num_branches)
    cases = {}
    for num_samples in CASES[num_branches]:
        mass = random_cells(rng, num_samples, num_branches, empty=1, bits=42)
        want = numpy_epca(mass, first, 64)
        assert int(want[3]["used"]) == USED[num_samples] and int(want[3]["converged"]) == 1 and int(want[3]["sweeps"]) <= 64
        assert_epca(host_epca_raw(mass, first, 64), want, ("host", num_samples))
        assert_epca(host_epca_raw(mass, first, 5), fewer_components(want, 5), ("host", num_samples, 5))
        cases[num_samples] = (mass, want)
    for name, env in (("default", {}), ("global path", {"EPIK_AMD_EPCA_LDS": "0"}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for num_samples, (mass, want) in cases.items():
                if name == "two workgroups" and num_samples not in (34, 70):
                    continue
                what = (name, num_samples)
                with pl.cohort(num_samples) as cohort:
                    cohort.add_cells(mass, None, None)
                    before = cohort.read()
                    assert_epca(cohort.epca(tree, 5), fewer_components(want, 5), what)
                    # into poisoned buffers on a stream of its own: every cell written; and this is the second time on
                    # this cohort: the workspace is used again
                    assert_epca(device_epca_raw(pl, cohort, tree, 64, torch.cuda.Stream()), want, what)
                    after = cohort.read()
                    assert np.array_equal(after.mass, before.mass) and np.array_equal(after.best, before.best)
                    assert np.array_equal(after.mass, mass)
                    if name == "default":
                        assert same_bits(cohort.kr(tree, bl), numpy_kr(mass, first, bl)), what
                        assert_records(cohort.squash(tree, bl), numpy_squash(mass, first, bl), what)
                        assert_epca(cohort.epca(tree, 1), fewer_components(want, 1), what)
        for key in env:
            monkeypatch.delenv(key)


def test_forged_cohorts_on_the_device(placer_cls, monkeypatch):
    for var in EPCA_ENV:
        monkeypatch.delenv(var, raising=False)
    cases = forged_epca_cohorts()
    by_parent = {}
    for name, (mass, parent, k) in cases.items():
        by_parent.setdefault(tuple(int(x) for x in parent), []).append(name)
    assert sorted(len(p) for p in by_parent) == [1, 4, 15]
    for parent, names in by_parent.items():
        parent = np.array(parent)
        first = numpy_first(parent)
        db = synth.make_db(len(parent), kmer_size=4, seed=31, p_present=0.7)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, np.ones(len(parent))) as tree:
            for name in names:
                mass, _, k = cases[name]
                host = host_epca_raw(mass, first, k)
                for lds in (None, "0"):
                    if lds is None:
                        monkeypatch.delenv("EPIK_AMD_EPCA_LDS", raising=False)
                    else:
                        monkeypatch.setenv("EPIK_AMD_EPCA_LDS", lds)
                    with pl.cohort(len(mass)) as cohort:
                        cohort.add_cells(mass, None, None)
                        assert_epca(device_epca_raw(pl, cohort, tree, k), host, (name, lds))
    monkeypatch.delenv("EPIK_AMD_EPCA_LDS", raising=False)


def test_epca_of_a_placed_cohort_and_the_errors(placer_cls, monkeypatch):
    for var in EPCA_ENV:
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
        got = device_epca_raw(pl, cohort, tree, 5)
        from epik_amd.confidence import Tree
        with Tree(pl.device, *kr_case(7)[:2]) as small_tree, pytest.raises(capi.EpikAmdError) as e:
            cohort.epca(small_tree, 5)
        assert e.value.code == capi.ERR_INVALID and "tree" in str(e.value)
        for bad in (0, 65):
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.epca(tree, bad)
            assert e.value.code == capi.ERR_INVALID and "num_components" in str(e.value)
        again = cohort.epca(tree, 5)
    assert cells.mass.any(axis=1).sum() >= 30 and not cells.mass[4].any()
    want = numpy_epca(cells.mass, first, 5)
    assert int(got[3]["used"]) == int(cells.mass.any(axis=1).sum()) and int(got[3]["converged"]) == 1
    assert_epca(got, want)
    assert_epca(again, want)
    assert_epca(host_epca_raw(cells.mass, first, 5), want)
    assert not got[1][4].view(U64).any() and got[1][0].any()


def test_epik_dna_cohort_epca_end_to_end(placer_cls, tmp_path):
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
        if name == "blank":                               # no placeable read: the sample stays out of the components
            reads = ["ACG", "AC", "A"] * 15
        else:
            data, offs = synth.make_clade_reads(refs[(i * 5) % 22:(i * 5) % 22 + 8], size, 150, seed=20 + i)
            reads = [bytes(data[int(offs[j]):int(offs[j + 1])]).decode() for j in range(size)]
        _write_fasta(str(tmp_path / "in" / f"s{i}.fasta"), [(f"s{i}_{j}", s) for j, s in enumerate(reads)])
        lines.append(f"{name}\tin/s{i}.fasta")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    names = list(sizes)
    variants = {"plain": ["-j", "1"], "squash only": ["-j", "1", "--cohort-squash"], "j1": ["-j", "1", "--cohort-epca"],
                "j4": ["-j", "4", "--cohort-epca"], "batch50": ["--batch-size", "50", "--cohort-epca"],
                "batch7000": ["--batch-size", "7000", "--cohort-epca", "-j", "4"],
                "with squash": ["-j", "1", "--cohort-epca", "--cohort-squash"],
                "three components": ["-j", "1", "--cohort-epca", "--cohort-epca-components", "3"]}
    new_names = ["cohort_epca_edges_samples.list.tsv", "cohort_epca_samples.list.tsv"]
    squash_names = ["cohort_squash_samples.list.nwk", "cohort_squash_samples.list.tsv"]
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant.replace(" ", "_"))
        outs[variant].mkdir()
        run = _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + extra)
        older = sorted(p.name for p in _cohort_files(outs[variant]).values())
        new = (new_names if "--cohort-epca" in extra else []) + (squash_names if "--cohort-squash" in extra else [])
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(older + new), variant
        assert ("Cohort principal components" in run.stdout) == ("--cohort-epca" in extra) and "Warning" not in run.stdout
        for what, path in _cohort_files(outs[variant]).items():                # the three older files: unchanged by the flag
            assert path.read_bytes() == _cohort_files(outs["plain"])[what].read_bytes(), (variant, what)
    for name in squash_names:
        assert (outs["with squash"] / name).read_bytes() == (outs["squash only"] / name).read_bytes(), name
    tsv, edges = ((outs["j1"] / name).read_bytes() for name in reversed(new_names))
    for variant in ("j4", "batch50", "batch7000", "with squash"):
        assert (outs[variant] / new_names[1]).read_bytes() == tsv, variant
        assert (outs[variant] / new_names[0]).read_bytes() == edges, variant
    # the components computed from the profile file's cells
    mass, _ = cohort_mod.read_profile_tsv(str(_cohort_files(outs["j1"])["profile"]), names, tree.num_nodes)
    used = mass.sum(axis=1, dtype=U64) > 0
    assert list(used) == [True, True, True, False, True, True]
    first = numpy_first(tree.parent)
    for variant, k in (("j1", 5), ("three components", 3)):
        epca = cohort_mod.epca_host(mass, first, k)
        assert_epca(epca, numpy_epca(mass, first, k))
        assert int(epca.info["used"]) == 5 and int(epca.info["components"]) == k and int(epca.info["converged"]) == 1
        assert (outs[variant] / new_names[1]).read_bytes().decode() == cohort_mod.format_epca_tsv(names, used, epca), variant
        assert (outs[variant] / new_names[0]).read_bytes().decode() == cohort_mod.format_epca_edges_tsv(first, epca), variant
    assert "# unused\tblank\n" in tsv.decode() and "\nskin 3\t" in tsv.decode() and "\nit's\t" in tsv.decode()
    back_names, proj, info = cohort_mod.read_epca_tsv(str(outs["j1"] / new_names[1]))
    epca = cohort_mod.epca_host(mass, first, 5)
    assert back_names == [n for n in names if n != "blank"] and info["unused"] == ["blank"]
    assert same_bits(proj, epca.proj[used][:, :5]) and same_bits(info["mu"], epca.mu)
    edge_num, coeff = cohort_mod.read_epca_edges_tsv(str(outs["j1"] / new_names[0]))
    inner = np.flatnonzero(first < np.arange(len(first)))
    assert list(edge_num) == list(inner) and same_bits(coeff, epca.edge[:, inner].T)
