"""Squash clustering of a cohort's samples on the device: epik_amd_cohort_squash / _squash_device against the host mirror
and the rule restated in numpy (test_squash_cpu.numpy_squash), bit for bit, all 32 bytes of every record; the forged tie
cohorts; two workgroups; a placed cohort; the errors; and epik-dna --cohort --cohort-squash end to end.
"""
import os
import subprocess

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, dbfile, synth
from test_cohort_cpu import numpy_first, numpy_kr, random_cells, same_bits
from test_cohort_gpu import ENV, _cohort_files, _run, kr_case
from test_profile_gpu import _reads, _write_fasta
from test_squash_cpu import assert_records, forged_cohorts, host_all_records, numpy_squash

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def device_all_records(pl, cohort, tree, bl, stream=None):
    """squash_device into a poisoned buffer: all S - 1 records and the count as the device left them."""
    import torch
    records = max(cohort.num_samples - 1, 0)
    d_out = torch.full((records * 32 + 4,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}")
    torch.cuda.synchronize()
    cohort.squash_device(tree, bl, d_out.data_ptr() if records else 0, d_out.data_ptr() + records * 32,
                         stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    return raw[:records * 32].view(capi.SQUASH_MERGE).copy(), int(raw[records * 32:].view(np.uint32)[0])


@pytest.mark.parametrize("num_branches", [7, 999, 5199])
def test_squash_equals_the_host_mirror_and_the_restatement_bit_for_bit(placer_cls, monkeypatch, num_branches):
    import torch
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(num_branches)
    rng = np.random.default_rng(100 + num_branches)
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
        for num_samples in (1, 2, 3, 33, 70):
            mass = random_cells(rng, num_samples, num_branches, empty=1)
            want = numpy_squash(mass, first, bl)
            host, host_count = host_all_records(mass, first, bl)
            assert host_count == want[1] and host.tobytes() == want[0].tobytes(), num_samples
            with pl.cohort(num_samples) as cohort:
                cohort.add_cells(mass, None, None)
                before = cohort.read()
                assert_records(cohort.squash(tree, bl), want, f"S = {num_samples}")
                # into a poisoned buffer on a stream of its own: every record written, the unused ones by rule; and this is
                # the second time on this cohort: the workspace is used again
                records, count = device_all_records(pl, cohort, tree, bl, torch.cuda.Stream())
                assert count == host_count and records.tobytes() == host.tobytes(), (num_samples, records, host)
                after = cohort.read()
                assert np.array_equal(after.mass, before.mass) and np.array_equal(after.best, before.best)
                assert np.array_equal(after.mass, mass)
                assert same_bits(cohort.kr(tree, bl), numpy_kr(mass, first, bl)), num_samples     # the KR matrix is still the KR matrix
                assert_records(cohort.squash(tree, bl), want, f"S = {num_samples}, after kr")


def test_squash_on_the_ladder_equals_the_host_mirror(placer_cls, monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(10_399)
    mass = random_cells(np.random.default_rng(5), 33, 10_399, empty=1)
    host, host_count = host_all_records(mass, first, bl)
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(33) as cohort:
        cohort.add_cells(mass, None, None)
        records, count = device_all_records(pl, cohort, tree, bl)
    assert count == host_count == 31 and records.tobytes() == host.tobytes()


def test_forged_cohorts_on_the_device(placer_cls, monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    cases = forged_cohorts()
    by_size = {}
    for name, (mass, first, bl) in cases.items():
        by_size.setdefault(len(first), []).append(name)
    from test_squash_cpu import BALANCED
    from test_cohort_cpu import tree_case
    parents = {7: BALANCED, 15: tree_case("tree15")[0]}
    assert sorted(by_size) == [7, 15]
    for n, names in by_size.items():
        db = synth.make_db(n, kmer_size=4, seed=31, p_present=0.7)
        with placer_cls.from_synth(db) as pl:
            for name in names:
                mass, first, bl = cases[name]
                assert np.array_equal(numpy_first(parents[n]), first)
                host, host_count = host_all_records(mass, first, bl)
                with pl.tree(parents[n], bl) as tree, pl.cohort(len(mass)) as cohort:
                    cohort.add_cells(mass, None, None)
                    records, count = device_all_records(pl, cohort, tree, bl)
                assert count == host_count and records.tobytes() == host.tobytes(), (name, records, host)


def test_squash_of_a_placed_cohort_under_two_workgroups_and_the_errors(placer_cls, monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(999)
    reads = _reads(db.kmer_size, np.random.default_rng(9))
    num_samples = 33
    samples = (np.arange(len(reads)) * (num_samples - 1) // len(reads)).astype(np.uint32)
    samples = np.where(samples >= 4, samples + 1, samples).astype(np.uint32)        # sample 4 stays empty
    data, offs = synth.pack_reads(reads)
    forged = random_cells(np.random.default_rng(12), 70, 999, empty=8)
    results = {}
    for name, env in (("default", {}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            with pl.cohort(num_samples) as cohort:
                pl.cohort_packed(cohort, data, offs, samples)
                cells = cohort.read()
                results[name] = [cells, device_all_records(pl, cohort, tree, bl)]
                # errors: another tree, a bad length
                from epik_amd.confidence import Tree
                with Tree(pl.device, *kr_case(7)[:2]) as small_tree, pytest.raises(capi.EpikAmdError) as e:
                    cohort.squash(small_tree, bl)
                assert e.value.code == capi.ERR_INVALID and "tree" in str(e.value)
                bad = bl.copy()
                bad[17] = -1.0
                with pytest.raises(capi.EpikAmdError) as e:
                    cohort.squash(tree, bad)
                assert e.value.code == capi.ERR_INVALID and "branch 17" in str(e.value)
            with pl.cohort(70) as cohort:
                cohort.add_cells(forged, None, None)
                results[name].append(device_all_records(pl, cohort, tree, bl))
        for key in env:
            monkeypatch.delenv(key)
    cells, (records, count), (records70, count70) = results["default"]
    assert cells.mass.any(axis=1).sum() >= 30 and not cells.mass[4].any()
    want, want_count = numpy_squash(cells.mass, first, bl)
    host, host_count = host_all_records(cells.mass, first, bl)
    assert count == want_count == host_count == int(cells.mass.any(axis=1).sum()) - 1
    assert records.tobytes() == want.tobytes() == host.tobytes()
    assert 4 not in set(records["a"][:count]) | set(records["b"][:count])
    host70, host_count70 = host_all_records(forged, first, bl)
    assert count70 == host_count70 == 68 and records70.tobytes() == host70.tobytes()
    two = results["two workgroups"]
    assert np.array_equal(two[0].mass, cells.mass)
    assert two[1][1] == count and two[1][0].tobytes() == records.tobytes()
    assert two[2][1] == count70 and two[2][0].tobytes() == records70.tobytes()


def test_epik_dna_cohort_squash_end_to_end(placer_cls, tmp_path):
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
        if name == "blank":                               # no placeable read: the sample stays out of the clustering
            reads = ["ACG", "AC", "A"] * 15
        else:
            data, offs = synth.make_clade_reads(refs[(i * 5) % 22:(i * 5) % 22 + 8], size, 150, seed=20 + i)
            reads = [bytes(data[int(offs[j]):int(offs[j + 1])]).decode() for j in range(size)]
        _write_fasta(str(tmp_path / "in" / f"s{i}.fasta"), [(f"s{i}_{j}", s) for j, s in enumerate(reads)])
        lines.append(f"{name}\tin/s{i}.fasta")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    names = list(sizes)
    variants = {"plain": ["-j", "1"], "j1": ["-j", "1", "--cohort-squash"], "j4": ["-j", "4", "--cohort-squash"],
                "batch50": ["--batch-size", "50", "--cohort-squash"], "batch7000": ["--batch-size", "7000", "--cohort-squash", "-j", "4"]}
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant)
        outs[variant].mkdir()
        run = _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + extra)
        older = sorted(p.name for p in _cohort_files(outs[variant]).values())
        new = [] if variant == "plain" else ["cohort_squash_samples.list.nwk", "cohort_squash_samples.list.tsv"]
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(older + new), variant
        assert ("Cohort cluster tree" in run.stdout) == (variant != "plain")
        for what, path in _cohort_files(outs[variant]).items():                # the three older files: unchanged by the flag
            assert path.read_bytes() == _cohort_files(outs["plain"])[what].read_bytes(), (variant, what)
    tsv = (outs["j1"] / "cohort_squash_samples.list.tsv").read_bytes()
    nwk = (outs["j1"] / "cohort_squash_samples.list.nwk").read_bytes()
    for variant in ("j4", "batch50", "batch7000"):
        assert (outs[variant] / "cohort_squash_samples.list.tsv").read_bytes() == tsv, variant
        assert (outs[variant] / "cohort_squash_samples.list.nwk").read_bytes() == nwk, variant
    # the records computed from the profile file's cells
    mass, _ = cohort_mod.read_profile_tsv(str(_cohort_files(outs["j1"])["profile"]), names, tree.num_nodes)
    live = mass.sum(axis=1, dtype=U64) > 0
    assert list(live) == [True, True, True, False, True, True]
    first = numpy_first(tree.parent)
    want, count = numpy_squash(mass, first, tree.branch_length)
    records = cohort_mod.squash_host(mass, first, tree.branch_length)
    assert count == 4
    assert_records(records, (want, count))
    assert tsv.decode() == cohort_mod.format_squash_tsv(names, live, records)
    assert nwk.decode() == cohort_mod.format_squash_newick(names, live, records)
    assert "# unclustered\tblank\n" in tsv.decode() and "'skin 3':" in nwk.decode() and "'it''s':" in nwk.decode()
    back, info = cohort_mod.read_squash_tsv(str(outs["j1"] / "cohort_squash_samples.list.tsv"))
    assert back.tobytes() == records.tobytes() and info["clustered"] == 5 and info["unclustered"] == ["blank"]
