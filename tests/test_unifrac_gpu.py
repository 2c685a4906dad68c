"""The UniFrac distances of a cohort on the device: epik_amd_cohort_unifrac / _unifrac_device against the host mirror and the
rule restated in numpy (test_unifrac_cpu.numpy_unifrac), bit for bit, at every tile and chunk edge and under two workgroups;
one handle whose cells change between the distances; PERMANOVA, PERMDISP and the principal coordinates over a UniFrac matrix
on a cohort whose KR distance never ran; the errors; and epik-dna --cohort --cohort-unifrac --cohort-distance end to end."""
import os
import subprocess

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, dbfile, synth
from test_cohort_cpu import numpy_first, random_cells, same_bits
from test_cohort_gpu import ENV, _cohort_files, _run, kr_case
from test_pcoa_gpu import device_pcoa_raw
from test_permdisp_gpu import device_permdisp_raw
from test_profile_gpu import _write_fasta
from test_unifrac_cpu import METRICS, numpy_unifrac, sparse_cells

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
SAMPLES = (1, 2, 31, 32, 33, 65)   # one lane's pair; a tile short of a sample, full, and one over; three tiles a side


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def device_matrix(pl, cohort, tree, bl, metric):
    """unifrac_device (kr_device for "kr") into a NaN-poisoned buffer on a stream of its own: (the tensor, float64 [S][S])."""
    import torch
    s = cohort.num_samples
    d_out = torch.full((s * s,), float("nan"), dtype=torch.float64, device=f"cuda:{pl.device}")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    if metric == "kr":
        cohort.kr_device(tree, bl, d_out.data_ptr(), stream.cuda_stream)
    else:
        cohort.unifrac_device(tree, bl, metric, d_out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return d_out, d_out.cpu().numpy().reshape(s, s)


UNIFRAC_CASES = {}


def unifrac_case(num_branches):
    """{S: (mass, {metric: the restatement's matrix})} at that tree, computed once and shared; the host mirror agrees."""
    if num_branches not in UNIFRAC_CASES:
        parent, bl, first, _ = kr_case(num_branches)
        rng = np.random.default_rng(100 + num_branches)
        cases = {}
        for s in SAMPLES:
            mass = sparse_cells(rng, s, num_branches, 0.1 if s % 2 else 0.7, empty=1)
            wants = {name: numpy_unifrac(mass, first, bl, name) for name in METRICS}
            for name, want in wants.items():
                assert same_bits(cohort_mod.unifrac_host(mass, first, bl, name), want), (num_branches, s, name)
            cases[s] = (mass, wants)
        UNIFRAC_CASES[num_branches] = cases
    return UNIFRAC_CASES[num_branches]


@pytest.mark.parametrize("blocks", [None, "2"])
@pytest.mark.parametrize("num_branches", [7, 999])
def test_unifrac_equals_the_host_mirror_and_the_restatement_bit_for_bit(placer_cls, monkeypatch, num_branches, blocks):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    if blocks:
        monkeypatch.setenv("EPIK_AMD_MAX_BLOCKS", blocks)
    parent, bl, first, db = kr_case(num_branches)
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
        for s, (mass, wants) in unifrac_case(num_branches).items():
            with pl.cohort(s) as cohort:
                cohort.add_cells(mass, None, None)
                for name, want in wants.items():
                    what = (num_branches, blocks, s, name)
                    got = cohort.unifrac(tree, bl, name)
                    assert same_bits(got, want), (what, np.argwhere(got.view(U64) != want.view(U64))[:10])
                    _, poisoned = device_matrix(pl, cohort, tree, bl, METRICS[name])
                    assert same_bits(poisoned, want), (what, np.argwhere(poisoned.view(U64) != want.view(U64))[:10])
                    if s > 1:
                        assert (got[1] == np.where(np.arange(s) == 1, 0.0, -1.0)).all(), what
                        used = mass.any(axis=1)                     # (sparse cells on seven branches leave other samples empty too)
                        inner = got[np.ix_(used, used)]
                        assert (inner >= 0.0).all() and (inner <= 1.0).all() and (got[~used][:, used] == -1.0).all(), what
                after = cohort.read()
                assert np.array_equal(after.mass, mass) and not after.best.any(), (num_branches, blocks, s)   # the cells are unchanged


def test_one_handle_whose_cells_change(placer_cls, monkeypatch):
    """Stale planes, stale padding samples and the shared half lengths: every matrix of every stage is its mirror's."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    num_branches, s = 999, 33
    parent, bl, first, db = kr_case(num_branches)
    other_bl = bl[::-1].copy()                       # another set of lengths for some calls: d_half is written by every call
    rng = np.random.default_rng(77)
    one = np.zeros((s, num_branches), U64)
    one[s - 1] = rng.integers(1, 1 << 40, size=num_branches, dtype=np.uint64)
    stages = [("dense", sparse_cells(rng, s, num_branches, 0.7)), ("sparse", sparse_cells(rng, s, num_branches, 0.05, empty=2)),
              ("all zero", np.zeros((s, num_branches), U64)), ("one sample with mass", one),
              ("dense again", sparse_cells(rng, s, num_branches, 0.7, empty=0))]
    calls = ["kr", "unweighted", "weighted", "generalized", "kr"]
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(s) as cohort:
        for i, (stage, mass) in enumerate(stages):
            cohort.reset()
            cohort.add_cells(mass, None, None)
            inner = calls[1:4]
            order = ["kr"] + inner[i % 3:] + inner[:i % 3] + ["kr"] if i % 2 == 0 else inner[i % 3:] + ["kr", "kr"] + inner[:i % 3]
            assert sorted(order) == sorted(calls)
            krs = []
            for j, name in enumerate(order):
                lengths = other_bl if (i + j) % 3 == 1 and name != "kr" else bl
                want = cohort_mod.kr_host(mass, first, lengths) if name == "kr" else cohort_mod.unifrac_host(mass, first, lengths, name)
                _, got = device_matrix(pl, cohort, tree, lengths, name)
                assert same_bits(got, want), (stage, order, j, name, np.argwhere(got.view(U64) != want.view(U64))[:10])
                if name == "kr":
                    krs.append(got)
            assert same_bits(krs[0], krs[1]), stage
            assert np.array_equal(cohort.read().mass, mass), stage


def device_permanova_over(pl, cohort, d_matrix, labels, permutations, seed, pairwise):
    """permanova_device over d_matrix into poisoned buffers on a stream of its own: a `Permanova` as the device left it."""
    import torch
    s, m = labels.shape
    slots = 1 + (capi.PERMANOVA_PAIR_SLOTS if pairwise else 0)
    sizes = (m * slots * 56, m * slots * (permutations + 1) * 8, m * 256 * 8)
    bufs = [torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}") for nbytes in sizes]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    cohort.permanova_device(d_matrix.data_ptr(), labels, permutations, seed, pairwise, bufs[0].data_ptr(), bufs[1].data_ptr(),
                            bufs[2].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    out, ssw, group_ss = (b.cpu().numpy() for b in bufs)
    return cohort_mod.Permanova(out.view(capi.PERMANOVA).reshape(m, slots).copy(),
                                ssw.view(np.float64).reshape(m, slots, permutations + 1).copy(),
                                group_ss.view(np.float64).reshape(m, 256).copy())


def test_the_analyses_over_a_unifrac_matrix_where_kr_never_ran(placer_cls, monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    num_branches, s = 999, 33
    parent, bl, first, db = kr_case(num_branches)
    rng = np.random.default_rng(31)
    mass = sparse_cells(rng, s, num_branches, 0.2, empty=4)
    totals = cohort_mod.totals_of(mass)
    labels = np.stack([np.arange(s) % 3, np.arange(s) % 2], axis=1).astype(np.uint32)
    labels[9, 0] = capi.PERMANOVA_MISSING
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
        for name in METRICS:
            matrix = cohort_mod.unifrac_host(mass, first, bl, name)
            want_perm = cohort_mod.permanova_kr_host(matrix, totals, labels, 99, 7, pairwise=True)
            want_disp = cohort_mod.permdisp_kr_host(matrix, totals, labels, 99, 7, pairwise=True)
            want_pcoa = cohort_mod.pcoa_kr_host(matrix, totals, 4)
            with pl.cohort(s) as cohort:                               # a fresh handle: kr_device never runs on it
                cohort.add_cells(mass, None, None)
                d_matrix, got = device_matrix(pl, cohort, tree, bl, name)
                assert same_bits(got, matrix), name
                perm = device_permanova_over(pl, cohort, d_matrix, labels, 99, 7, True)
                assert perm.records.tobytes() == want_perm.records.tobytes() and same_bits(perm.ssw, want_perm.ssw), name
                assert same_bits(perm.group_ss, want_perm.group_ss), name
                disp = device_permdisp_raw(pl, cohort, d_matrix, labels, 99, 7, True)
                assert disp.records.tobytes() == want_disp.records.tobytes() and same_bits(disp.stat, want_disp.stat), name
                assert same_bits(disp.group_mean, want_disp.group_mean) and same_bits(disp.z, want_disp.z), name
                mu, coord, info = device_pcoa_raw(pl, cohort, d_matrix, 4)
                assert same_bits(mu, want_pcoa.mu) and same_bits(coord, want_pcoa.coord) and info.tobytes() == want_pcoa.info.tobytes(), name
                assert same_bits(d_matrix.cpu().numpy().reshape(s, s), matrix), name                 # the matrix is not changed
            with pl.cohort(s) as cohort:                               # and the synchronous entries with metric=
                cohort.add_cells(mass, None, None)
                perm = cohort.permanova(tree, bl, labels, 99, 7, pairwise=True, with_ssw=True, metric=name)
                assert perm.records.tobytes() == want_perm.records.tobytes() and same_bits(perm.ssw, want_perm.ssw), name
                disp = cohort.permdisp(tree, bl, labels, 99, 7, pairwise=True, with_stat=True, metric=name)
                assert disp.records.tobytes() == want_disp.records.tobytes() and same_bits(disp.z, want_disp.z), name
                pcoa = cohort.pcoa(tree, bl, 4, metric=METRICS[name])
                assert same_bits(pcoa.mu, want_pcoa.mu) and same_bits(pcoa.coord, want_pcoa.coord), name
                assert pcoa.info.tobytes() == want_pcoa.info.tobytes(), name
        with pl.cohort(s) as cohort:                                   # the default stays KR
            cohort.add_cells(mass, None, None)
            kr = cohort_mod.kr_host(mass, first, bl)
            pcoa, want = cohort.pcoa(tree, bl, 4), cohort_mod.pcoa_kr_host(kr, totals, 4)
            assert same_bits(pcoa.coord, want.coord) and same_bits(cohort.pcoa(tree, bl, 4, metric="kr").coord, want.coord)


def test_the_errors_of_the_device_entries(placer_cls, monkeypatch):
    import torch
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(7)
    lib = capi.load()
    err = lambda: lib.epik_amd_last_error().decode()
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(3) as cohort:
        cohort.add_cells(random_cells(np.random.default_rng(2), 3, 7), None, None)
        d_out = torch.full((9,), float("nan"), dtype=torch.float64, device=f"cuda:{pl.device}")
        lengths = np.ascontiguousarray(bl, dtype=np.float64)
        call = lambda c=cohort._handle, t=tree._handle, l=lengths.ctypes.data, m=1, d=d_out.data_ptr(): \
            lib.epik_amd_cohort_unifrac_device(c, t, l, m, d, None)
        for metric in (0, 4):
            assert call(m=metric) == capi.ERR_INVALID and f"metric = {metric}" in err()
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.unifrac(tree, bl, metric)
            assert e.value.code == capi.ERR_INVALID and f"metric = {metric}" in str(e.value)
        assert call(c=None) == capi.ERR_INVALID and "null cohort" in err()
        assert call(d=None) == capi.ERR_INVALID and "null argument" in err()
        assert call(l=None) == capi.ERR_INVALID and "null argument" in err()
        from epik_amd.confidence import Tree
        with Tree(pl.device, *kr_case(999)[:2]) as other_tree:
            assert call(t=other_tree._handle) == capi.ERR_INVALID and "tree" in err()
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.unifrac(other_tree, bl, 1)
            assert e.value.code == capi.ERR_INVALID and "tree" in str(e.value)
        for value in (-1.0, np.nan):
            bad = bl.copy()
            bad[5] = value
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.unifrac(tree, bad, "weighted")
            assert e.value.code == capi.ERR_INVALID and "branch 5" in str(e.value)
        with pytest.raises(capi.EpikAmdError) as e:
            cohort.pcoa(tree, bl, 2, metric=4)
        assert e.value.code == capi.ERR_INVALID and "metric = 4" in str(e.value)
        torch.cuda.synchronize()
        assert torch.isnan(d_out).all()                           # the refused calls wrote nothing
        assert call() == capi.OK
        torch.cuda.synchronize()
        assert not torch.isnan(d_out).any()


def test_epik_dna_cohort_unifrac_end_to_end(placer_cls, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-dna")
    tree = synth.make_tree(60, seed=13)
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=30, ref_length=500, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    sizes = {"gut_1": 300, "gut_2": 120, "soil": 40, "blank": 45, "skin 3": 210, "it's": 90}
    lines, design = [], ["sample\tsite"]
    (tmp_path / "in").mkdir()
    for i, (name, size) in enumerate(sizes.items()):
        if name == "blank":                               # no placeable read: -1 in every matrix, out of the analyses
            reads = ["ACG", "AC", "A"] * 15
        else:
            data, offs = synth.make_clade_reads(refs[(i * 5) % 22:(i * 5) % 22 + 8], size, 150, seed=20 + i)
            reads = [bytes(data[int(offs[j]):int(offs[j + 1])]).decode() for j in range(size)]
        _write_fasta(str(tmp_path / "in" / f"s{i}.fasta"), [(f"s{i}_{j}", s) for j, s in enumerate(reads)])
        lines.append(f"{name}\tin/s{i}.fasta")
        design.append(f"{name}\t{'gut' if name.startswith('gut') else 'other'}")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    design_path = tmp_path / "design.tsv"
    design_path.write_text("\n".join(design) + "\n")
    names = list(sizes)
    analyses = ["--cohort-pcoa", "--cohort-permanova", str(design_path), "--cohort-permanova-permutations", "19"]
    new = ["--cohort-unifrac", "all", "--cohort-distance", "unweighted"]
    variants = {"before": ["-j", "1"] + analyses, "kr given": ["-j", "1", "--cohort-distance", "kr"] + analyses,
                "j1": ["-j", "1"] + new + analyses, "j4 batch50": ["-j", "4", "--batch-size", "50"] + new + analyses,
                "distance alone": ["-j", "1", "--cohort-distance", "unweighted"] + analyses,
                "matrices alone": ["-j", "1", "--cohort-unifrac", "generalized,unweighted"]}
    unifrac_names = {name: f"cohort_unifrac_{name}_samples.list.tsv" for name in METRICS}
    pcoa_name, permanova_name = "cohort_pcoa_samples.list.tsv", "cohort_permanova_samples.list.tsv"
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant.replace(" ", "_"))
        outs[variant].mkdir()
        run = _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + extra)
        expected = [p.name for p in _cohort_files(outs[variant]).values()]
        expected += [pcoa_name, permanova_name] if "--cohort-pcoa" in extra else []
        if "--cohort-unifrac" in extra:
            listed = extra[extra.index("--cohort-unifrac") + 1]
            expected += [unifrac_names[n] for n in (METRICS if listed == "all" else listed.split(","))]
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(expected), variant       # and no .part file is left
        assert ("Cohort UniFrac distances (" in run.stdout) == ("--cohort-unifrac" in extra), variant
        for what, path in _cohort_files(outs[variant]).items():                # the three older files: unchanged by the flags
            assert path.read_bytes() == _cohort_files(outs["before"])[what].read_bytes(), (variant, what)
    # without the new flags, and with kr given: the files of before, byte for byte, and no unifrac file
    parent, bl = np.asarray(tree.parent, dtype=np.int64), np.asarray(tree.branch_length, dtype=np.float64)
    first = numpy_first(parent)
    mass, best = cohort_mod.read_profile_tsv(str(_cohort_files(outs["j1"])["profile"]), names, tree.num_nodes)
    totals = cohort_mod.totals_of(mass)
    assert [t > 0 for t in totals] == [name != "blank" for name in names]
    columns, labels, label_names, _ = cohort_mod.read_factors(str(design_path), names)
    kr_pcoa = cohort_mod.pcoa_host(mass, first, bl, 5)
    kr_perm = cohort_mod.permanova_host(mass, first, bl, labels, 19, 1, False)
    for variant in ("before", "kr given"):
        assert (outs[variant] / pcoa_name).read_bytes().decode() == cohort_mod.format_pcoa_tsv(names, totals, kr_pcoa), variant
        assert (outs[variant] / permanova_name).read_bytes().decode() == \
            cohort_mod.format_permanova_tsv(names, totals, columns, label_names, labels, 19, 1, False, kr_perm.records, kr_perm.group_ss), variant
        assert b"distance=" not in (outs[variant] / pcoa_name).read_bytes() + (outs[variant] / permanova_name).read_bytes()
    # the matrices: the bits of the host mirror on the profile file's masses
    for name, file_name in unifrac_names.items():
        back_names, matrix = cohort_mod.read_unifrac_tsv(str(outs["j1"] / file_name))
        want = cohort_mod.unifrac_host(mass, first, bl, name)
        assert back_names == names and same_bits(matrix, want), name
        assert (matrix[3] == np.where(np.arange(6) == 3, 0.0, -1.0)).all()
        assert (outs["j1"] / file_name).read_bytes().decode() == cohort_mod.format_unifrac_tsv(names, want), name
        assert (outs["j4 batch50"] / file_name).read_bytes() == (outs["j1"] / file_name).read_bytes(), name
    for name in ("generalized", "unweighted"):
        assert (outs["matrices alone"] / unifrac_names[name]).read_bytes() == (outs["j1"] / unifrac_names[name]).read_bytes(), name
    # the analyses over the chosen distance: the formatters over the mirrors' results, byte for byte, and named in the first line
    pcoa = cohort_mod.pcoa_host(mass, first, bl, 5, metric="unweighted")
    perm = cohort_mod.permanova_host(mass, first, bl, labels, 19, 1, False, metric="unweighted")
    want_pcoa = cohort_mod.format_pcoa_tsv(names, totals, pcoa, distance="unweighted")
    want_perm = cohort_mod.format_permanova_tsv(names, totals, columns, label_names, labels, 19, 1, False, perm.records, perm.group_ss,
                                                distance="unweighted")
    assert want_pcoa.split("\n")[0].endswith("\tdistance=unweighted") and want_perm.split("\n")[0].endswith("\tdistance=unweighted")
    assert want_pcoa != cohort_mod.format_pcoa_tsv(names, totals, kr_pcoa, distance="unweighted")
    for variant in ("j1", "j4 batch50", "distance alone"):
        assert (outs[variant] / pcoa_name).read_bytes().decode() == want_pcoa, variant
        assert (outs[variant] / permanova_name).read_bytes().decode() == want_perm, variant
    assert cohort_mod.read_pcoa_tsv(str(outs["j1"] / pcoa_name))[2]["distance"] == "unweighted"
    assert cohort_mod.read_permanova_tsv(str(outs["j1"] / permanova_name))[3]["distance"] == "unweighted"
    assert "distance" not in cohort_mod.read_pcoa_tsv(str(outs["before"] / pcoa_name))[2]
