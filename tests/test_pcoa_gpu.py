"""Principal coordinates of a cohort's samples on the device: epik_amd_cohort_pcoa / _pcoa_device against the host mirror
and the rule restated in numpy (test_pcoa_cpu.numpy_pcoa), bit for bit, every byte of mu, coord and the info block; the
eigensolver's LDS and global paths and two workgroups; the star fed through d_kr; no side effects; the errors; and
epik-dna --cohort --cohort-pcoa end to end, alone and with --cohort-permdisp and --cohort-permanova on the same design file.
"""
import os
import subprocess

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, dbfile, synth
from test_cohort_cpu import numpy_first, numpy_kr, same_bits
from test_cohort_gpu import ENV, _cohort_files, _run, kr_case
from test_profile_gpu import _write_fasta
from test_pcoa_cpu import (STAR_KR, STAR_MU, STAR_TOLERANCE, assert_pcoa, host_pcoa_kr_raw, numpy_decomposition, numpy_pcoa,
                           pcoa_cells)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
SWITCH = "EPIK_AMD_PCOA_LDS"
PCOA_ENV = ENV + (SWITCH,)
LDS_SIDE = 64                # the largest matrix the eigensolver keeps in LDS (jacobi_device.hpp: kJacobiLdsSide)


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def device_pcoa_raw(pl, cohort, d_kr, k):
    """pcoa_device over d_kr into poisoned buffers on a stream of its own: (mu, coord, info) as the device left them."""
    import torch
    s = cohort.num_samples
    sizes = [s * 8, s * k * 8, 48]
    at = np.concatenate([[0], np.cumsum(sizes)])
    d_out = torch.full((int(at[-1]),), 0xA5, dtype=torch.uint8, device=f"cuda:{pl.device}")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    base = d_out.data_ptr()
    cohort.pcoa_device(d_kr.data_ptr(), k, base + int(at[0]), base + int(at[1]), base + int(at[2]), stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    part = lambda i, dtype: raw[int(at[i]):int(at[i + 1])].view(dtype).copy()
    return part(0, np.float64), part(1, np.float64).reshape(s, k), part(2, capi.PCOA_INFO)[0]


# L: nothing, one, a pair, the first odd size, more than a wave's half, the last two LDS sizes, the first of the global path,
# and more than two workgroups' worth of pairs
USED = (0, 1, 2, 3, 33, LDS_SIDE - 1, LDS_SIDE, LDS_SIDE + 1, 130)


def test_pcoa_equals_the_host_mirror_and_the_restatement_bit_for_bit(placer_cls, monkeypatch):
    import torch
    for var in PCOA_ENV:
        monkeypatch.delenv(var, raising=False)
    num_branches = 7
    parent, bl, first, db = kr_case(num_branches)
    cases = {}
    for num_used in USED:
        mass = pcoa_cells(num_used, num_branches)
        kr, totals = numpy_kr(mass, first, bl), mass.sum(axis=1, dtype=U64)
        once = numpy_decomposition(kr, totals)
        wants = {k: numpy_pcoa(kr, totals, k, once) for k in (5, 64)}
        assert int(wants[64][2]["used"]) == num_used and int(wants[64][2]["converged"]) == 1
        for k, want in wants.items():
            assert_pcoa(host_pcoa_kr_raw(kr, totals, k), want, ("host", num_used, k))
        cases[num_used] = (mass, kr, wants)
    for name, env in (("default", {}), ("global path", {SWITCH: "0"}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
            for num_used, (mass, kr, wants) in cases.items():
                if name == "global path" and num_used > LDS_SIDE + 1:
                    continue                                     # (beyond the LDS sizes the default is the global path)
                what = (name, num_used)
                s = len(mass)
                with pl.cohort(s) as cohort:
                    cohort.add_cells(mass, None, None)
                    assert_pcoa(cohort.pcoa(tree, bl, 5), wants[5], what)
                    d_kr = torch.full((s * s,), np.nan, dtype=torch.float64, device=f"cuda:{pl.device}")
                    cohort.kr_device(tree, bl, d_kr.data_ptr())
                    torch.cuda.synchronize()
                    before = d_kr.cpu().numpy().copy()
                    assert same_bits(before.reshape(s, s), kr), what
                    # into poisoned buffers on a stream of its own: every cell written; the workspace is used again
                    assert_pcoa(device_pcoa_raw(pl, cohort, d_kr, 64), wants[64], what)
                    assert same_bits(d_kr.cpu().numpy(), before), what                          # d_kr is not changed
                    after = cohort.read()
                    assert np.array_equal(after.mass, mass) and not after.best.any(), what      # nor the cells
        for key in env:
            monkeypatch.delenv(key)


def test_the_star_through_d_kr_and_the_errors(placer_cls, monkeypatch):
    import torch
    for var in PCOA_ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(7)
    totals = np.ones(4, U64)
    want = numpy_pcoa(STAR_KR, totals, 4)
    lib = capi.load()
    err = lambda: lib.epik_amd_last_error().decode()
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(4) as cohort:
        mass = np.zeros((4, 7), U64)
        mass[:, 0] = 1                                            # every sample has mass: T_s > 0 is all the rule takes of it
        cohort.add_cells(mass, None, None)
        device = f"cuda:{pl.device}"
        d_kr = torch.full((16,), np.nan, dtype=torch.float64, device=device)
        d_out = torch.full((4 * 8 + 4 * 4 * 8 + 48,), 0xA5, dtype=torch.uint8, device=device)
        base = d_out.data_ptr()
        call = lambda c=cohort._handle, d=d_kr.data_ptr(), k=4, m=base, x=base + 32, i=base + 160: \
            lib.epik_amd_cohort_pcoa_device(c, d, k, m, x, i, None)
        # before any distance: T_s is not on the device yet
        assert call() == capi.ERR_INVALID and "kr_device" in err()
        cohort.kr_device(tree, bl, d_kr.data_ptr())
        torch.cuda.synchronize()
        assert call(c=None) == capi.ERR_INVALID and "null cohort" in err()
        for null in ("d", "m", "x", "i"):
            assert call(**{null: None}) == capi.ERR_INVALID and "null argument" in err(), null
        for bad in (0, 65):
            assert call(k=bad) == capi.ERR_INVALID and "num_components" in err() and "[1, 64]" in err()
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.pcoa(tree, bl, bad)
            assert e.value.code == capi.ERR_INVALID and "num_components" in str(e.value)
        from epik_amd.confidence import Tree
        with Tree(pl.device, *kr_case(999)[:2]) as other_tree, pytest.raises(capi.EpikAmdError) as e:
            cohort.pcoa(other_tree, bl, 4)
        assert e.value.code == capi.ERR_INVALID and "tree" in str(e.value)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0xA5).all()                # the refused calls wrote nothing
        # the forged matrix: the star's distances in the place of the cohort's own
        d_kr.copy_(torch.from_numpy(STAR_KR.reshape(-1)).to(device))
        torch.cuda.synchronize()
        for lds in (None, "0"):
            if lds is not None:
                monkeypatch.setenv(SWITCH, lds)
            got = device_pcoa_raw(pl, cohort, d_kr, 4)
            assert_pcoa(got, want, ("star", lds))
            assert same_bits(d_kr.cpu().numpy().reshape(4, 4), STAR_KR)
        monkeypatch.delenv(SWITCH)
    mu, coord, info = got
    assert (np.abs(mu - STAR_MU) <= STAR_TOLERANCE).all() and abs((0.0 - float(info["neg"])) / float(info["pos"]) - 0.0625) <= STAR_TOLERANCE
    assert cohort_mod.Pcoa(mu, coord, info).kinds() == ["real", "real", "null", "negative"]


def test_epik_dna_cohort_pcoa_end_to_end(placer_cls, tmp_path):
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
        if name == "blank":                               # no placeable read: the sample stays out of the ordination
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
    permanova = ["--cohort-permanova", str(design_path), "--cohort-permanova-permutations", "19"]
    variants = {"plain": ["-j", "1"], "permanova only": ["-j", "1"] + permanova, "j1": ["-j", "1", "--cohort-pcoa"],
                "j4": ["-j", "4", "--cohort-pcoa"], "batch50": ["--batch-size", "50", "--cohort-pcoa"],
                "two handles": ["--devices", "0,0", "-j", "4", "--cohort-pcoa"],
                "with permanova": ["-j", "1", "--cohort-pcoa"] + permanova,
                "three axes": ["-j", "1", "--cohort-pcoa", "--cohort-pcoa-components", "3"],
                "all three": ["-j", "1", "--cohort-pcoa", "--cohort-permdisp", str(design_path), "--cohort-permdisp-permutations", "19",
                              "--cohort-permdisp-seed", "3"] + permanova,
                "all three j4": ["-j", "4", "--batch-size", "50", "--devices", "0,0", "--cohort-pcoa", "--cohort-permdisp", str(design_path),
                                 "--cohort-permdisp-permutations", "19", "--cohort-permdisp-seed", "3"] + permanova}
    new_name, permanova_name = "cohort_pcoa_samples.list.tsv", "cohort_permanova_samples.list.tsv"
    permdisp_name = "cohort_permdisp_samples.list.tsv"
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant.replace(" ", "_"))
        outs[variant].mkdir()
        run = _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + extra)
        older = sorted(p.name for p in _cohort_files(outs[variant]).values())
        new = ([new_name] if "--cohort-pcoa" in extra else []) + ([permanova_name] if "--cohort-permanova" in extra else []) + \
            ([permdisp_name] if "--cohort-permdisp" in extra else [])
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(older + new), variant
        assert ("Cohort principal coordinates: " in run.stdout) == ("--cohort-pcoa" in extra)
        assert ("Cohort PERMDISP: " in run.stdout) == ("--cohort-permdisp" in extra)
        if "--cohort-permdisp" not in extra:
            assert "Warning" not in run.stdout
        else:
            permdisp_stdout = run.stdout
        for what, path in _cohort_files(outs[variant]).items():                # the three older files: unchanged by the flag
            assert path.read_bytes() == _cohort_files(outs["plain"])[what].read_bytes(), (variant, what)
    assert (outs["with permanova"] / permanova_name).read_bytes() == (outs["permanova only"] / permanova_name).read_bytes()
    assert (outs["all three"] / permanova_name).read_bytes() == (outs["permanova only"] / permanova_name).read_bytes()
    assert (outs["all three j4"] / permdisp_name).read_bytes() == (outs["all three"] / permdisp_name).read_bytes()
    tsv = (outs["j1"] / new_name).read_bytes()
    for variant in ("j4", "batch50", "two handles", "with permanova", "all three", "all three j4"):
        assert (outs[variant] / new_name).read_bytes() == tsv, variant
    # the file is the formatter over the mirror's results for the profile file's cells, and over the device's
    mass, best = cohort_mod.read_profile_tsv(str(_cohort_files(outs["j1"])["profile"]), names, tree.num_nodes)
    totals = cohort_mod.totals_of(mass)
    assert [t > 0 for t in totals] == [name != "blank" for name in names]
    parent, bl = np.asarray(tree.parent, dtype=np.int64), np.asarray(tree.branch_length, dtype=np.float64)
    first = numpy_first(parent)
    for variant, k in (("j1", 5), ("three axes", 3)):
        mirror = cohort_mod.pcoa_host(mass, first, bl, k)
        assert_pcoa(mirror, numpy_pcoa(cohort_mod.kr_host(mass, first, bl), totals, k))
        assert int(mirror.info["used"]) == 5 and mirror.components == k and int(mirror.info["converged"]) == 1
        assert (outs[variant] / new_name).read_bytes().decode() == cohort_mod.format_pcoa_tsv(names, totals, mirror), variant
    # the PERMDISP file of the same run: the Python formatter over the mirror's results, byte for byte
    columns, labels, label_names, _ = cohort_mod.read_factors(str(design_path), names, most=32)
    disp = cohort_mod.permdisp_host(mass, first, bl, labels, 19, 3, False)
    assert disp.records["used"][0, 0] == 5 and disp.records["groups"][0, 0] == 2 and not np.isnan(disp.records["p"][0, 0])
    assert (outs["all three"] / permdisp_name).read_bytes().decode() == \
        cohort_mod.format_permdisp_tsv(names, totals, columns, label_names, labels, 19, 3, False, disp.records, disp.group_mean, disp.z)
    assert ("Warning" in permdisp_stdout) == bool(disp.records["clipped"][0, 0]) and "did not converge" not in permdisp_stdout
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as device_tree, pl.cohort(len(names)) as cohort:
        cohort.add_cells(mass, best, None)
        assert_pcoa(cohort.pcoa(device_tree, bl, 5), cohort_mod.pcoa_host(mass, first, bl, 5), "end to end")
    text = tsv.decode()
    assert text.startswith("# epik_amd pcoa v1  samples=6 used=5 components=5 sweeps=") and "# unused\tblank\n" in text
    assert text.count("# eigenvalue\t") == 5 and "\nskin 3\t" in text and "\nit's\t" in text
    back_names, coord, info = cohort_mod.read_pcoa_tsv(str(outs["j1"] / new_name))
    mirror = cohort_mod.pcoa_host(mass, first, bl, 5)
    assert back_names == [n for n in names if n != "blank"] and info["unused"] == ["blank"]
    assert same_bits(coord, mirror.coord[totals > 0][:, :5]) and same_bits(info["mu"], mirror.mu[:5])
