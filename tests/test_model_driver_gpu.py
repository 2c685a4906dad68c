"""epik-dna --cohort --cohort-model end to end on the device: cohort_model_<list>.tsv is the same bytes at -j 1 and -j 16 and two
batch sizes, is the formatter over the host mirror's and over the device's records for the profile file's cells, reads back,
names the aliased column and the incomplete sample; over a UniFrac distance with --cohort-distance; and every other cohort
file of the run is unchanged by the flags.
"""
import os
import subprocess

import numpy as np
import pytest

from epik_amd import cohort as cohort_mod, dbfile, synth
from test_cohort_cpu import numpy_first
from test_cohort_gpu import _cohort_files, _run
from test_model_cpu import same_model
from test_profile_gpu import _write_fasta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERMUTATIONS, SEED = 99, 2
TERMS = "n:age,f:site,n:age2,f:state"


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def test_epik_dna_cohort_model_end_to_end(placer_cls, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-dna")
    tree = synth.make_tree(500, seed=13)
    assert tree.num_nodes == 999
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=30, ref_length=500, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    # two states of six samples, each drawn from its own eight references, a blank sample and one without an age
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
        age = "NA" if name == "nobody" else f"{20 + (7 * i) % 31}.5"
        rows.append(f"{name}\t{'sick' if group in (1, None) else 'healthy'}\t{age}\t{'abc'[i % 3]}\t{age}")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    names = [name for name, _ in plan]
    design_path = tmp_path / "design.tsv"
    design_path.write_text("# the design\nsample\tstate\tage\tsite\tage2\nelsewhere\tx\t1\ty\t1\n" + "\n".join(rows) + "\n")
    flags = ["--cohort-model", str(design_path), "--cohort-model-terms", TERMS, "--cohort-model-permutations", str(PERMUTATIONS),
             "--cohort-model-seed", str(SEED)]
    variants = {"plain": ["-j", "1"], "j1": ["-j", "1"] + flags, "j16": ["-j", "16"] + flags,
                "batch50": ["--batch-size", "50", "-j", "16"] + flags, "batch7": ["--batch-size", "7", "-j", "1"] + flags,
                "with the others": ["-j", "4"] + flags + ["--cohort-squash", "--cohort-alpha", "--cohort-pcoa"],
                "others alone": ["-j", "1", "--cohort-squash", "--cohort-alpha", "--cohort-pcoa"],
                "unweighted": ["-j", "4"] + flags + ["--cohort-distance", "unweighted"]}
    new_name = "cohort_model_samples.list.tsv"
    other_names = ["cohort_alpha_samples.list.tsv", "cohort_pcoa_samples.list.tsv", "cohort_squash_samples.list.nwk",
                   "cohort_squash_samples.list.tsv"]
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant.replace(" ", "_"))
        outs[variant].mkdir()
        run = _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + extra)
        older = sorted(p.name for p in _cohort_files(outs[variant]).values())
        new = ([new_name] if "--cohort-model" in extra else []) + (other_names if "--cohort-squash" in extra else [])
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(older + new), variant
        assert ("Cohort model: " in run.stdout) == ("--cohort-model" in extra)
        assert ("Cohort model design: 4 terms, 1 lines of samples that are not in the list skipped" in run.stdout) == ("--cohort-model" in extra)
        assert ("Warning: 1 columns of the design are explained by the columns before them" in run.stdout) == ("--cohort-model" in extra)
        for what, path in _cohort_files(outs[variant]).items():                # the three older files: unchanged by the flags
            assert path.read_bytes() == _cohort_files(outs["plain"])[what].read_bytes(), (variant, what)
    model_bytes = (outs["j1"] / new_name).read_bytes()
    for variant in ("j16", "batch50", "batch7", "with the others"):
        assert (outs[variant] / new_name).read_bytes() == model_bytes, variant
    for name in other_names:                                                   # the other analyses' files: unchanged too
        assert (outs["with the others"] / name).read_bytes() == (outs["others alone"] / name).read_bytes(), name
    # the file is the formatter over the mirror's results for the profile file's cells, and over the device's
    mass, best = cohort_mod.read_profile_tsv(str(_cohort_files(outs["j1"])["profile"]), names, tree.num_nodes)
    totals = cohort_mod.totals_of(mass)
    assert [t > 0 for t in totals] == [name != "blank" for name in names]
    terms, kind, labels, values, label_names, skipped = cohort_mod.read_design(str(design_path), TERMS, names)
    assert terms == ["age", "site", "age2", "state"] and skipped == 1 and label_names[3] == ["healthy", "sick"]
    parent = np.asarray(tree.parent, dtype=np.int64)
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    first = numpy_first(parent)
    mirror = cohort_mod.model_host(mass, first, bl, kind, labels, values, PERMUTATIONS, SEED)
    assert tuple(mirror.info)[:5] == (12, 4, 5, 4, 7) and list(mirror.records["df"]) == [1, 2, 0, 1, 4]
    state = mirror.records[3]
    assert not np.isnan(state["p"]) and state["r2"] > 0.3                      # the two clades separate, after age and site too
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as device_tree, pl.cohort(len(names)) as cohort:
        cohort.add_cells(mass, best, None)
        device = cohort.model(device_tree, bl, kind, labels, values, PERMUTATIONS, SEED, with_stat=True)
        device_unweighted = cohort.model(device_tree, bl, kind, labels, values, PERMUTATIONS, SEED, metric="unweighted")
    same_model(device, mirror, "end to end")
    text = cohort_mod.format_model_tsv(names, totals, terms, kind, label_names, labels, values, PERMUTATIONS, SEED, mirror)
    assert model_bytes.decode() == text
    assert text.startswith("# epik_amd model v1  samples=14 used=12 terms=4 columns=5 rank=4 permutations=99 seed=2\n# unused\tblank\n"
                           "# incomplete\tnobody\tage\n# term\t0\tn\tage\t1\t1\n# term\t1\tf\tsite\t2\t2\n# term\t2\tn\tage2\t1\t0\n")
    assert "\n# aliased\t2\t-\n" in text
    back_terms, records, info = cohort_mod.read_model_tsv(str(outs["j1"] / new_name))
    assert [t[0] for t in back_terms] == terms and records.tobytes() == mirror.records.tobytes()
    assert info["unused"] == ["blank"] and info["incomplete"] == [("nobody", "age")] and info["aliased"] == [(2, "-")]
    # over unweighted UniFrac: the field on the first line, and the device's records for that distance
    text = cohort_mod.format_model_tsv(names, totals, terms, kind, label_names, labels, values, PERMUTATIONS, SEED, device_unweighted,
                                       distance="unweighted")
    assert (outs["unweighted"] / new_name).read_bytes().decode() == text and text.split("\n")[0].endswith("seed=2\tdistance=unweighted")
    assert text.encode() != model_bytes
