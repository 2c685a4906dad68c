"""epik-dna and epik.py --cohort --cohort-edge-model end to end on the device, 13 samples: cohort_edgemodel_<list>.tsv is the same
bytes at -j 1 and -j 4 and two batch sizes and from the launcher, is the formatter over the host mirror's and over the device's
records for the profile file's cells, reads back, names the aliased column and the incomplete sample; with --cohort-strata only
what the rule says changes; and every other cohort file of the run is unchanged by the flags.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import cohort as cohort_mod, dbfile, synth
from test_cohort_cpu import numpy_first
from test_cohort_gpu import _cohort_files, _run
from test_edgemodel_cpu import same_edgemodel
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


def test_epik_dna_and_the_launcher_cohort_edge_model_end_to_end(placer_cls, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-dna")
    tree = synth.make_tree(500, seed=13)
    assert tree.num_nodes == 999
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=30, ref_length=500, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    # two states, each drawn from its own eight references, a blank sample and one without an age: 13 samples
    plan = [("gut_1", 0), ("skin 1", 1), ("gut_2", 0), ("blank", None), ("skin 2", 1), ("gut_3", 0), ("it's", 1), ("gut_4", 0),
            ("skin 4", 1), ("gut_5", 0), ("skin 5", 1), ("nobody", 0), ("gut_6", 0)]
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
        rows.append(f"{name}\t{'sick' if group in (1, None) else 'healthy'}\t{age}\t{'abc'[i % 3]}\t{age}\t{'pq'[i % 2]}")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    names = [name for name, _ in plan]
    design_path = tmp_path / "design.tsv"
    design_path.write_text("# the design\nsample\tstate\tage\tsite\tage2\tsubject\nelsewhere\tx\t1\ty\t1\tp\n" + "\n".join(rows) + "\n")
    flags = ["--cohort-edge-model", str(design_path), "--cohort-edge-model-terms", TERMS, "--cohort-edge-model-permutations",
             str(PERMUTATIONS), "--cohort-edge-model-seed", str(SEED)]
    within = ["--cohort-strata", str(design_path), "--cohort-strata-column", "subject"]
    model_flags = ["--cohort-model", str(design_path), "--cohort-model-terms", TERMS]      # (the same file serves --cohort-model)
    variants = {"plain": ["-j", "1"], "j1": ["-j", "1"] + flags, "j4": ["-j", "4"] + flags,
                "batch50": ["--batch-size", "50", "-j", "4"] + flags, "batch7": ["--batch-size", "7", "-j", "1"] + flags,
                "with the others": ["-j", "4"] + flags + model_flags + ["--cohort-squash", "--cohort-alpha"],
                "others alone": ["-j", "1"] + model_flags + ["--cohort-squash", "--cohort-alpha"],
                "strata": ["-j", "4"] + flags + within}
    new_name = "cohort_edgemodel_samples.list.tsv"
    other_names = ["cohort_alpha_samples.list.tsv", "cohort_model_samples.list.tsv", "cohort_squash_samples.list.nwk",
                   "cohort_squash_samples.list.tsv"]
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant.replace(" ", "_"))
        outs[variant].mkdir()
        run = _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + extra)
        older = sorted(p.name for p in _cohort_files(outs[variant]).values())
        new = ([new_name] if "--cohort-edge-model" in extra else []) + (other_names if "--cohort-squash" in extra else [])
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(older + new), variant
        given = "--cohort-edge-model" in extra
        assert ("Cohort edge model: " in run.stdout) == given
        assert ("Cohort edge model design: 4 terms, 1 lines of samples that are not in the list skipped" in run.stdout) == given
        assert ("Warning: 1 columns of the edge model's design are explained by the columns before them" in run.stdout) == given
        for what, path in _cohort_files(outs[variant]).items():                # the three older files: unchanged by the flags
            assert path.read_bytes() == _cohort_files(outs["plain"])[what].read_bytes(), (variant, what)
    file_bytes = (outs["j1"] / new_name).read_bytes()
    for variant in ("j4", "batch50", "batch7", "with the others"):
        assert (outs[variant] / new_name).read_bytes() == file_bytes, variant
    for name in other_names:                                                   # the other analyses' files: unchanged too
        assert (outs["with the others"] / name).read_bytes() == (outs["others alone"] / name).read_bytes(), name
    # the launcher passes the flags on: the same bytes
    launched = tmp_path / "launcher"
    launched.mkdir()
    _run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "-i", db_path, "-o", str(launched), "--cohort"] + flags +
         [str(tmp_path / "samples.list")])
    assert (launched / new_name).read_bytes() == file_bytes
    # the file is the formatter over the mirror's results for the profile file's cells, and over the device's
    mass, best = cohort_mod.read_profile_tsv(str(_cohort_files(outs["j1"])["profile"]), names, tree.num_nodes)
    totals = cohort_mod.totals_of(mass)
    assert [t > 0 for t in totals] == [name != "blank" for name in names]
    terms, kind, labels, values, label_names, skipped = cohort_mod.read_design(str(design_path), TERMS, names)
    assert terms == ["age", "site", "age2", "state"] and skipped == 1 and label_names[3] == ["healthy", "sick"]
    strata, strata_name = cohort_mod.read_strata(str(design_path), names, "subject")
    parent = np.asarray(tree.parent, dtype=np.int64)
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    first = numpy_first(parent)
    mirror = cohort_mod.edgemodel_host(mass, first, kind, labels, values, PERMUTATIONS, SEED)
    stratified = cohort_mod.edgemodel_host(mass, first, kind, labels, values, PERMUTATIONS, SEED, strata=strata)
    assert tuple(mirror.info)[:5] == (11, 4, 5, 4, 6) and list(mirror.info["df"][:4]) == [1, 2, 0, 1]
    state = mirror.records["family"][3, :, 0]
    assert (state["p"][~np.isnan(state["p"])] <= 0.05).any()                   # the two clades separate on some branch, after age and site
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as device_tree, pl.cohort(len(names)) as cohort:
        cohort.add_cells(mass, best, None)
        device = cohort.edgemodel(device_tree, kind, labels, values, PERMUTATIONS, SEED, with_stat=True, with_max=True)
        device_stratified = cohort.edgemodel(device_tree, kind, labels, values, PERMUTATIONS, SEED, strata=strata)
    same_edgemodel(device, mirror, "end to end")
    same_edgemodel(device_stratified, stratified, "end to end, strata")
    text = cohort_mod.format_edgemodel_tsv(names, totals, terms, kind, label_names, labels, values, PERMUTATIONS, SEED, mirror)
    assert file_bytes.decode() == text
    assert text == cohort_mod.format_edgemodel_tsv(names, totals, terms, kind, label_names, labels, values, PERMUTATIONS, SEED, device)
    assert text.startswith("# epik_amd edgemodel v1  samples=13 used=11 terms=4 columns=5 rank=4 permutations=99 seed=2\n# unused\tblank\n"
                           "# incomplete\tnobody\tage\n# term\t0\tn\tage\t1\t1\n# term\t1\tf\tsite\t2\t2\n# term\t2\tn\tage2\t1\t0\n")
    assert "\n# aliased\t2\t-\n" in text
    back_terms, records, info = cohort_mod.read_edgemodel_tsv(str(outs["j1"] / new_name), tree.num_nodes)
    assert [t[0] for t in back_terms] == terms
    for f in cohort_mod.EDGEMODEL_FIELDS:
        assert np.ascontiguousarray(records["family"][f]).tobytes() == np.ascontiguousarray(mirror.records["family"][f]).tobytes(), f
    assert info["unused"] == ["blank"] and info["incomplete"] == [("nobody", "age")] and info["aliased"] == [(2, "-")]
    # with --cohort-strata: the field on the first line, the observed half of every line the same, the p-values the strata rule's
    text_within = cohort_mod.format_edgemodel_tsv(names, totals, terms, kind, label_names, labels, values, PERMUTATIONS, SEED,
                                                  device_stratified, strata=strata_name)
    assert (outs["strata"] / new_name).read_bytes().decode() == text_within
    plain_lines, strata_lines = text.split("\n"), text_within.split("\n")
    assert strata_lines[0] == plain_lines[0] + "\tstrata=subject" and len(strata_lines) == len(plain_lines) and text_within != text
    observed = [0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13]                         # all but mass_p, mass_p_adj, imbalance_p, imbalance_p_adj
    for a, b in zip(plain_lines[1:-1], strata_lines[1:-1]):
        if a.startswith("#") or a.startswith("term\t"):
            assert a == b
        else:
            assert [a.split("\t")[k] for k in observed] == [b.split("\t")[k] for k in observed]
