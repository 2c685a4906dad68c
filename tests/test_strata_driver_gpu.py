"""epik-dna --cohort with the four permutation tests and --cohort-strata end to end on the device: the four files are the same
bytes at -j 1 and -j 16 and two batch sizes, are the formatters over the host mirror's stratified records with the strata=NAME
field, and read back; every other cohort file of the run is unchanged by the flag; the nested column is warned about; and a
run without the flag writes the four files as before: the formatters, which without a name are what they were, over the
unstratified mirror's records.
"""
import os
import subprocess

import numpy as np
import pytest

from epik_amd import cohort as cohort_mod, dbfile, synth
from test_cohort_cpu import numpy_first
from test_cohort_gpu import _cohort_files, _run
from test_profile_gpu import _write_fasta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERMUTATIONS, SEED = 99, 2
TERMS = "f:batch,f:state"


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def test_epik_dna_cohort_strata_end_to_end(placer_cls, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-dna")
    tree = synth.make_tree(500, seed=13)
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=30, ref_length=500, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    # six subjects sampled twice, healthy then sick, each state drawn from its own eight references; a blank sample.  The
    # subject lives in the design file itself; the batch is constant inside every subject.
    plan = [(f"subject {k} {'ab'[state]}", k, state) for k in range(6) for state in (0, 1)]
    plan.insert(3, ("blank", 6, None))
    lines, rows = [], []
    (tmp_path / "in").mkdir()
    for i, (name, subject, state) in enumerate(plan):
        if state is None:                                  # no placeable read: the sample is not used
            reads = ["ACG", "AC", "A"] * 15
        else:
            data, offs = synth.make_clade_reads(refs[state * 14:state * 14 + 8], 60, 150, seed=40 + i)
            reads = [bytes(data[int(offs[j]):int(offs[j + 1])]).decode() for j in range(60)]
        _write_fasta(str(tmp_path / "in" / f"s{i}.fasta"), [(f"s{i}_{j}", s) for j, s in enumerate(reads)])
        lines.append(f"{name}\tin/s{i}.fasta")
        rows.append(f"{name}\t{'sick' if state else 'healthy'}\tbatch {subject % 2}\tperson {subject}")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    names = [name for name, _, _ in plan]
    design_path = tmp_path / "design.tsv"
    design_path.write_text("# the design\nsample\tstate\tbatch\tsubject\nelsewhere\tx\ty\tz\n" + "\n".join(rows) + "\n")
    tests = []
    for flag in ("permanova", "permdisp", "edge-test", "model"):
        tests += [f"--cohort-{flag}", str(design_path), f"--cohort-{flag}-permutations", str(PERMUTATIONS), f"--cohort-{flag}-seed", str(SEED)]
    tests += ["--cohort-model-terms", TERMS, "--cohort-permanova-pairwise"]
    strata = ["--cohort-strata", str(design_path), "--cohort-strata-column", "subject"]
    others = ["--cohort-squash", "--cohort-alpha"]
    variants = {"plain": ["-j", "1"], "free": ["-j", "1"] + tests + others, "j1": ["-j", "1"] + tests + strata + others,
                "j16": ["-j", "16"] + tests + strata, "batch50": ["--batch-size", "50", "-j", "16"] + tests + strata,
                "batch7": ["--batch-size", "7", "-j", "1"] + tests + strata}
    new_names = {what: f"cohort_{what}_samples.list.tsv" for what in ("permanova", "permdisp", "edgetest", "model")}
    other_names = ["cohort_alpha_samples.list.tsv", "cohort_squash_samples.list.nwk", "cohort_squash_samples.list.tsv"]
    outs, runs = {}, {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant)
        outs[variant].mkdir()
        runs[variant] = run = _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + extra)
        older = sorted(p.name for p in _cohort_files(outs[variant]).values())
        new = (sorted(new_names.values()) if "--cohort-model" in extra else []) + (other_names if "--cohort-squash" in extra else [])
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(older + new), variant
        assert ("Cohort strata: column subject, 7 strata of 13 samples" in run.stdout) == ("--cohort-strata" in extra), variant
        for flag in ("--cohort-permanova", "--cohort-permdisp", "--cohort-edge-test"):     # the nested columns are named, with strata only
            for column in ("batch", "subject"):
                warned = f"Warning: {flag}: the column {column} is constant inside every stratum of subject" in run.stdout
                assert warned == ("--cohort-strata" in extra), (variant, flag, column, run.stdout)
            assert f"{flag}: the column state is constant" not in run.stdout
        assert ("Warning: --cohort-model: the term batch is constant inside every stratum of subject" in run.stdout) == ("--cohort-strata" in extra)
        for what, path in _cohort_files(outs[variant]).items():                # the three older files: unchanged by the flags
            assert path.read_bytes() == _cohort_files(outs["plain"])[what].read_bytes(), (variant, what)
    for what, name in new_names.items():
        for variant in ("j16", "batch50", "batch7"):
            assert (outs[variant] / name).read_bytes() == (outs["j1"] / name).read_bytes(), (variant, what)
        assert (outs["free"] / name).read_bytes() != (outs["j1"] / name).read_bytes(), what
    for name in other_names:                                                   # the other analyses' files: unchanged by the strata
        assert (outs["j1"] / name).read_bytes() == (outs["free"] / name).read_bytes(), name
    # the files are the formatters over the mirror's records for the profile file's cells
    mass, best = cohort_mod.read_profile_tsv(str(_cohort_files(outs["j1"])["profile"]), names, tree.num_nodes)
    totals = cohort_mod.totals_of(mass)
    assert [t > 0 for t in totals] == [name != "blank" for name in names]
    subjects, strata_name = cohort_mod.read_strata(str(design_path), names, "subject")
    assert strata_name == "subject" and len(set(subjects.tolist())) == 7
    parent = np.asarray(tree.parent, dtype=np.int64)
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    first = numpy_first(parent)
    columns, labels, label_names, skipped = cohort_mod.read_factors(str(design_path), names, True)
    columns32, labels32, label_names32, _ = cohort_mod.read_factors(str(design_path), names, most=32)
    terms, kind, mlabels, values, mlabel_names, _ = cohort_mod.read_design(str(design_path), TERMS, names)
    assert columns == columns32 == ["state", "batch", "subject"] and skipped == 1 and terms == ["batch", "state"]

    def expected(within, field):
        more = {} if field is None else {"strata": field}
        nova = cohort_mod.permanova_host(mass, first, bl, labels, PERMUTATIONS, SEED, True, strata=within)
        disp = cohort_mod.permdisp_host(mass, first, bl, labels32, PERMUTATIONS, SEED, False, strata=within)
        edge = cohort_mod.edgetest_host(mass, first, labels32, PERMUTATIONS, SEED, with_stat=False, with_max=False, strata=within)
        model = cohort_mod.model_host(mass, first, bl, kind, mlabels, values, PERMUTATIONS, SEED, strata=within)
        return {"permanova": cohort_mod.format_permanova_tsv(names, totals, columns, label_names, labels, PERMUTATIONS, SEED, True,
                                                             nova.records, nova.group_ss, **more),
                "permdisp": cohort_mod.format_permdisp_tsv(names, totals, columns32, label_names32, labels32, PERMUTATIONS, SEED, False,
                                                           disp.records, disp.group_mean, disp.z, **more),
                "edgetest": cohort_mod.format_edgetest_tsv(names, totals, columns32, label_names32, labels32, PERMUTATIONS, SEED,
                                                           edge.records, **more),
                "model": cohort_mod.format_model_tsv(names, totals, terms, kind, mlabel_names, mlabels, values, PERMUTATIONS, SEED, model,
                                                     **more)}, (nova, model)

    within, (nova, model) = expected(subjects, "subject")
    free, (free_nova, free_model) = expected(None, None)          # without the flag: the calls and the formatters as they were
    readers = {"permanova": cohort_mod.read_permanova_tsv, "permdisp": cohort_mod.read_permdisp_tsv, "edgetest": cohort_mod.read_edgetest_tsv,
               "model": cohort_mod.read_model_tsv}
    for what, name in new_names.items():
        assert (outs["j1"] / name).read_bytes().decode() == within[what], what
        assert (outs["free"] / name).read_bytes().decode() == free[what], what
        assert within[what].split("\n")[0] == free[what].split("\n")[0] + "\tstrata=subject", what
        assert readers[what](str(outs["j1"] / name))[-1]["strata"] == "subject" and "strata" not in readers[what](str(outs["free"] / name))[-1]
    # what the strata are for: the state differs within every subject, and only the stratified test may say so at its smallest p
    state, free_state = nova.records[0, 0], free_nova.records[0, 0]
    assert state["used"] == 12 and state["groups"] == 2 and state["ss_within"] == free_state["ss_within"]
    assert nova.records["p"][1, 0] == 1.0 and nova.records["p"][2, 0] == 1.0 and free_nova.records["p"][1, 0] < 1.0       # batch, subject
    assert model.records["ss"][0] == free_model.records["ss"][0] and not np.isnan(model.records["p"][0])                  # the term batch
    # and the device's own records for the same cells
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as device_tree, pl.cohort(len(names)) as cohort:
        cohort.add_cells(mass, best, None)
        device = cohort.permanova(device_tree, bl, labels, PERMUTATIONS, SEED, True, strata=subjects)
    assert device.records.tobytes() == nova.records.tobytes()
