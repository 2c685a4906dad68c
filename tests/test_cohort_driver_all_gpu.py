"""epik-dna --cohort with every analysis of a cohort asked for at once, end to end on the device, 13 samples: the files written are
exactly the table's, the same bytes at -j 1 and at -j 4 --batch-size 7, each the same bytes as from a run that asks for its
analysis with a few others only, and the "Cohort ...:" lines of the report stand in their fixed order.
"""
import os
import subprocess

import pytest

from epik_amd import dbfile, synth
from test_cohort_gpu import _run
from test_profile_gpu import _write_fasta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the summary calls every file, in the summary's order, and the file's name less its cohort_ and _samples.list
SUMMARY = [("Cohort samples", "samples.tsv"), ("Cohort profile", "profile.tsv"), ("Cohort distances", "kr.tsv"),
           ("Cohort UniFrac distances (unweighted)", "unifrac_unweighted.tsv"), ("Cohort UniFrac distances (weighted)", "unifrac_weighted.tsv"),
           ("Cohort UniFrac distances (generalized)", "unifrac_generalized.tsv"), ("Cohort clustering", "squash.tsv"),
           ("Cohort cluster tree", "squash.nwk"), ("Cohort principal components", "epca.tsv"), ("Cohort component edges", "epca_edges.tsv"),
           ("Cohort k-means", "kmeans.tsv"), ("Cohort k-means centroids", "kmeans_centroids.tsv"), ("Cohort alpha diversity", "alpha.tsv"),
           ("Cohort rarefaction curves", "rarefy.tsv"), ("Cohort edge correlation", "correlation.tsv"),
           ("Cohort edge dispersion", "dispersion.tsv"), ("Cohort PERMANOVA", "permanova.tsv"), ("Cohort edge test", "edgetest.tsv"),
           ("Cohort PERMDISP", "permdisp.tsv"), ("Cohort Mantel", "mantel.tsv"), ("Cohort ANOSIM", "anosim.tsv"), ("Cohort model", "model.tsv"),
           ("Cohort edge model", "edgemodel.tsv"), ("Cohort principal coordinates", "pcoa.tsv")]


def file_name(what):
    stem, extension = what.rsplit(".", 1)
    return f"cohort_{stem}_samples.list.{extension}"


def test_every_analysis_at_once_writes_what_each_writes_alone(gpu_available, tmp_path):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-dna")
    tree = synth.make_tree(500, seed=13)
    assert tree.num_nodes == 999
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=30, ref_length=500, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    # two states, each drawn from its own eight references, a blank sample and one without an age: 13 samples of 60 reads
    plan = [("gut_1", 0), ("skin 1", 1), ("gut_2", 0), ("blank", None), ("skin 2", 1), ("gut_3", 0), ("it's", 1), ("gut_4", 0),
            ("skin 4", 1), ("gut_5", 0), ("skin 5", 1), ("nobody", 0), ("gut_6", 0)]
    names = [name for name, _ in plan]
    lines, design, factors, metadata = [], [], [], []
    (tmp_path / "in").mkdir()
    for i, (name, group) in enumerate(plan):
        if group is None:                                 # no placeable read: the sample is not used
            reads = ["ACG", "AC", "A"] * 20
        else:
            data, offs = synth.make_clade_reads(refs[group * 14:group * 14 + 8], 60, 150, seed=40 + i)
            reads = [bytes(data[int(offs[j]):int(offs[j + 1])]).decode() for j in range(60)]
        _write_fasta(str(tmp_path / "in" / f"s{i}.fasta"), [(f"s{i}_{j}", s) for j, s in enumerate(reads)])
        lines.append(f"{name}\tin/s{i}.fasta")
        state, site, subject = "sick" if group in (1, None) else "healthy", "abc"[i % 3], "pq"[i % 2]
        age = "NA" if name == "nobody" else f"{20 + (7 * i) % 31}.5"
        design.append(f"{name}\t{state}\t{age}\t{site}\t{subject}")
        factors.append(f"{name}\t{state}\t{site}")
        metadata.append(f"{name}\t{age}\t{(5 * i) % 13}")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    (tmp_path / "design.tsv").write_text("sample\tstate\tage\tsite\tsubject\nelsewhere\tx\t1\ty\tp\n" + "\n".join(design) + "\n")
    (tmp_path / "factors.tsv").write_text("sample\tstate\tsite\n" + "\n".join(factors) + "\n")
    (tmp_path / "metadata.tsv").write_text("sample\tage\tdepth\n" + "\n".join(metadata) + "\n")
    (tmp_path / "geo.tsv").write_text("name\t" + "\t".join(names) + "\n" + "".join(
        a + "\t" + "\t".join(str(abs(i - j) % 5) for j in range(len(names))) + "\n" for i, a in enumerate(names)))
    at = lambda name: str(tmp_path / name)  # noqa: E731
    permutations = lambda flag: [f"--cohort-{flag}-permutations", "99", f"--cohort-{flag}-seed", "3"]  # noqa: E731
    distance, strata = ["--cohort-distance", "weighted"], ["--cohort-strata", at("design.tsv"), "--cohort-strata-column", "subject"]
    groups = {
        "no test": (["--cohort-squash", "--cohort-epca", "--cohort-kmeans", "3", "--cohort-alpha", "--cohort-rarefy", "40", "--cohort-correlation",
                     at("metadata.tsv"), "--cohort-dispersion", "--cohort-unifrac", "all"], [],
                    ["unifrac_unweighted.tsv", "unifrac_weighted.tsv", "unifrac_generalized.tsv", "squash.tsv", "squash.nwk", "epca.tsv",
                     "epca_edges.tsv", "kmeans.tsv", "kmeans_centroids.tsv", "alpha.tsv", "rarefy.tsv", "correlation.tsv", "dispersion.tsv"]),
        "groups": (["--cohort-permanova", at("factors.tsv"), "--cohort-permanova-pairwise", "--cohort-permdisp", at("factors.tsv"),
                    "--cohort-permdisp-pairwise", "--cohort-pcoa"] + permutations("permanova") + permutations("permdisp"), distance + strata,
                   ["permanova.tsv", "permdisp.tsv", "pcoa.tsv"]),
        "distances": (["--cohort-mantel", at("metadata.tsv"), "--cohort-mantel-matrix", "geo=" + at("geo.tsv"), "--cohort-mantel-method", "both",
                       "--cohort-anosim", at("factors.tsv"), "--cohort-model", at("design.tsv"), "--cohort-model-terms", "n:age,f:site,f:state"] +
                      permutations("mantel") + permutations("anosim") + permutations("model"), distance + strata,
                      ["mantel.tsv", "anosim.tsv", "model.tsv"]),
        "branches": (["--cohort-edge-test", at("factors.tsv"), "--cohort-edge-model", at("design.tsv"), "--cohort-edge-model-terms",
                      "n:age,f:site,f:state"] + permutations("edge-test") + permutations("edge-model"), strata,
                     ["edgetest.tsv", "edgemodel.tsv"]),
    }
    every_flag = [flag for flags, _, _ in groups.values() for flag in flags] + distance + strata
    runs = {"j1": ["-j", "1"] + every_flag, "j4": ["-j", "4", "--batch-size", "7"] + every_flag}
    runs.update({group: ["-j", "4"] + flags + extra for group, (flags, extra, _) in groups.items()})
    outs, stdout = {}, {}
    for run, flags in runs.items():
        outs[run] = tmp_path / ("out_" + run.replace(" ", "_"))
        outs[run].mkdir()
        stdout[run] = _run([driver, "-d", db_path, "-q", at("samples.list"), "-o", str(outs[run]), "--cohort"] + flags).stdout
    # the files written are exactly the table's, and the two runs' are the same bytes
    every_file = sorted(file_name(what) for _, what in SUMMARY)
    assert len(every_file) == 24
    for run in ("j1", "j4"):
        assert sorted(p.name for p in outs[run].iterdir()) == every_file, run
    for name in every_file:
        assert (outs["j1"] / name).read_bytes() == (outs["j4"] / name).read_bytes(), name
    # each file is what the run with its analysis and a few others wrote: no analysis changes another's
    alone = {what: group for group, (_, _, files) in groups.items() for what in files}
    assert sorted(alone) == sorted(what for _, what in SUMMARY[3:])
    for group, (_, _, files) in groups.items():
        assert sorted(p.name for p in outs[group].iterdir()) == sorted(file_name(what) for what in files + [w for _, w in SUMMARY[:3]]), group
        for what in files + [w for _, w in SUMMARY[:3]]:
            assert (outs[group] / file_name(what)).read_bytes() == (outs["j1"] / file_name(what)).read_bytes(), (group, what)
    first_line = lambda what: (outs["j1"] / file_name(what)).read_text().split("\n")[0]  # noqa: E731
    assert first_line("permanova.tsv").endswith("\tdistance=weighted\tstrata=subject") and first_line("pcoa.tsv").endswith("\tdistance=weighted")
    assert first_line("edgemodel.tsv").endswith("seed=3\tstrata=subject")
    # the report names every file, in the fixed order
    for run in ("j1", "j4"):
        report = stdout[run][stdout[run].index("\nPlaced "):]
        said = [line for line in report.split("\n") if line.startswith("Cohort ")]
        assert said == [f"{label}: {outs[run] / file_name(what)}" for label, what in SUMMARY], run
