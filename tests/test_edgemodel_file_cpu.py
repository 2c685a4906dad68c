"""The file of --cohort-edge-model without a GPU: cohort_edgemodel_<list>.tsv from the Python and the C++ formatter byte for byte
(the stand-alone host binary, plain and under the sanitizers) and read back; the design's errors from the drivers before the
database is touched; the drivers' refusals; the launcher's flags.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import cohort as cohort_mod
from test_cohort_cpu import host_bins  # noqa: F401 (a fixture)
from test_model_file_cpu import BAD_DESIGNS, TERMS, file_case
from test_permanova_cpu import FILE_NAMES, _cells_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g17(v):
    return "NA" if np.isnan(v) else "%.17g" % v


@pytest.mark.parametrize("sanitized", [False, True])
def test_the_file_reads_back_and_the_python_and_the_c_formatters_agree(host_bins, tmp_path, sanitized):
    mass, first, bl = file_case(tmp_path)
    terms, kind, labels, values, label_names, skipped = cohort_mod.read_design(str(tmp_path / "design.tsv"), TERMS, FILE_NAMES)
    totals = cohort_mod.totals_of(mass)
    result = cohort_mod.edgemodel_host(mass, first, kind, labels, values, 99, 7, with_stat=False, with_max=False)
    text = cohort_mod.format_edgemodel_tsv(FILE_NAMES, totals, terms, kind, label_names, labels, values, 99, 7, result)
    lines = text.split("\n")
    # the head is the model's for the same design: used, columns, rank, the unused and incomplete samples, terms, groups, aliased
    model = cohort_mod.model_host(mass, first, bl, kind, labels, values, 1, 7, with_stat=False)
    model_lines = cohort_mod.format_model_tsv(FILE_NAMES, totals, terms, kind, label_names, labels, values, 1, 7, model).split("\n")
    assert lines[0] == "# epik_amd edgemodel v1  samples=9 used=6 terms=6 columns=5 rank=4 permutations=99 seed=7"
    assert lines[1:16] == model_lines[1:16] and lines[15] == "# aliased\t3\t-" and lines[16] == cohort_mod.EDGEMODEL_HEADER
    assert lines[16].split("\t")[:4] == ["term", "edge_num", "mass_ss", "mass_r2"] and len(lines[16].split("\t")) == 16
    # per term with a column, a line per branch with a defined family; the terms without a column have none
    n = mass.shape[1]
    rows = [ln.split("\t") for ln in lines[17:-1]]
    assert lines[-1] == "" and {r[0] for r in rows} == {"age", "site", "state", "dose"}
    defined = ~np.isnan(result.records["family"]["ss"]).all(axis=2)
    assert len(rows) == int(defined.sum()) and defined[0].any() and not defined[3].any() and not defined[4].any()
    t, b = 0, int(np.flatnonzero(defined[0])[0])
    fams = result.records["family"][t, b]
    want = ["age", str(b)]
    for fam in fams:
        want += [g17(fam["ss"]), g17(fam["r2"]), g17(fam["partial_r2"]), g17(fam["f"]), "NA" if np.isnan(fam["ss"]) else str(int(fam["sign"])),
                 g17(fam["p"]), g17(fam["p_adj"])]
    assert rows[0] == want
    leaf = int(np.flatnonzero(first == np.arange(n))[0])
    leaf_row = [r for r in rows if r[0] == "age" and int(r[1]) == leaf][0]
    assert leaf_row[9:] == ["NA"] * 7 and "NA" not in leaf_row[2:4]                # a leaf has no imbalance
    # the C++ reader and formatter, stand-alone
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    _cells_input(tmp_path / "mass.bin", mass, first, bl)
    (tmp_path / "names.txt").write_text("".join(name + "\n" for name in FILE_NAMES))
    run = subprocess.run([binary, "edgemodel-tsv", str(tmp_path / "cpp.tsv"), str(tmp_path / "mass.bin"), str(tmp_path / "names.txt"),
                          str(tmp_path / "design.tsv"), TERMS, "99", "7"], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr
    assert "Cohort edge model design: 6 terms, 1 lines of samples that are not in the list skipped" in run.stdout
    assert (tmp_path / "cpp.tsv").read_bytes() == text.encode()
    # read back: every double and sign of the file; the counts are not in it
    back_terms, records, info = cohort_mod.read_edgemodel_tsv(str(tmp_path / "cpp.tsv"), n)
    assert back_terms == [("age", "n", 1, 1), ("site", "f", 1, 1), ("state", "f", 1, 1), ("twice", "n", 1, 0), ("lone", "f", 0, 0),
                          ("dose", "n", 1, 1)]
    for f in cohort_mod.EDGEMODEL_FIELDS:
        a, b = np.ascontiguousarray(records["family"][f]), np.ascontiguousarray(result.records["family"][f])
        assert a.tobytes() == b.tobytes(), f
    assert info["unused"] == ["none"] and info["incomplete"] == [("z.9_-", "site"), ("s", "age")] and info["aliased"] == [(3, "-")]
    assert (info["samples"], info["used"], info["columns"], info["rank"], info["permutations"], info["seed"]) == (9, 6, 5, 4, 99, 7)
    assert info["groups"][1] == (1, 1, "gut", 4) and "strata" not in info
    # with strata the first line says so, and nothing else changes in form
    strata = np.arange(9, dtype=np.uint32) % 2
    within = cohort_mod.edgemodel_host(mass, first, kind, labels, values, 99, 7, with_stat=False, with_max=False, strata=strata)
    text = cohort_mod.format_edgemodel_tsv(FILE_NAMES, totals, terms, kind, label_names, labels, values, 99, 7, within, strata="subject")
    assert text.split("\n")[0] == lines[0] + "\tstrata=subject" and text.split("\n")[1:17] == lines[1:17]
    (tmp_path / "s.tsv").write_text(text)
    assert cohort_mod.read_edgemodel_tsv(str(tmp_path / "s.tsv"), n)[2]["strata"] == "subject"
    with pytest.raises(ValueError):
        cohort_mod.format_edgemodel_tsv(FILE_NAMES, totals, terms[:-1], kind, label_names, labels, values, 99, 7, result)
    (tmp_path / "not.tsv").write_text(text.replace("edgemodel v1", "model v1"))
    with pytest.raises(ValueError):
        cohort_mod.read_edgemodel_tsv(str(tmp_path / "not.tsv"), n)


# ---- the drivers and the launcher --------------------------------------------------------------------------------------------
DEPENDENTS = (["--cohort-edge-model-terms", "n:age"], ["--cohort-edge-model-permutations", "99"], ["--cohort-edge-model-seed", "5"])


@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_drivers_refuse_the_flags_and_read_the_design_before_the_database(host_bins, tmp_path, binary):
    out = tmp_path / "out"
    out.mkdir()
    base = [os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "none.list"), "-o", str(out)]

    def refused(extra, *words):
        run = subprocess.run(base + extra, capture_output=True, text=True)
        assert run.returncode == 255 and run.stderr.startswith("Error:"), (extra, run.stdout + run.stderr)
        assert all(w in run.stderr for w in words), (extra, run.stderr)
        assert "Loading database" not in run.stdout and "HIP device" not in run.stderr and not list(out.iterdir())
        return run

    refused(["--cohort-edge-model", "d.tsv", "--cohort-edge-model-terms", "n:age"], "--cohort-edge-model", "--cohort ")
    refused(["--cohort", "--cohort-edge-model", "d.tsv"], "--cohort-edge-model needs --cohort-edge-model-terms")
    for dependent in DEPENDENTS:
        refused(dependent, dependent[0], "needs --cohort-edge-model")
        refused(["--cohort"] + dependent, dependent[0], "needs --cohort-edge-model")
        refused(["--cohort", "--cohort-model", "d.tsv", "--cohort-model-terms", "n:age"] + dependent, dependent[0], "needs --cohort-edge-model")
    # no distance enters: --cohort-distance does not count it; --cohort-strata does
    refused(["--cohort", "--cohort-edge-model", "d.tsv", "--cohort-edge-model-terms", "n:age", "--cohort-distance", "weighted"],
            "--cohort-distance needs --cohort-permanova, --cohort-pcoa or --cohort-permdisp")
    refused(["--cohort", "--cohort-strata", "s.tsv"], "--cohort-strata needs --cohort-permanova, --cohort-permdisp, --cohort-edge-test or --cohort-model")
    shown = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert shown.returncode == 0 and "cohort_edgemodel_<list>.tsv" in shown.stdout
    for flag in ("--cohort-edge-model arg", "--cohort-edge-model-terms arg", "--cohort-edge-model-permutations arg",
                 "--cohort-edge-model-seed arg"):
        assert flag in shown.stdout, flag
    for name in "abc":
        (tmp_path / f"{name}.fasta").write_text(">r\nACGT\n")
    (tmp_path / "samples.list").write_text("a\ta.fasta\nb\tb.fasta\nc\tc.fasta\n")
    base[4] = str(tmp_path / "samples.list")
    design = str(tmp_path / "bad.tsv")
    (tmp_path / "bad.tsv").write_text("sample\tage\na\t1\nb\t2\nc\t3\n")
    model = ["--cohort", "--cohort-edge-model", design, "--cohort-edge-model-terms"]
    for value in ("0", "1000000", "many", "12x"):
        refused(model + ["n:age", "--cohort-edge-model-permutations", value], "--cohort-edge-model-permutations", "[1, 999999]")
    for value in ("18446744073709551616", "seed", "7x"):
        refused(model + ["n:age", "--cohort-edge-model-seed", value], "--cohort-edge-model-seed", "uint64")
    refused(["--cohort", "--cohort-edge-model", str(tmp_path / "nowhere.tsv"), "--cohort-edge-model-terms", "n:age"], "cannot open")
    # every error of the design, from the driver, before the database: read_cohort_design's, unchanged
    for terms, text, words in BAD_DESIGNS:
        if text is None:
            text = "# a design\nsample\tstate\tage\tsite\na\tx\t1\tg\nb\ty\t2\tg\nc\tx\t3\th\n"
        (tmp_path / "bad.tsv").write_text(text)
        refused(model + [terms], *words)
    # with strata and a good design the strata file is read next, before the database
    (tmp_path / "bad.tsv").write_text("sample\tage\na\t1\nb\t2\nc\t3\n")
    refused(model + ["n:age", "--cohort-strata", str(tmp_path / "nowhere.tsv")], "nowhere.tsv")


def test_launcher_passes_the_flags_only_when_given():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw)
    assert "cohort-edge-model" not in " ".join(default) and "cohort-edge-model" not in " ".join(epik.driver_command(**kw, cohort=True))
    assert epik.driver_command(**kw, cohort_edge_model=None, cohort_edge_model_terms=None, cohort_edge_model_permutations=None,
                               cohort_edge_model_seed=None) == default
    assert epik.driver_command(**kw, cohort=True, cohort_edge_model="d.tsv", cohort_edge_model_terms="n:age,f:state")[:-1] == \
        default[:-1] + ["--cohort", "--cohort-edge-model", "d.tsv", "--cohort-edge-model-terms", "n:age,f:state"]
    full = epik.driver_command(**kw, cohort=True, cohort_edge_model="d.tsv", cohort_edge_model_terms="f:state",
                               cohort_edge_model_permutations=9999, cohort_edge_model_seed=(1 << 64) - 1, cohort_model="d.tsv",
                               cohort_model_terms="n:age", cohort_strata="s.tsv")
    at = full.index("--cohort-edge-model")
    assert full[at:at + 8] == ["--cohort-edge-model", "d.tsv", "--cohort-edge-model-terms", "f:state", "--cohort-edge-model-permutations", "9999",
                               "--cohort-edge-model-seed", "18446744073709551615"]
    assert "--cohort-model" in full and "--cohort-strata" in full
    # --cohort-strata counts it among the analyses that allow it; --cohort-distance does not
    assert "--cohort-strata" in epik.driver_command(**kw, cohort=True, cohort_edge_model="d.tsv", cohort_edge_model_terms="n:a",
                                                    cohort_strata="s.tsv")
    for bad in (dict(cohort_edge_model="d.tsv", cohort_edge_model_terms="n:a"), dict(cohort=True, cohort_edge_model="d.tsv"),
                dict(cohort=True, cohort_edge_model_terms="n:a"), dict(cohort=True, cohort_edge_model_permutations=9),
                dict(cohort=True, cohort_edge_model_seed=9),
                dict(cohort=True, cohort_edge_model="d.tsv", cohort_edge_model_terms="n:a", cohort_distance="weighted")):
        with pytest.raises(click.UsageError):
            epik.driver_command(**kw, **bad)
    me = os.path.join(ROOT, "epik.py")
    out = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("--cohort-edge-model ", "--cohort-edge-model-terms", "--cohort-edge-model-permutations", "--cohort-edge-model-seed"):
        assert flag in out.stdout, flag
    for flags, word in ((["--cohort-edge-model", me, "--cohort-edge-model-terms", "n:a"], "--cohort"),
                        (["--cohort", "--cohort-edge-model", me], "--cohort-edge-model-terms"),
                        (["--cohort", "--cohort-edge-model-seed", "3"], "--cohort-edge-model"),
                        (["--cohort", "--cohort-edge-model", me, "--cohort-edge-model-terms", "n:a", "--cohort-edge-model-permutations", "0"],
                         "999999")):
        run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, *flags, me], capture_output=True, text=True)
        assert run.returncode == 2 and word in run.stderr, (flags, run.stdout, run.stderr)
