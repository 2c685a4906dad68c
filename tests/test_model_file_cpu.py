"""The file of --cohort-model without a GPU: the design file and the terms list, every error naming its line and column, from
Python and from the drivers before the database is touched; cohort_model_<list>.tsv from the Python and the C++ formatter byte for
byte (the stand-alone host binary, plain and under the sanitizers) and read back; the drivers' refusals; the launcher's flags.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import cohort as cohort_mod
from test_cohort_cpu import host_bins  # noqa: F401 (a fixture)
from test_permanova_cpu import FILE_NAMES, _cells_input, cohort_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
# state and site are factors, age and dose covariates, twice is age again, lone a factor of one label; z.9_- lacks a site, s an age
FILE_DESIGN = ("# a design\nsample\tstate\tage\tsite\tdose\ttwice\tlone\n"
               "q\tsick\t31\tgut\t0.5\t31\tx\n" "a\thealthy\t40.5\tskin\t1e-1\t40.5\tx\n" "skin 3\tsick\t22\tskin\t.25\t22\tx\n"
               "it's\thealthy\t+67\tgut\t2.\t+67\tx\n" "none\tsick\t50\tmouth\t1\t50\tx\n" "z.9_-\thealthy\t19\tNA\t3\t19\tx\n"
               "r\tsick\t58\tgut\t0.75\t58\tx\n" "s\thealthy\t\tmouth of 2\t4\t\tx\n" "t\tsick\t45\tgut\t1.5\t45\tx\n"
               "other\t1\t2\t3\t4\t5\t6\n")
TERMS = "n:age,f:site,f:state,n:twice,f:lone,n:dose"


def file_case(tmp_path):
    mass, first, bl, _ = cohort_input("tree15", 9, seed=8)
    mass[2] = mass[4] // U64(2) + U64(1)                                       # (cohort_input leaves sample 2 empty)
    mass[3] = 0                                                                # "none" has no mass
    (tmp_path / "design.tsv").write_text(FILE_DESIGN)
    return mass, first, bl


@pytest.mark.parametrize("sanitized", [False, True])
def test_the_file_reads_back_and_the_python_and_the_c_formatters_agree(host_bins, tmp_path, sanitized):
    mass, first, bl = file_case(tmp_path)
    terms, kind, labels, values, label_names, skipped = cohort_mod.read_design(str(tmp_path / "design.tsv"), TERMS, FILE_NAMES)
    assert skipped == 1 and terms == ["age", "site", "state", "twice", "lone", "dose"] and list(kind) == [1, 0, 0, 1, 0, 1]
    assert label_names[1] == ["gut", "skin", "mouth", "mouth of 2"] and label_names[2] == ["sick", "healthy"] and label_names[0] == []
    assert values[5, 0] == 31.0 and values[1, 5] == 0.25 and values[0, 5] == 0.1 and np.isnan(values[7, 0]) and values[2, 0] == 67.0
    totals = cohort_mod.totals_of(mass)
    model = cohort_mod.model_host(mass, first, bl, kind, labels, values, 99, 7, with_stat=False)
    text = cohort_mod.format_model_tsv(FILE_NAMES, totals, terms, kind, label_names, labels, values, 99, 7, model)
    lines = text.split("\n")
    r = model.records
    # used: nine samples less none (no mass), z.9_- (no site) and s (no age, which comes before its twice)
    assert lines[:4] == ["# epik_amd model v1  samples=9 used=6 terms=6 columns=5 rank=4 permutations=99 seed=7", "# unused\tnone",
                         "# incomplete\tz.9_-\tsite", "# incomplete\ts\tage"]
    assert lines[4:10] == ["# term\t0\tn\tage\t1\t1", "# term\t1\tf\tsite\t1\t1", "# term\t2\tf\tstate\t1\t1", "# term\t3\tn\ttwice\t1\t0",
                           "# term\t4\tf\tlone\t0\t0", "# term\t5\tn\tdose\t1\t1"]
    # the groups in the rule's order: first appearance among the used samples in list order, not in the file
    assert lines[10:15] == ["# group\t1\t0\tskin\t2", "# group\t1\t1\tgut\t4", "# group\t2\t0\thealthy\t2", "# group\t2\t1\tsick\t4",
                            "# group\t4\t0\tx\t6"]
    assert lines[15] == "# aliased\t3\t-" and lines[16] == cohort_mod.MODEL_HEADER
    assert lines[17] == "age\t1\t%.17g\t%.17g\t%.17g\t%d\t%.17g" % (r["ss"][0], r["r2"][0], r["f"][0], r["at_least"][0], r["p"][0])
    assert lines[20] == "twice\t0\tNA\tNA\tNA\tNA\tNA" and lines[21] == "lone\t0\tNA\tNA\tNA\tNA\tNA"
    assert lines[23].startswith("model\t4\t") and lines[24].startswith("residual\t1\t%.17g\t" % model.info["ss_res"])
    rest = np.float64(1.0)
    for k in (0, 1, 2, 5):
        rest = rest - r["r2"][k]
    assert lines[24] == "residual\t1\t%.17g\t%.17g\tNA\tNA\tNA" % (model.info["ss_res"], rest)
    assert lines[25] == "total\t5\t%.17g\t1\tNA\tNA\tNA" % model.info["ss_total"] and lines[26:] == [""]
    # the C++ reader and formatter, stand-alone
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    _cells_input(tmp_path / "mass.bin", mass, first, bl)
    (tmp_path / "names.txt").write_text("".join(name + "\n" for name in FILE_NAMES))
    run = subprocess.run([binary, "model-tsv", str(tmp_path / "cpp.tsv"), str(tmp_path / "mass.bin"), str(tmp_path / "names.txt"),
                          str(tmp_path / "design.tsv"), TERMS, "99", "7"], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr
    assert "Cohort model design: 6 terms, 1 lines of samples that are not in the list skipped" in run.stdout
    assert (tmp_path / "cpp.tsv").read_bytes() == text.encode()
    # read back
    back_terms, records, info = cohort_mod.read_model_tsv(str(tmp_path / "cpp.tsv"))
    assert back_terms == [("age", "n", 1, 1), ("site", "f", 1, 1), ("state", "f", 1, 1), ("twice", "n", 1, 0), ("lone", "f", 0, 0),
                          ("dose", "n", 1, 1)]
    assert records.tobytes() == model.records.tobytes()
    assert info["unused"] == ["none"] and info["incomplete"] == [("z.9_-", "site"), ("s", "age")] and info["aliased"] == [(3, "-")]
    assert (info["samples"], info["used"], info["columns"], info["rank"], info["permutations"], info["seed"]) == (9, 6, 5, 4, 99, 7)
    assert info["groups"][1] == (1, 1, "gut", 4) and "distance" not in info
    assert info["residual"][:2] == (1, float(model.info["ss_res"])) and info["total"] == (5, float(model.info["ss_total"]), 1.0)
    # over another distance the first line says so, and nothing else changes in form
    other = cohort_mod.model_host(mass, first, bl, kind, labels, values, 99, 7, with_stat=False, metric="weighted")
    text = cohort_mod.format_model_tsv(FILE_NAMES, totals, terms, kind, label_names, labels, values, 99, 7, other, distance="weighted")
    assert text.split("\n")[0] == lines[0] + "\tdistance=weighted"
    (tmp_path / "w.tsv").write_text(text)
    assert cohort_mod.read_model_tsv(str(tmp_path / "w.tsv"))[2]["distance"] == "weighted"
    with pytest.raises(ValueError):
        cohort_mod.format_model_tsv(FILE_NAMES, totals, terms[:-1], kind, label_names, labels, values, 99, 7, model)


# every error of the terms list and the design file: (terms, file text or None for FILE_DESIGN, the words of the message)
BAD_DESIGNS = (
    ("", None, ("--cohort-model-terms", "term 1", "f:NAME")),
    ("n:age,x:site", None, ("--cohort-model-terms", "term 2", "'x:site'", "f:NAME")),
    ("n:age,site", None, ("term 2", "'site'", "n:NAME")),
    ("n:age,f:", None, ("term 2", "'f:'")),
    ("n:age,f:site,f:age", None, ("term 3", "'age'", "given twice")),
    (",".join(f"n:c{i}" for i in range(17)), None, ("more than 16 terms",)),
    ("n:age,f:weight", None, ("line 2", "no column 'weight'", "term 2")),
    ("n:age", "state\tage\na\tx\t1\n", ("line 1", "must begin with 'sample'")),
    ("n:age", "sample\tage\tage\n", ("line 1", "'age' is given twice")),
    ("n:age", "sample\tage\t\n", ("line 1", "column 2 has an empty name")),
    ("n:age", "# nothing\n\n", ("no header line",)),
    ("n:age", "sample\tstate\tage\na\tx\t1\nb\ty\n", ("line 3", "2 fields, not 3")),
    ("n:age", "sample\tage\na\t1\nb\t2\na\t3\n", ("line 4", "'a' is given twice", "line 2")),
    ("n:age", "sample\tage\na\t1\nb\t2\n", ("no line for the sample 'c'",)),
    ("f:state,n:age", "sample\tage\tstate\na\t1\tx\nb\told\ty\nc\t3\tx\n", ("line 3", "column age", "'old' is not a number")),
    ("n:age", "sample\tage\na\t1\nb\t2\nc\t0x10\n", ("line 4", "column age", "'0x10' is not a number")),
    ("n:age", "sample\tage\na\t1\nb\tinf\nc\t3\n", ("line 3", "column age", "'inf' is not a number")),
    ("n:age", "sample\tage\na\t1\nb\t2\nc\t1e999\n", ("line 4", "column age", "'1e999' overflows")),
)


def test_every_error_of_the_design_names_its_line_and_column(tmp_path):
    (tmp_path / "design.tsv").write_text(FILE_DESIGN)
    for terms, text, words in BAD_DESIGNS:
        path = tmp_path / ("design.tsv" if text is None else "bad.tsv")
        if text is not None:
            path.write_text(text)
        with pytest.raises(ValueError) as e:
            cohort_mod.read_design(str(path), terms, FILE_NAMES if text is None else ["a", "b", "c"])
        assert all(w in str(e.value) for w in words), (terms, text, str(e.value))
    names = [f"s{i}" for i in range(33)]
    (tmp_path / "wide.tsv").write_text("sample\tn\tmany\n" + "".join(f"{n}\t{i}\tv{i}\n" for i, n in enumerate(names)))
    with pytest.raises(ValueError) as e:
        cohort_mod.read_design(str(tmp_path / "wide.tsv"), "n:n,f:many", names)
    assert all(w in str(e.value) for w in ("line 34", "column many", "'v32'", "more than 32"))
    # a numeric column may hold any number of distinct values
    assert cohort_mod.read_design(str(tmp_path / "wide.tsv"), "n:n", names)[3][32, 0] == 32.0


# ---- the drivers and the launcher --------------------------------------------------------------------------------------------
DEPENDENTS = (["--cohort-model-terms", "n:age"], ["--cohort-model-permutations", "99"], ["--cohort-model-seed", "5"])


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

    refused(["--cohort-model", "d.tsv", "--cohort-model-terms", "n:age"], "--cohort-model", "--cohort ")
    refused(["--cohort", "--cohort-model", "d.tsv"], "--cohort-model needs --cohort-model-terms")
    for dependent in DEPENDENTS:
        refused(dependent, dependent[0], "needs --cohort-model")
        refused(["--cohort"] + dependent, dependent[0], "needs --cohort-model")
        refused(["--cohort", "--cohort-permanova", "f.tsv"] + dependent, dependent[0], "needs --cohort-model")
    refused(["--cohort", "--cohort-distance", "weighted"], "--cohort-distance needs --cohort-permanova, --cohort-pcoa or --cohort-permdisp")
    shown = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert shown.returncode == 0 and "cohort_model_<list>.tsv" in shown.stdout
    for flag in ("--cohort-model arg", "--cohort-model-terms arg", "--cohort-model-permutations arg", "--cohort-model-seed arg"):
        assert flag in shown.stdout, flag
    for name in "abc":
        (tmp_path / f"{name}.fasta").write_text(">r\nACGT\n")
    (tmp_path / "samples.list").write_text("a\ta.fasta\nb\tb.fasta\nc\tc.fasta\n")
    base[4] = str(tmp_path / "samples.list")
    design = str(tmp_path / "bad.tsv")
    (tmp_path / "bad.tsv").write_text("sample\tage\na\t1\nb\t2\nc\t3\n")
    model = ["--cohort", "--cohort-model", design, "--cohort-model-terms"]
    for value in ("0", "1000000", "many", "12x"):
        refused(model + ["n:age", "--cohort-model-permutations", value], "--cohort-model-permutations", "[1, 999999]")
    for value in ("18446744073709551616", "seed", "7x"):
        refused(model + ["n:age", "--cohort-model-seed", value], "--cohort-model-seed", "uint64")
    refused(["--cohort", "--cohort-model", str(tmp_path / "nowhere.tsv"), "--cohort-model-terms", "n:age"], "--cohort-model", "cannot open")
    # every error of the design, from the driver, before the database
    for terms, text, words in BAD_DESIGNS:
        if text is None:
            text = "# a design\nsample\tstate\tage\tsite\na\tx\t1\tg\nb\ty\t2\tg\nc\tx\t3\th\n"
        (tmp_path / "bad.tsv").write_text(text)
        refused(model + [terms], *words)
    names = [f"s{i}" for i in range(33)]
    (tmp_path / "wide.list").write_text("".join(f"{n}\ta.fasta\n" for n in names))
    (tmp_path / "bad.tsv").write_text("sample\tn\tmany\n" + "".join(f"{n}\t{i}\tv{i}\n" for i, n in enumerate(names)))
    base[4] = str(tmp_path / "wide.list")
    refused(model + ["n:n,f:many"], "--cohort-model", "line 34", "column many", "'v32'", "more than 32")
    # a good design passes on to the device and the database (there is none); --cohort-distance takes the model as its analysis
    run = subprocess.run(base + model + ["n:n", "--cohort-model-seed", "18446744073709551615", "--cohort-distance", "unweighted"],
                         capture_output=True, text=True)
    assert run.returncode == 255 and "--cohort-model" not in run.stderr and "bad.tsv" not in run.stderr, run.stderr
    assert "Cohort model design: 1 terms, 0 lines of samples that are not in the list skipped" in run.stdout


def test_launcher_passes_the_flags_only_when_given():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw)
    assert "cohort-model" not in " ".join(default) and "cohort-model" not in " ".join(epik.driver_command(**kw, cohort=True))
    assert epik.driver_command(**kw, cohort_model=None, cohort_model_terms=None, cohort_model_permutations=None,
                               cohort_model_seed=None) == default
    assert epik.driver_command(**kw, cohort=True, cohort_model="d.tsv", cohort_model_terms="n:age,f:state")[:-1] == \
        default[:-1] + ["--cohort", "--cohort-model", "d.tsv", "--cohort-model-terms", "n:age,f:state"]
    assert epik.driver_command(**kw, cohort=True, cohort_permdisp="f.tsv", cohort_model="d.tsv", cohort_model_terms="f:state",
                               cohort_model_permutations=9999, cohort_model_seed=(1 << 64) - 1, cohort_pcoa=True,
                               cohort_distance="weighted")[:-1] == \
        default[:-1] + ["--cohort", "--cohort-permdisp", "f.tsv", "--cohort-model", "d.tsv", "--cohort-model-terms", "f:state",
                        "--cohort-model-permutations", "9999", "--cohort-model-seed", "18446744073709551615", "--cohort-pcoa",
                        "--cohort-distance", "weighted"]
    assert "--cohort-distance" in epik.driver_command(**kw, cohort=True, cohort_model="d.tsv", cohort_model_terms="f:s",
                                                      cohort_distance="unweighted")
    for bad in (dict(cohort_model="d.tsv", cohort_model_terms="n:a"), dict(cohort=True, cohort_model="d.tsv"),
                dict(cohort=True, cohort_model_terms="n:a"), dict(cohort=True, cohort_model_permutations=9),
                dict(cohort=True, cohort_model_seed=9), dict(cohort=True, cohort_distance="weighted")):
        with pytest.raises(click.UsageError):
            epik.driver_command(**kw, **bad)
    me = os.path.join(ROOT, "epik.py")
    out = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("--cohort-model ", "--cohort-model-terms", "--cohort-model-permutations", "--cohort-model-seed"):
        assert flag in out.stdout, flag
    for flags, word in ((["--cohort-model", me, "--cohort-model-terms", "n:a"], "--cohort"), (["--cohort", "--cohort-model", me], "--cohort-model-terms"),
                        (["--cohort", "--cohort-model-seed", "3"], "--cohort-model"),
                        (["--cohort", "--cohort-model", me, "--cohort-model-terms", "n:a", "--cohort-model-permutations", "0"], "999999")):
        run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, *flags, me], capture_output=True, text=True)
        assert run.returncode == 2 and word in run.stderr, (flags, run.stdout, run.stderr)
