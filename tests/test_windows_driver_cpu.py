"""The drivers' side of painting by windows without a device: every refusal of --windows and its flags, in its exact
words, before anything is opened (epik-dna, epik-aa, epik.py), the errors of --window-groups, and groups_at_rank of the
host driver against Python's."""
import os
import struct
import subprocess

import numpy as np
import pytest

from epik_amd import capi, synth, taxonomy
from test_taxa_cpu import write_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "epik_amd", "bin")


@pytest.fixture(scope="module")
def host_bins():
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    return BIN


W = ["--windows", "100", "--window-groups", "groups.tsv"]
REFUSALS = [
    (["--window-step", "10"], "Error: --window-step needs --windows\n"),
    (["--window-mass", "0.9"], "Error: --window-mass needs --windows\n"),
    (["--window-groups", "groups.tsv"], "Error: --window-groups needs --windows\n"),
    (["--window-rank", "2"], "Error: --window-rank needs --windows\n"),
    (["--windows-per-window"], "Error: --windows-per-window needs --windows\n"),
    (["--windows", "100"], "Error: --windows needs --window-groups\n"),
    (W + ["--mates", "r2.fasta"], "Error: --windows does not work with --mates\n"),
    (W + ["--profile"], "Error: --windows does not work with --profile\n"),
    (W + ["--profile-only"], "Error: --windows does not work with --profile-only\n"),
    (W + ["--assign"], "Error: --windows does not work with --assign\n"),
    (W + ["--taxonomy", "t.tsv"], "Error: --windows does not work with --taxonomy\n"),
    (W + ["--cohort"], "Error: --windows does not work with --cohort\n"),
    (W + ["--db-shard", "2"], "Error: --windows does not work with --db-shard > 1\n"),
    (["--windows", "0", "--window-groups", "g"], "Error: --windows must be a whole number in [1, 2^31), not '0'\n"),
    (["--windows", "2147483648", "--window-groups", "g"], "Error: --windows must be a whole number in [1, 2^31), not '2147483648'\n"),
    (["--windows", "12x", "--window-groups", "g"], "Error: --windows must be a whole number in [1, 2^31), not '12x'\n"),
    (["--windows=-5", "--window-groups", "g"], "Error: --windows must be a whole number in [1, 2^31), not '-5'\n"),
    (W + ["--window-step", "101"], "Error: --window-step must be a whole number in [1, 100], not '101'\n"),
    (W + ["--window-step", "0"], "Error: --window-step must be a whole number in [1, 100], not '0'\n"),
    (W + ["--window-rank", "0"], "Error: --window-rank must be a whole number from 1 up, not '0'\n"),
    (W + ["--window-mass", "0.5"], "Error: --window-mass must be a number in (0.5, 1], not '0.5'\n"),
    (W + ["--window-mass", "1.01"], "Error: --window-mass must be a number in (0.5, 1], not '1.01'\n"),
    (W + ["--window-mass", "most"], "Error: --window-mass must be a number in (0.5, 1], not 'most'\n"),
]


@pytest.mark.parametrize("extra,message", REFUSALS, ids=[" ".join(e) for e, _ in REFUSALS])
def test_drivers_refuse_before_touching_anything(host_bins, tmp_path, extra, message):
    # (a database, query and groups file that do not exist: the error must come before any is opened, or any device asked for)
    for binary in ("epik-dna", "epik-aa") if "--mates" not in extra else ("epik-dna",):    # (epik-aa refuses --mates by itself)
        run = subprocess.run([os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "none.fasta"),
                              "-o", str(tmp_path)] + extra, capture_output=True, text=True)
        assert run.returncode == 255, run.stdout + run.stderr
        assert run.stderr == message, run.stderr
        assert "Loading database" not in run.stdout
        assert not list(tmp_path.iterdir())


def test_translate_is_refused_by_epik_aa(host_bins, tmp_path):
    run = subprocess.run([os.path.join(host_bins, "epik-aa"), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "none.fasta"),
                          "-o", str(tmp_path), "--translate", "both"] + W, capture_output=True, text=True)
    assert run.returncode == 255 and run.stderr == "Error: --windows does not work with --translate\n", run.stderr


def test_the_groups_file_is_read_before_the_database(host_bins, tmp_path):
    args = [os.path.join(host_bins, "epik-dna"), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "none.fasta"), "-o",
            str(tmp_path / "out"), "--windows", "100", "--window-groups"]
    run = subprocess.run(args + [str(tmp_path / "none.tsv")], capture_output=True, text=True)
    assert run.returncode == 255 and run.stderr == f"Error: Could not open the groups file {tmp_path / 'none.tsv'}\n", run.stderr
    (tmp_path / "groups.tsv").write_text("# groups\nA\tBacteria;Firmicutes\nB Bacteria\n")
    run = subprocess.run(args + [str(tmp_path / "groups.tsv")], capture_output=True, text=True)
    assert run.returncode == 255, run.stdout
    assert run.stderr == f"Error: {tmp_path / 'groups.tsv'}: line 3: no tab between the leaf label and the taxopath\n", run.stderr
    assert "Loading database" not in run.stdout
    for name in ("epik-dna", "epik-aa"):
        out = subprocess.run([os.path.join(host_bins, name), "--help"], capture_output=True, text=True).stdout
        for flag in ("--windows arg", "--window-step arg", "--window-mass arg", "--window-groups arg", "--window-rank arg",
                     "--windows-per-window"):
            assert flag in out, flag


def test_launcher_refusals_and_translation():
    import click
    import importlib.util
    spec = importlib.util.spec_from_file_location("epik_launcher", os.path.join(ROOT, "epik.py"))
    epik = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(epik)
    base = dict(database="db", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1, input_file="q.fasta")
    refused = [
        (dict(window_step=10), "--window-step needs --windows"),
        (dict(window_mass=0.9), "--window-mass needs --windows"),
        (dict(window_groups="g.tsv"), "--window-groups needs --windows"),
        (dict(window_rank=2), "--window-rank needs --windows"),
        (dict(windows_per_window=True), "--windows-per-window needs --windows"),
        (dict(windows=100), "--windows needs --window-groups"),
        (dict(windows=100, window_groups="g", mates="m"), "--windows does not work with --mates"),
        (dict(windows=100, window_groups="g", translate="both"), "--windows does not work with --translate"),
        (dict(windows=100, window_groups="g", profile=True), "--windows does not work with --profile"),
        (dict(windows=100, window_groups="g", profile_only=True), "--windows does not work with --profile-only"),
        (dict(windows=100, window_groups="g", assign=True), "--windows does not work with --assign"),
        (dict(windows=100, window_groups="g", taxonomy="t"), "--windows does not work with --taxonomy"),
        (dict(windows=100, window_groups="g", cohort=True), "--windows does not work with --cohort"),
        (dict(windows=100, window_groups="g", db_shard=2), "--windows does not work with --db-shard > 1"),
        (dict(windows=100, window_groups="g", window_step=101), "--window-step must be a whole number in [1, 100], not '101'"),
        (dict(windows=100, window_groups="g", window_mass=0.5), "--window-mass must lie in (0.5, 1]"),
    ]
    for options, message in refused:
        with pytest.raises(click.UsageError) as e:
            epik.driver_command(**base, **options)
        assert e.value.message == message, options
    argv = epik.driver_command(**base, windows=300, window_groups="g.tsv", window_step=75, window_mass=0.9, window_rank=2,
                               windows_per_window=True, strand="both")
    assert argv[-12:] == ["--windows", "300", "--window-groups", "g.tsv", "--window-step", "75", "--window-mass", "0.9",
                          "--window-rank", "2", "--windows-per-window", "q.fasta"]
    assert "--strand" in argv
    assert "--windows" not in epik.driver_command(**base)


@pytest.mark.parametrize("leaves,ranks", [(8, 2), (60, 3), (200, 4)])
def test_groups_at_rank_of_the_host_driver_equal_python(host_bins, tmp_path, leaves, ranks):
    tree = synth.make_tree(leaves, seed=leaves)
    text = synth.synth_taxonomy(tree, ranks)
    taxa = taxonomy.parse_taxonomy(text)
    label = taxonomy.label_branches(taxa, tree.parent, tree.labels)
    (tmp_path / "taxonomy.tsv").write_bytes(text.encode())
    write_tree(tmp_path / "tree.bin", tree.parent, tree.labels)
    deepest = 0
    for t in range(taxa.num_taxa):
        deepest = max(deepest, taxa.path[t].count(";") + 1 if taxa.path[t] else 0)
    for depth in (1, 2, deepest, deepest + 1):
        run = subprocess.run([os.path.join(host_bins, "taxa_test"), "groups", str(tmp_path / "taxonomy.tsv"), str(tmp_path / "tree.bin"),
                              str(depth), str(tmp_path / "groups.bin")], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        raw = (tmp_path / "groups.bin").read_bytes()
        G, = struct.unpack_from("<Q", raw, 0)
        group = np.frombuffer(raw, np.uint32, tree.num_nodes, 8)
        group_taxa = np.frombuffer(raw, np.uint32, G, 8 + 4 * tree.num_nodes)
        assert len(raw) == 8 + 4 * tree.num_nodes + 4 * G
        want_group, want_taxa = taxonomy.groups_at_rank(taxa, label, depth)
        assert np.array_equal(group, want_group) and list(group_taxa) == want_taxa, depth
        if depth == deepest + 1:
            assert G == 0 and (group == capi.WINDOW_NO_GROUP).all()
        elif depth == 1:
            assert G >= 1 and (group != capi.WINDOW_NO_GROUP).any()
