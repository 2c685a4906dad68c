"""The abundance profile without a GPU: q() and the host mirror (epik_amd/host/profile.cpp, through bin/profile_test)
against the rule of include/epik_amd.h written out here in numpy, the clade sums against a walk of the tree, the TSV
both ways, the launcher's and the drivers' flags, and the new symbols of the C ABI."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import mixed_reads
from epik_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "epik_amd", "bin")
LWR_BITS = 30
TOO_NARROW = 0xFFFFFFFF
M64 = (1 << 64) - 1


def q(x):
    """llrint(x * 2^30), round half to even."""
    return int(np.rint(np.float64(x) * np.float64(1 << LWR_BITS)))


def numpy_rule(rows, n_rows, counts, weights, num_branches):
    """The table of the rule, read by read; Python integers modulo 2^64."""
    mass, best = [0] * num_branches, [0] * num_branches
    totals = dict(placed=0, no_hit=0, too_short=0, too_narrow=0, bad_rows=0)
    keep = rows.shape[1]
    for i in range(len(n_rows)):
        w, nr = int(weights[i]), int(n_rows[i])
        if nr == TOO_NARROW:
            totals["too_narrow"] += w
        elif nr == 0:
            totals["too_short"] += w
        elif int(counts[i, 0]) == 0:
            totals["no_hit"] += w
        else:
            totals["placed"] += w
            for j in range(min(nr, keep)):
                b = int(rows[i, j]["branch"])
                if b >= num_branches:
                    totals["bad_rows"] += 1
                    continue
                mass[b] = (mass[b] + w * q(rows[i, j]["lwr"])) & M64
                if j == 0:
                    best[b] = (best[b] + w) & M64
    return (np.array(mass, dtype=np.uint64), np.array(best, dtype=np.uint64), {k: v & M64 for k, v in totals.items()})


def brute_clade(per_branch, tree):
    """Sum over the subtree of every node, by walking up from each node to the root."""
    out = [0] * tree.num_nodes
    for b in range(tree.num_nodes):
        node = b
        while node >= 0:
            out[node] = (out[node] + int(per_branch[b])) & M64
            node = int(tree.parent[node])
    return np.array(out, dtype=np.uint64)


@pytest.fixture(scope="module")
def host_bins():
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    return BIN


def write_input(path, rows, n_rows, counts, weights, subtree_num_nodes):
    n, keep = rows.shape
    with open(path, "wb") as fh:
        fh.write(struct.pack("<3Q", n, keep, len(subtree_num_nodes)))
        fh.write(np.ascontiguousarray(rows, dtype=capi.PLACEMENT).tobytes())
        fh.write(np.ascontiguousarray(n_rows, dtype=np.uint32).tobytes())
        fh.write(np.ascontiguousarray(counts, dtype=np.uint32).tobytes())
        fh.write(np.ascontiguousarray(weights, dtype=np.uint32).tobytes())
        fh.write(np.ascontiguousarray(subtree_num_nodes, dtype=np.uint64).tobytes())


def host_profile(host_bins, tmp_path, inputs, name="out.tsv"):
    from epik_amd import profile
    out = str(tmp_path / name)
    run = subprocess.run([os.path.join(host_bins, "profile_test"), "tsv", out] + inputs, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    return out, profile.read_tsv(out)


Q_CASES = [(0.0, 0), (1.0, 1 << 30), (0.5 * 2.0 ** -30, 0), (1.5 * 2.0 ** -30, 2), (2.5 * 2.0 ** -30, 2), (5e-324, 0)]


def test_q_on_hand_picked_values(host_bins):
    from epik_amd import profile
    assert [q(x) for x, _ in Q_CASES] == [want for _, want in Q_CASES]                  # the test's own restatement
    assert profile.quantise([x for x, _ in Q_CASES]).tolist() == [want for _, want in Q_CASES]
    bits = [format(struct.unpack("<Q", struct.pack("<d", x))[0], "x") for x, _ in Q_CASES]
    run = subprocess.run([os.path.join(host_bins, "profile_test"), "q"] + bits, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert [int(line) for line in run.stdout.split()] == [want for _, want in Q_CASES]


def _oracle_rows(oracle_lib, small_case):
    _, db = small_case
    rng = np.random.default_rng(1)
    reads = mixed_reads(rng, 600, db.kmer_size, alphabet_amb="ACGTNRYKMSWBDHV-", max_len=200)
    reads = [r.lower() if i % 7 == 0 else r for i, r in enumerate(reads)]
    reads += ["ACG", "", "NNNNNNNNNN", "-" * 12]
    rows, n_rows, counts = oracle_lib.Oracle.from_synth(db).place(*synth.pack_reads(reads), num_threads=0)
    weights = np.random.default_rng(2).integers(0, 5, size=len(reads)).astype(np.uint32)
    return rows, n_rows, counts, weights


def test_host_mirror_equals_the_rule_on_oracle_rows(host_bins, oracle_lib, small_case, tmp_path):
    tree, db = small_case
    rows, n_rows, counts, weights = _oracle_rows(oracle_lib, small_case)
    short, no_hit = n_rows == 0, (n_rows != 0) & (counts[:, 0] == 0)
    placed = ~short & ~no_hit
    assert short.sum() >= 2 and no_hit.sum() > 0 and placed.sum() > 0      # all three classes, each with weight
    assert weights[short].sum() > 0 and weights[no_hit].sum() > 0 and (weights == 0).any()
    mass, best, totals = numpy_rule(rows, n_rows, counts, weights, db.num_branches)
    write_input(tmp_path / "in.bin", rows, n_rows, counts, weights, tree.subtree_num_nodes)
    _, got = host_profile(host_bins, tmp_path, [str(tmp_path / "in.bin")])
    assert np.array_equal(got["mass_q"], mass) and np.array_equal(got["best"], best)
    assert (got["placed"], got["no_hit"], got["too_short"]) == (totals["placed"], totals["no_hit"], totals["too_short"])
    assert got["records"] == int(weights.sum()) and totals["bad_rows"] == 0
    assert got["no_hit"] == int(weights[no_hit].sum()) and got["too_short"] == int(weights[short].sum())
    # the fabricated rows (branches 0, 1, 2, ... with LWR 1/N) of the reads without hits add no mass: branches 0..6
    # hold what the placed reads alone put there
    keep = rows.shape[1]
    assert all(rows[i, j]["branch"] == j for i in np.nonzero(no_hit)[0] for j in range(keep))
    only_placed = numpy_rule(rows[placed], n_rows[placed], counts[placed], weights[placed], db.num_branches)
    assert np.array_equal(got["mass_q"][:keep], only_placed[0][:keep])
    assert np.array_equal(got["best"][:keep], only_placed[1][:keep])
    spread = numpy_rule(rows, n_rows, np.ones_like(counts), weights, db.num_branches)     # what a jplace reader would sum
    assert (spread[0][:keep] > mass[:keep]).all()


def test_too_narrow_and_bad_rows_on_the_host(host_bins, tmp_path):
    rows = np.zeros((4, 3), dtype=capi.PLACEMENT)
    rows["branch"] = [[1, 9, 2], [5, 0, 0], [0, 1, 2], [2, 2, 2]]
    rows["lwr"] = [[0.5, 0.25, 0.25], [1.0, 0, 0], [0.2, 0.2, 0.2], [1.0, 0.5, 0.25]]
    n_rows = np.array([3, 1, TOO_NARROW, 0], dtype=np.uint32)
    counts = np.ones((4, 3), dtype=np.uint32)
    weights = np.array([3, 0xFFFFFFFF, 7, 2], dtype=np.uint32)
    write_input(tmp_path / "in.bin", rows, n_rows, counts, weights, [1, 1, 3, 1, 5])
    _, got = host_profile(host_bins, tmp_path, [str(tmp_path / "in.bin")])
    mass, best, totals = numpy_rule(rows, n_rows, counts, weights, 5)
    assert totals == dict(placed=3 + 0xFFFFFFFF, no_hit=0, too_short=2, too_narrow=7, bad_rows=2)
    assert mass.tolist() == [0, 3 << 29, 3 << 28, 0, 0] and best.tolist() == [0, 3, 0, 0, 0]
    assert np.array_equal(got["mass_q"], mass) and np.array_equal(got["best"], best)
    assert got["records"] == 3 + 0xFFFFFFFF + 2 + 7 and got["too_short"] == 2


@pytest.mark.parametrize("leaves", [8, 500, 1500])
def test_clade_sums_against_a_walk_of_the_tree(host_bins, tmp_path, leaves):
    from epik_amd import profile
    tree = synth.make_tree(leaves, seed=leaves)
    n = tree.num_nodes
    # every subtree is the id range the prefix sums rely on
    for b in range(n):
        below = {b}
        for c in range(b - 1, -1, -1):   # post-order: children come before their parent
            if int(tree.parent[c]) in below:
                below.add(c)
        assert below == set(range(b - int(tree.subtree_num_nodes[b]) + 1, b + 1))
        if leaves > 8 and b > 40:
            break
    rng = np.random.default_rng(leaves)
    per_branch = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)   # (sums wrap: modulo 2^64 on both sides)
    want = brute_clade(per_branch, tree)
    assert np.array_equal(profile.clade_sums(per_branch, tree.subtree_num_nodes), want)
    # ... and the host's: one read per branch whose single row carries LWR 1, weight w -> mass = w << 30
    w = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    rows = np.zeros((n, 1), dtype=capi.PLACEMENT)
    rows["branch"][:, 0], rows["lwr"][:, 0] = np.arange(n), 1.0
    write_input(tmp_path / "in.bin", rows, np.ones(n, np.uint32), np.ones((n, 1), np.uint32), w, tree.subtree_num_nodes)
    _, got = host_profile(host_bins, tmp_path, [str(tmp_path / "in.bin")])
    assert np.array_equal(got["clade_best"], brute_clade(w, tree))
    assert np.array_equal(got["clade_mass_q"], brute_clade(w.astype(np.uint64) << np.uint64(30), tree))
    assert got["clade_best"][n - 1] == int(w.astype(np.uint64).sum())   # the root's clade is the sample


def test_tsv_round_trip_and_both_writers_agree(host_bins, oracle_lib, small_case, tmp_path):
    from epik_amd import profile
    tree, db = small_case
    rows, n_rows, counts, weights = _oracle_rows(oracle_lib, small_case)
    write_input(tmp_path / "in.bin", rows, n_rows, counts, weights, tree.subtree_num_nodes)
    path, got = host_profile(host_bins, tmp_path, [str(tmp_path / "in.bin")])
    mass, best, totals = numpy_rule(rows, n_rows, counts, weights, db.num_branches)
    with open(path) as fh:
        lines = fh.read().split("\n")
    assert lines[0] == (f"# epik_amd profile v1\tlwr_bits=30\trecords={int(weights.sum())}\tplaced={totals['placed']}"
                        f"\tno_hit={totals['no_hit']}\ttoo_short={totals['too_short']}")
    assert lines[1] == "edge_num\tbest\tmass_q\tmass\tclade_best\tclade_mass_q\tclade_mass"
    assert len(lines) == 2 + db.num_branches + 1 and lines[-1] == ""
    b = int(np.argmax(mass))
    assert lines[2 + b].split("\t")[:4] == [str(b), str(int(best[b])), str(int(mass[b])), "%.9f" % (int(mass[b]) / 2.0 ** 30)]
    assert got["edge_num"].tolist() == list(range(db.num_branches)) and got["lwr_bits"] == 30
    assert np.allclose(got["mass"], mass.astype(np.float64) / 2.0 ** 30, rtol=0, atol=5e-10)
    # the Python writer writes the same bytes, and reads its own file back
    sample = profile.SampleProfile(mass, best, totals)
    profile.write_tsv(str(tmp_path / "py.tsv"), sample, tree.subtree_num_nodes)
    with open(path, "rb") as a, open(tmp_path / "py.tsv", "rb") as c:
        assert a.read() == c.read()
    again = profile.read_tsv(str(tmp_path / "py.tsv"))
    assert all(np.array_equal(again[k], got[k]) for k in got)


def test_merging_two_profiles_is_profiling_the_concatenation(host_bins, oracle_lib, small_case, tmp_path):
    from epik_amd import profile
    tree, db = small_case
    rows, n_rows, counts, weights = _oracle_rows(oracle_lib, small_case)
    cut = 251
    write_input(tmp_path / "all.bin", rows, n_rows, counts, weights, tree.subtree_num_nodes)
    write_input(tmp_path / "a.bin", rows[:cut], n_rows[:cut], counts[:cut], weights[:cut], tree.subtree_num_nodes)
    write_input(tmp_path / "b.bin", rows[cut:], n_rows[cut:], counts[cut:], weights[cut:], tree.subtree_num_nodes)
    whole, _ = host_profile(host_bins, tmp_path, [str(tmp_path / "all.bin")], "whole.tsv")
    parts, _ = host_profile(host_bins, tmp_path, [str(tmp_path / "b.bin"), str(tmp_path / "a.bin")], "parts.tsv")
    with open(whole, "rb") as a, open(parts, "rb") as b:
        assert a.read() == b.read()
    pa = profile.SampleProfile(*numpy_rule(rows[:cut], n_rows[:cut], counts[:cut], weights[:cut], db.num_branches))
    pb = profile.SampleProfile(*numpy_rule(rows[cut:], n_rows[cut:], counts[cut:], weights[cut:], db.num_branches))
    both = numpy_rule(rows, n_rows, counts, weights, db.num_branches)
    merged = pa.merged(pb)
    assert np.array_equal(merged.mass, both[0]) and np.array_equal(merged.best, both[1]) and merged.totals == both[2]


def test_launcher_passes_the_flags_only_when_given():
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="q.fasta")
    default = epik.driver_command(**kw)
    assert "--profile" not in default and "--profile-only" not in default
    assert epik.driver_command(**kw, profile=False, profile_only=False) == default
    with_profile = epik.driver_command(**kw, profile=True)
    assert with_profile[:-1] == default[:-1] + ["--profile"] and with_profile[-1] == default[-1]
    only = epik.driver_command(**kw, profile_only=True, strand="both")
    assert only[:-1] == default[:-1] + ["--strand", "both", "--profile-only"] and "--profile" not in only
    out = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--profile " in out.stdout and "--profile-only" in out.stdout


@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
@pytest.mark.parametrize("extra", [["--profile-only", "--db-shard", "2"], ["--db-shard=2", "--profile-only"]])
def test_drivers_refuse_profile_only_of_a_sharded_database_before_touching_anything(host_bins, tmp_path, binary, extra):
    run = subprocess.run([os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q",
                          str(tmp_path / "none.fasta"), "-o", str(tmp_path)] + extra, capture_output=True, text=True)
    assert run.returncode == 255, run.stdout + run.stderr
    assert run.stderr.startswith("Error:") and "--profile-only" in run.stderr and "--db-shard" in run.stderr
    assert "Loading database" not in run.stdout and "HIP device" not in run.stderr
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_driver_help_names_both_flags(host_bins, binary):
    out = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--profile " in out.stdout and "--profile-only" in out.stdout


def test_profile_symbols_exist_and_refuse_null():
    lib = capi.load()
    names = ("epik_amd_profile_create", "epik_amd_profile_destroy", "epik_amd_profile_reset", "epik_amd_profile_read",
             "epik_amd_profile_info", "epik_amd_profile_add_device", "epik_amd_placer_profile_reads",
             "epik_amd_placer_profile_strands", "epik_amd_placer_profile_frames")
    for name in names:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert capi.ABI_VERSION == 3 and capi.PROFILE_LWR_BITS == 30
    out = ctypes.c_void_p(7)
    assert lib.epik_amd_profile_create(None, ctypes.byref(out)) == capi.ERR_INVALID and not out.value
    assert b"null placer" in lib.epik_amd_last_error()
    assert lib.epik_amd_profile_create(None, None) == capi.ERR_INVALID
    lib.epik_amd_profile_destroy(None)                      # (as free(NULL))
    assert lib.epik_amd_profile_reset(None) == capi.ERR_INVALID
    assert lib.epik_amd_profile_read(None, None, None, None) == capi.ERR_INVALID
    assert lib.epik_amd_profile_info(None, None, None) == capi.ERR_INVALID
    assert lib.epik_amd_profile_add_device(None, None, None, None, None, 1, None) == capi.ERR_INVALID
    assert b"null profile" in lib.epik_amd_last_error()
    assert lib.epik_amd_placer_profile_reads(None, None, None, None, None, 1) == capi.ERR_INVALID
    assert lib.epik_amd_placer_profile_strands(None, None, None, None, None, 1, capi.STRAND_BOTH, None) == capi.ERR_INVALID
    assert lib.epik_amd_placer_profile_frames(None, None, None, None, None, 1, capi.FRAMES_BOTH, None) == capi.ERR_INVALID
    assert b"null placer" in lib.epik_amd_last_error()
    assert ctypes.sizeof(capi.ProfileTotals) == 40
