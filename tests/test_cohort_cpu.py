"""A cohort of samples without a GPU (include/epik_amd.h: epik_amd_cohort): the host mirror's cells and
epik_amd_cohort_kr_host against the rule restated here in numpy -- bit for bit --, hand-derived distances, the
properties of a metric on random cohorts, the error cases that need no device, the refusals of the drivers and the
launcher, and the host test binary."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, synth
from test_assign_cpu import caterpillar
from test_profile_gpu import numpy_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "epik_amd", "bin")
U64 = np.uint64
TOTALS = ("placed", "no_hit", "too_short", "too_narrow", "bad_rows")


# ---- the rule, restated ----------------------------------------------------------------------------------------------
def numpy_first(parent):
    """first[b] by walking up from every node (no prefix sums, no sizes)."""
    parent = np.asarray(parent, dtype=np.int64)
    first = np.arange(len(parent), dtype=np.int64)
    for b in range(len(parent)):     # post-order: a child comes before its parent, so first[b] is final when b is reached
        if parent[b] >= 0:
            first[parent[b]] = min(first[parent[b]], first[b])
    return first.astype(np.uint32)


def numpy_kr(mass, first, branch_length):
    """KR of the rule: prefix sums in uint64, a python loop over the branches, S x S float64 array operations."""
    mass = np.asarray(mass, dtype=U64)
    s, n = mass.shape
    first = np.asarray(first, dtype=np.int64)
    bl = np.asarray(branch_length, dtype=np.float64)
    prefix = np.zeros((s, n + 1), dtype=U64)
    np.cumsum(mass, axis=1, dtype=U64, out=prefix[:, 1:])
    total = prefix[:, n]
    clade = prefix[:, 1:] - prefix[:, first]
    below = clade - mass
    with np.errstate(invalid="ignore", divide="ignore"):
        c = clade.astype(np.float64) / total.astype(np.float64)[:, None]
        b = below.astype(np.float64) / total.astype(np.float64)[:, None]
        acc = np.zeros((s, s), dtype=np.float64)
        for x in range(n):
            acc = acc + (0.5 * bl[x]) * (np.abs(c[:, x][:, None] - c[:, x][None, :]) + np.abs(b[:, x][:, None] - b[:, x][None, :]))
    empty = total == 0
    acc[empty, :] = -1.0
    acc[:, empty] = -1.0
    np.fill_diagonal(acc, 0.0)
    return acc


def numpy_cohort(rows, n_rows, counts, weights, samples, num_samples, num_branches):
    """The cells of the rule: the profile's rule (test_profile_gpu.numpy_rule) applied per sample."""
    samples = np.asarray(samples)
    mass, best = np.zeros((num_samples, num_branches), U64), np.zeros((num_samples, num_branches), U64)
    totals = []
    for s in range(num_samples):
        m = samples == s
        mass[s], best[s], t = numpy_rule(rows[m], n_rows[m], counts[m], None if weights is None else np.asarray(weights)[m],
                                         num_branches)
        totals.append(t)
    return mass, best, totals, int((samples >= num_samples).sum())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(U64), b.view(U64))


def assert_cells(got, want, what=""):
    mass, best, totals, bad = want
    assert got.bad_samples == bad, (what, got.bad_samples, bad)
    for s, t in enumerate(totals):
        assert {k: int(got.totals[s][k]) for k in TOTALS} == t, (what, s, got.totals[s], t)
    assert np.array_equal(got.best, best), (what, np.argwhere(got.best != best)[:10])
    assert np.array_equal(got.mass, mass), (what, np.argwhere(got.mass != mass)[:10])


def random_cells(rng, num_samples, num_branches, empty=None, bits=40):
    mass = rng.integers(0, 1 << bits, size=(num_samples, num_branches), dtype=np.uint64)
    mass[rng.random(mass.shape) < 0.3] = 0
    if empty is not None and num_samples > 1:
        mass[empty % num_samples] = 0
    return mass


TREES = {}


def tree_case(name):
    """(parent, branch_length) of the trees of the issue, some lengths 0."""
    if name not in TREES:
        if name == "one":
            parent, bl = np.array([-1]), np.array([0.25])
        elif name == "ladder10399":
            parent, bl = caterpillar(10_399)
            bl = bl.copy()
        else:
            tree = synth.make_tree({"tree15": 8, "tree2999": 1500}[name], seed=30)
            parent, bl = tree.parent, tree.branch_length.copy()
        bl[::5] = 0.0
        TREES[name] = (np.asarray(parent, dtype=np.int64), bl)
    return TREES[name]


@pytest.fixture(scope="module")
def host_bins():
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    return BIN


# ---- KR: the host mirror against the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("tree_name", ["one", "tree15", "tree2999", "ladder10399"])
@pytest.mark.parametrize("num_samples", [1, 2, 33])
def test_kr_host_equals_the_numpy_restatement_bit_for_bit(tree_name, num_samples):
    parent, bl = tree_case(tree_name)
    first = numpy_first(parent)
    assert np.array_equal(first, cohort_mod.first_of(parent))
    rng = np.random.default_rng(1000 + num_samples)
    mass = random_cells(rng, num_samples, len(parent), empty=1)
    got = cohort_mod.kr_host(mass, first, bl)
    want = numpy_kr(mass, first, bl)
    assert same_bits(got, want), np.argwhere(got.view(U64) != want.view(U64))[:10]
    if num_samples > 1:
        assert (got[1] == np.where(np.arange(num_samples) == 1, 0.0, -1.0)).all() and (got[:, 1] == got[1]).all()
    if num_samples == 33 and len(parent) > 1:
        rest = np.delete(np.delete(got, 1, 0), 1, 1)
        assert (rest[~np.eye(32, dtype=bool)] > 0).all()


def test_two_samples_on_sister_branches_are_the_path_between_the_midpoints():
    first = cohort_mod.first_of([2, 2, -1])
    kr = cohort_mod.kr_host(np.array([[5, 0, 0], [0, 7, 0]], U64), first, [0.5, 0.25, 0.0])
    assert same_bits(kr, [[0.0, 0.375], [0.375, 0.0]])          # 0.25 + 0.125, exactly
    kr = cohort_mod.kr_host(np.array([[5, 0, 0], [0, 0, 7]], U64), first, [0.5, 0.25, 0.2])
    assert kr[0, 0] == 0.0 and kr[1, 1] == 0.0 and kr[0, 1] == kr[1, 0]
    assert abs(kr[0, 1] - 0.35) <= np.spacing(0.35), kr[0, 1]   # 0.25 + 0.1, within 1 ulp


def test_properties_on_random_cohorts():
    tree = synth.make_tree(40, seed=7)
    parent, bl = tree.parent, tree.branch_length
    first = numpy_first(parent)
    n = len(parent)
    rng = np.random.default_rng(5)
    mass = random_cells(rng, 12, n, bits=50)
    kr = cohort_mod.kr_host(mass, first, bl)
    assert np.array_equal(kr.view(U64), kr.T.copy().view(U64)) and not kr.diagonal().any() and (kr >= 0).all()
    # the triangle inequality, within 1e-12 relative
    through = kr[:, :, None] + kr[None, :, :]                             # [s][u][t] = kr[s][u] + kr[u][t]
    assert (kr[:, None, :] <= through * (1 + 1e-12)).all()
    # one sample's masses times 3: with the sample's total below 2^50 every clade sum and its triple convert exactly,
    # and the quotients are the same rationals, rounded once
    low = random_cells(rng, 12, n, bits=43)
    tripled = low.copy()
    tripled[4] *= U64(3)
    assert int(low[4].max()) < 1 << 50 and int(low[4].sum()) < 1 << 50 and int(tripled[4].sum()) < 1 << 53
    assert same_bits(cohort_mod.kr_host(tripled, first, bl), cohort_mod.kr_host(low, first, bl))
    # all of a sample's mass on branch b moved to b's parent: the distance to any other sample moves by at most the
    # path between the two midpoints
    for b in (0, 3, n // 2, n - 2):
        p = int(parent[b])
        moved = low.copy()
        moved[4, p] += moved[4, b]
        moved[4, b] = 0
        before, after = cohort_mod.kr_host(low, first, bl)[4], cohort_mod.kr_host(moved, first, bl)[4]
        share = float(low[4, b]) / float(low[4].sum())
        path = (bl[b] + bl[p]) / 2
        # (two sums of 4 n rounded terms each: their rounding is at most 4 n ulps of the larger distance apart)
        slack = 8 * n * np.finfo(np.float64).eps * before.max()
        others = np.arange(12) != 4
        assert (np.abs(after - before)[others] <= path + slack).all(), (b, np.abs(after - before).max(), path)
        assert (np.abs(after - before)[others] <= share * path + slack).all(), (b, np.abs(after - before).max(), share * path)


# ---- the cells: the host mirror through its test binary --------------------------------------------------------------
def write_add_input(path, rows, n_rows, counts, weights, samples, num_branches, num_samples):
    n, keep = rows.shape
    with open(path, "wb") as fh:
        fh.write(np.array([n, keep, num_branches, num_samples], dtype="<u8").tobytes())
        for arr, dtype in ((rows, capi.PLACEMENT), (n_rows, "<u4"), (counts, "<u4"), (weights, "<u4"), (samples, "<u4")):
            fh.write(np.ascontiguousarray(arr, dtype=dtype).tobytes())


def hand_rows(rng, n, keep, num_branches):
    rows = np.zeros((n, keep), dtype=capi.PLACEMENT)
    rows["branch"] = rng.integers(0, num_branches, size=(n, keep))
    rows["lwr"] = rng.random((n, keep))
    rows["lwr"][::9, 0] = 0.5 + 2.0 ** -31          # a tie of q(): half to even
    n_rows = rng.integers(0, keep + 1, size=n).astype(np.uint32)
    n_rows[::17] = 0xFFFFFFFF
    counts = rng.integers(0, 3, size=(n, keep)).astype(np.uint32)
    rows["branch"][5::23, min(1, keep - 1)] = num_branches + 3       # bad rows
    return rows, n_rows, counts


def test_host_mirror_adds_and_merges_as_the_rule_says(host_bins, tmp_path):
    rng = np.random.default_rng(3)
    n, keep, branches, num_samples = 700, 7, 29, 5
    rows, n_rows, counts = hand_rows(rng, n, keep, branches)
    weights = rng.integers(0, 4, size=n).astype(np.uint32)
    weights[3::29] = 0xFFFFFFFF
    samples = rng.integers(0, num_samples + 2, size=n).astype(np.uint32)      # some reads of no sample
    samples[samples == 3] = 1                                                # sample 3 stays empty
    cut = 301
    write_add_input(tmp_path / "a.bin", rows[:cut], n_rows[:cut], counts[:cut], weights[:cut], samples[:cut], branches, num_samples)
    write_add_input(tmp_path / "b.bin", rows[cut:], n_rows[cut:], counts[cut:], weights[cut:], samples[cut:], branches, num_samples)
    subprocess.run([os.path.join(host_bins, "cohort_test"), "add", str(tmp_path / "out.bin"), str(tmp_path / "a.bin"),
                    str(tmp_path / "b.bin")], check=True)
    raw = np.fromfile(tmp_path / "out.bin", dtype="<u8")
    cells = num_samples * branches
    assert raw.size == 2 * cells + 5 * num_samples + 1
    got = cohort_mod.CohortCells(raw[:cells].reshape(num_samples, branches), raw[cells:2 * cells].reshape(num_samples, branches),
                                 raw[2 * cells:2 * cells + 5 * num_samples].copy().view(cohort_mod._TOTALS_DTYPE), int(raw[-1]))
    want = numpy_cohort(rows, n_rows, counts, weights, samples, num_samples, branches)
    assert_cells(got, want)
    assert want[3] > 0 and not want[0][3].any() and sum(t["bad_rows"] for t in want[2]) > 0


def test_host_test_binary_kr_is_the_library_s(host_bins, tmp_path):
    parent, bl = tree_case("tree15")
    first = numpy_first(parent)
    mass = random_cells(np.random.default_rng(8), 6, len(parent), empty=2)
    with open(tmp_path / "kr.bin", "wb") as fh:
        fh.write(np.array([6, len(parent)], dtype="<u8").tobytes() + mass.tobytes() + first.tobytes() + bl.tobytes())
    subprocess.run([os.path.join(host_bins, "cohort_test"), "kr", str(tmp_path / "out.bin"), str(tmp_path / "kr.bin")], check=True)
    got = np.fromfile(tmp_path / "out.bin", dtype="<f8").reshape(6, 6)
    assert same_bits(got, cohort_mod.kr_host(mass, first, bl)) and same_bits(got, numpy_kr(mass, first, bl))
    bl_bad = bl.copy()
    bl_bad[4] = -0.5
    with open(tmp_path / "bad.bin", "wb") as fh:
        fh.write(np.array([6, len(parent)], dtype="<u8").tobytes() + mass.tobytes() + first.tobytes() + bl_bad.tobytes())
    run = subprocess.run([os.path.join(host_bins, "cohort_test"), "kr", str(tmp_path / "o.bin"), str(tmp_path / "bad.bin")],
                         capture_output=True, text=True)
    assert run.returncode == 1 and "branch 4" in run.stderr


# ---- errors that need no device ----------------------------------------------------------------------------------------
def test_cohort_symbols_exist_and_refuse_what_the_header_says():
    lib = capi.load()
    names = ("epik_amd_cohort_create", "epik_amd_cohort_destroy", "epik_amd_cohort_reset", "epik_amd_cohort_info",
             "epik_amd_cohort_read", "epik_amd_cohort_add_cells", "epik_amd_cohort_add_device", "epik_amd_cohort_kr_device",
             "epik_amd_cohort_kr", "epik_amd_cohort_kr_host", "epik_amd_placer_cohort_reads", "epik_amd_placer_cohort_strands",
             "epik_amd_placer_cohort_frames", "epik_amd_placer_cohort_mates")
    for name in names:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert capi.ABI_VERSION == 3
    err = lambda: lib.epik_amd_last_error().decode()
    out = ctypes.c_void_p(7)
    assert lib.epik_amd_cohort_create(None, 4, ctypes.byref(out)) == capi.ERR_INVALID and not out.value and "null placer" in err()
    assert lib.epik_amd_cohort_create(None, 4, None) == capi.ERR_INVALID
    lib.epik_amd_cohort_destroy(None)                       # (as free(NULL))
    for call in (lambda: lib.epik_amd_cohort_reset(None), lambda: lib.epik_amd_cohort_info(None, None, None, None),
                 lambda: lib.epik_amd_cohort_read(None, None, None, None, None),
                 lambda: lib.epik_amd_cohort_add_cells(None, None, None, None),
                 lambda: lib.epik_amd_cohort_add_device(None, None, None, None, None, None, 1, None),
                 lambda: lib.epik_amd_cohort_kr_device(None, None, None, None, None),
                 lambda: lib.epik_amd_cohort_kr(None, None, None, None)):
        assert call() == capi.ERR_INVALID and "null cohort" in err()
    assert lib.epik_amd_placer_cohort_reads(None, None, None, None, None, None, 1) == capi.ERR_INVALID and "null placer" in err()
    for fn, mode in ((lib.epik_amd_placer_cohort_strands, capi.STRAND_BOTH), (lib.epik_amd_placer_cohort_frames, capi.FRAMES_BOTH),
                     (lib.epik_amd_placer_cohort_mates, capi.STRAND_FORWARD)):
        assert fn(None, None, None, None, None, None, 1, mode, None) == capi.ERR_INVALID and "null placer" in err()
    # kr_host: the shapes, first[] and the lengths
    first = cohort_mod.first_of([2, 2, -1])
    mass = np.ones((2, 3), U64)
    kr = np.zeros((2, 2))
    bl = np.array([0.1, 0.2, 0.0])
    args = lambda m=mass, s=2, n=3, f=first, l=bl: (m.ctypes.data, s, n, f.ctypes.data, l.ctypes.data, kr.ctypes.data)
    assert lib.epik_amd_cohort_kr_host(*args()) == capi.OK
    assert lib.epik_amd_cohort_kr_host(*args(s=0)) == capi.ERR_INVALID and "num_samples is 0" in err()
    assert lib.epik_amd_cohort_kr_host(*args(n=0)) == capi.ERR_INVALID
    assert lib.epik_amd_cohort_kr_host(None, 2, 3, first.ctypes.data, bl.ctypes.data, kr.ctypes.data) == capi.ERR_INVALID
    for bad, word in ((-0.1, "branch 1"), (np.nan, "branch 1"), (np.inf, "branch 1")):
        lengths = np.array([0.1, bad, 0.0])
        assert lib.epik_amd_cohort_kr_host(*args(l=lengths)) == capi.ERR_INVALID and word in err() and "length" in err()
    above = np.array([0, 2, 0], dtype=np.uint32)
    assert lib.epik_amd_cohort_kr_host(*args(f=above)) == capi.ERR_INVALID and "branch 1" in err() and "first" in err()
    with pytest.raises(capi.EpikAmdError):
        cohort_mod.kr_host(mass, first, [0.1, -1.0, 0.0])
    with pytest.raises(ValueError):
        cohort_mod.kr_host(mass, first[:2], bl)


# ---- the drivers and the launcher refuse before they touch anything ---------------------------------------------------
@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
@pytest.mark.parametrize("extra,words", [
    (["--cohort", "--mates", "r2.fasta"], ("--mates",)),          # (epik-aa refuses --mates by itself, in its own words)
    (["--cohort", "--profile"], ("--cohort", "--profile")),
    (["--profile-only", "--cohort"], ("--cohort", "--profile-only")),
    (["--cohort", "--assign"], ("--cohort", "--assign")),
    (["--cohort", "--db-shard", "2"], ("--cohort", "--db-shard")),
])
def test_drivers_refuse_the_flags_cohort_does_not_combine_with(host_bins, tmp_path, binary, extra, words):
    run = subprocess.run([os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q",
                          str(tmp_path / "none.list"), "-o", str(tmp_path)] + extra, capture_output=True, text=True)
    assert run.returncode == 255, run.stdout + run.stderr
    assert run.stderr.startswith("Error:") and all(w in run.stderr for w in words), run.stderr
    assert "Loading database" not in run.stdout and "HIP device" not in run.stderr
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_drivers_refuse_a_bad_list_before_the_database(host_bins, tmp_path, binary):
    (tmp_path / "a.fasta").write_text(">r\nACGTACGT\n")
    out = tmp_path / "out"
    out.mkdir()
    lists = {
        "no tab": ("# samples\n\nfirst\ta.fasta\nsecond a.fasta\n", ("line 4", "name<TAB>path")),
        "twice": ("first\ta.fasta\n# again\nfirst\ta.fasta\n", ("line 3", "'first'", "twice")),
        "unreadable": ("first\ta.fasta\nsecond\tmissing.fasta\n", ("line 2", "missing.fasta")),
        "empty": ("# nothing\n\n", ("names no sample",)),
        "no name": ("\ta.fasta\n", ("line 1",)),
    }
    for name, (text, words) in lists.items():
        path = tmp_path / "samples.list"
        path.write_text(text)
        run = subprocess.run([os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q", str(path), "-o", str(out),
                              "--cohort"], capture_output=True, text=True)
        assert run.returncode == 255, (name, run.stdout, run.stderr)
        assert run.stderr.startswith("Error: --cohort") and all(w in run.stderr for w in words), (name, run.stderr)
        assert "Loading database" not in run.stdout and "HIP device" not in run.stderr and not list(out.iterdir())
    run = subprocess.run([os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "no.list"),
                          "-o", str(out), "--cohort"], capture_output=True, text=True)
    assert run.returncode == 255 and "no.list" in run.stderr and "Loading database" not in run.stdout


@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_driver_help_names_the_flag(host_bins, binary):
    out = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort " in out.stdout and "cohort_kr_<list>.tsv" in out.stdout


def test_launcher_passes_the_flag_only_when_given():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw)
    assert "--cohort" not in default and epik.driver_command(**kw, cohort=False) == default
    assert epik.driver_command(**kw, cohort=True)[:-1] == default[:-1] + ["--cohort"]
    assert epik.driver_command(**{**kw, "gpus": 2}, cohort=True, strand="both")[:-1] == default[:-1] + [
        "--gpus", "2", "--strand", "both", "--cohort"]
    for bad in (dict(mates="r2.fasta"), dict(profile=True), dict(profile_only=True), dict(assign=True), dict(db_shard=2)):
        with pytest.raises(click.UsageError):
            epik.driver_command(**kw, cohort=True, **bad)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort" in out.stdout
    me = os.path.join(ROOT, "epik.py")
    for extra in (["--cohort", "--profile-only"], ["--cohort", "--assign"], ["--cohort", "--db-shard", "2"], ["--cohort", "--mates", me]):
        run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT] + extra + [me], capture_output=True, text=True)
        assert run.returncode == 2, (extra, run.stdout, run.stderr)


def test_the_files_of_the_drivers_read_back():
    names = ["a", "b b", "c"]
    mass = np.array([[0, 5, 0], [0, 0, 0], [1 << 63, 0, 7]], U64)
    best = np.array([[0, 1, 0], [0, 0, 0], [0, 2, 0]], U64)
    totals = np.zeros(3, dtype=cohort_mod._TOTALS_DTYPE)
    totals["placed"], totals["too_short"] = [1, 0, 2], [0, 4, 0]
    cells = cohort_mod.CohortCells(mass, best, totals)
    assert cohort_mod.format_samples_tsv(names, cells) == (
        "name\trecords\tplaced\tno_hit\ttoo_short\ttoo_narrow\ttotal_mass_q\na\t1\t1\t0\t0\t0\t5\nb b\t4\t0\t0\t4\t0\t0\n"
        f"c\t2\t2\t0\t0\t0\t{(1 << 63) + 7}\n")
    assert cohort_mod.format_profile_tsv(names, cells) == (
        f"name\tedge_num\tbest\tmass_q\na\t1\t1\t5\nc\t0\t0\t{1 << 63}\nc\t1\t2\t0\nc\t2\t0\t7\n")
    kr = np.array([[0.0, -1.0, 0.1], [-1.0, 0.0, -1.0], [0.1, -1.0, 0.0]])
    text = cohort_mod.format_kr_tsv(names, kr)
    assert text == "name\ta\tb b\tc\na\t0\t-1\t0.10000000000000001\nb b\t-1\t0\t-1\nc\t0.10000000000000001\t-1\t0\n"
