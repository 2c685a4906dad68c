"""The UniFrac distances of a cohort without a GPU (include/epik_amd.h: the UniFrac rule): epik_amd_cohort_unifrac_host
against the rule restated here in numpy, bit for bit; hand-derived values; the properties the rule promises; the errors;
PERMANOVA, PERMDISP and the principal coordinates over a chosen distance; the host test binary, once more under the
sanitizers; the files; and the refusals of the launcher and the driver."""
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod
from test_cohort_cpu import numpy_first, numpy_kr, random_cells, same_bits, tree_case
from test_cohort_gpu import kr_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "epik_amd", "bin")
U64 = np.uint64
METRICS = {"unweighted": 1, "weighted": 2, "generalized": 3}


# ---- the rule, restated ----------------------------------------------------------------------------------------------
def numpy_unifrac_terms(mass, first, branch_length, metric):
    """(num, den, total) of the rule: prefix sums in uint64, a python loop over the branches, S x S float64 array
    operations; num and den as they stand after the last branch, before any of the rule's four cases."""
    metric = METRICS.get(metric, metric)
    mass = np.asarray(mass, dtype=U64)
    s, n = mass.shape
    first = np.asarray(first, dtype=np.int64)
    bl = np.asarray(branch_length, dtype=np.float64)
    prefix = np.zeros((s, n + 1), dtype=U64)
    np.cumsum(mass, axis=1, dtype=U64, out=prefix[:, 1:])
    total = prefix[:, n]
    clade = prefix[:, 1:] - prefix[:, first]
    below = clade - mass
    num, den = np.zeros((s, s), dtype=np.float64), np.zeros((s, s), dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        planes = [clade.astype(np.float64) / total.astype(np.float64)[:, None],
                  below.astype(np.float64) / total.astype(np.float64)[:, None]]
        for b in range(n):
            h = 0.5 * bl[b]
            tn, td = [], []
            for plane in planes:                                   # C, the proximal half, then B, the distal half
                x, y = plane[:, b][:, None], plane[:, b][None, :]
                if metric == 1:
                    tn.append(((x > 0) != (y > 0)).astype(np.float64))
                    td.append(((x > 0) | (y > 0)).astype(np.float64))
                elif metric == 2:
                    tn.append(np.abs(x - y))
                    td.append(x + y)
                else:
                    total_xy = x + y
                    root = np.sqrt(total_xy)
                    tn.append(np.where(total_xy > 0, root * (np.abs(x - y) / total_xy), 0.0))
                    td.append(root)
            num = num + h * (tn[0] + tn[1])
            den = den + h * (td[0] + td[1])
    return num, den, total


def numpy_unifrac(mass, first, branch_length, metric):
    """D of the rule, float64 [S][S]: the four cases in the rule's order, applied last to first."""
    num, den, total = numpy_unifrac_terms(mass, first, branch_length, metric)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(den == 0, 0.0, num / den)
    empty = total == 0
    d[empty, :] = -1.0
    d[:, empty] = -1.0
    np.fill_diagonal(d, 0.0)
    return d


def sparse_cells(rng, num_samples, num_branches, density, empty=None):
    mass = rng.integers(1, 1 << 40, size=(num_samples, num_branches), dtype=np.uint64)
    mass[rng.random(mass.shape) >= density] = 0
    if empty is not None and num_samples > 1:
        mass[empty % num_samples] = 0
    return mass


def assert_mirror(mass, first, bl, what):
    for name, metric in METRICS.items():
        got = cohort_mod.unifrac_host(mass, first, bl, metric)
        want = numpy_unifrac(mass, first, bl, metric)
        assert same_bits(got, want), (what, name, np.argwhere(got.view(U64) != want.view(U64))[:10])
        assert same_bits(got, cohort_mod.unifrac_host(mass, first, bl, name)), (what, name)      # by name as by number


# ---- the host mirror against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("tree_name", ["one", "tree15", "tree2999", "ladder10399"])
@pytest.mark.parametrize("num_samples", [1, 2, 33])
def test_unifrac_host_equals_the_numpy_restatement_on_the_cohort_trees(tree_name, num_samples):
    parent, bl = tree_case(tree_name)
    first = numpy_first(parent)
    rng = np.random.default_rng(2000 + num_samples)
    mass = random_cells(rng, num_samples, len(parent), empty=1)
    assert_mirror(mass, first, bl, tree_name)
    if num_samples > 1:
        got = cohort_mod.unifrac_host(mass, first, bl, "unweighted")
        assert (got[1] == np.where(np.arange(num_samples) == 1, 0.0, -1.0)).all() and (got[:, 1] == got[1]).all()


@pytest.mark.parametrize("num_branches", [7, 999])
@pytest.mark.parametrize("num_samples", [1, 2, 33])
@pytest.mark.parametrize("density", [0.1, 0.7])
def test_unifrac_host_equals_the_numpy_restatement_on_sparse_and_dense_cells(num_branches, num_samples, density):
    parent, bl, first, _ = kr_case(num_branches)
    rng = np.random.default_rng(5)
    mass = sparse_cells(rng, num_samples, num_branches, density)
    assert_mirror(mass, first, bl, (num_branches, num_samples, density))
    if num_samples > 1:
        assert_mirror(sparse_cells(rng, num_samples, num_branches, density, empty=0), first, bl, "an empty sample")


def test_the_sparse_cells_differ_in_clade_presence():
    """Without this `unweighted` would be tested on terms that are all zero (26.5 % of the combinations differ at seed 5)."""
    parent, bl, first, _ = kr_case(999)
    mass = sparse_cells(np.random.default_rng(5), 33, 999, 0.1)
    prefix = np.zeros((33, 1000), dtype=U64)
    np.cumsum(mass, axis=1, dtype=U64, out=prefix[:, 1:])
    present = (prefix[:, 1:] - prefix[:, first.astype(np.int64)]) > 0                     # [S][N]: clade presence
    with_mass = np.flatnonzero(prefix[:, -1] > 0)
    present = present[with_mass]
    pairs = np.triu_indices(len(with_mass), 1)
    differ = present[pairs[0]] != present[pairs[1]]                                      # [pairs][N]
    share = differ.mean()
    print(f"(pair, branch) combinations that differ in clade presence: {share:.3%}")
    assert len(with_mass) >= 30 and share >= 0.10, share


# ---- hand-derived ----------------------------------------------------------------------------------------------------
def test_hand_derived_values_on_a_cherry():
    """Two leaves 0 and 1 (lengths 2 and 4) under the root 2; sample 0 has half its mass on each leaf, sample 1 all on
    leaf 1.  C_0 = (.5, .5, 1), B_0 = (0, 0, 1); C_1 = (0, 1, 1), B_1 = (0, 0, 1); h = (1, 2, 0).
    unweighted: num = 1 * 1, den = 1 * 1 + 2 * 1                                -> 1/3
    weighted:   num = 1 * .5 + 2 * .5 = 1.5, den = 1 * .5 + 2 * 1.5 = 3.5       -> 3/7
    generalized: num = sqrt(.5) * 1 + 2 * sqrt(1.5) * (.5 / 1.5), den = sqrt(.5) + 2 * sqrt(1.5)"""
    first = cohort_mod.first_of([2, 2, -1])
    mass = np.array([[1, 1, 0], [0, 1, 0], [0, 0, 0]], U64)
    bl = [2.0, 4.0, 0.0]
    d = {name: cohort_mod.unifrac_host(mass, first, bl, name) for name in METRICS}
    assert d["unweighted"][0, 1] == 1.0 / 3.0 and d["weighted"][0, 1] == 3.0 / 7.0
    want = (np.sqrt(0.5) + 2.0 * np.sqrt(1.5) / 3.0) / (np.sqrt(0.5) + 2.0 * np.sqrt(1.5))
    assert abs(want - 0.48267282515986) < 1e-13
    assert abs(d["generalized"][0, 1] - want) <= 4 * np.spacing(want), (d["generalized"][0, 1], want)
    for m in d.values():
        assert (m[2] == [-1.0, -1.0, 0.0]).all() and (m[:, 2] == [-1.0, -1.0, 0.0]).all()
        assert m[0, 0] == 0.0 and m[1, 1] == 0.0 and m[0, 1] == m[1, 0]


# ---- the properties the rule promises --------------------------------------------------------------------------------
def test_properties():
    parent, bl, first, _ = kr_case(999)
    rng = np.random.default_rng(17)
    mass = sparse_cells(rng, 12, 999, 0.3, empty=5)
    mass[7] = mass[3]                                               # identical rows
    mass[8] = mass[3] * U64(2)                                      # the same shares, the same presence
    used = np.arange(12) != 5
    for name in METRICS:
        d = cohort_mod.unifrac_host(mass, first, bl, name)
        assert np.array_equal(d.view(U64), d.T.copy().view(U64)) and not d.diagonal().any(), name
        inner = d[np.ix_(used, used)]
        assert (inner >= 0.0).all() and (inner <= 1.0).all(), name
        assert d[3, 7] == 0.0 and d[7, 3] == 0.0, name
        assert (d[5, used] == -1.0).all() and (d[used, 5] == -1.0).all()
    assert cohort_mod.unifrac_host(mass, first, bl, "unweighted")[3, 8] == 0.0
    # weighted's numerator is the KR distance bit for bit; D is that numerator over a denominator computed again
    num, den, total = numpy_unifrac_terms(mass, first, bl, "weighted")
    kr = numpy_kr(mass, first, bl)
    live = np.ix_(used, used)
    off = ~np.eye(11, dtype=bool)
    assert same_bits(num[live][off], kr[live][off]) and same_bits(kr, cohort_mod.kr_host(mass, first, bl))
    again = numpy_unifrac_terms(mass, first, bl, 2)[1]
    weighted = cohort_mod.unifrac_host(mass, first, bl, "weighted")
    assert same_bits(weighted[live][off], (kr[live] / again[live])[off])
    # disjoint supports: the two samples share no clade but the root's, whose length is 0 here
    n = 999
    root_children = np.flatnonzero(parent == n - 1)
    assert len(root_children) >= 2
    left = np.zeros(n, U64)
    right = np.zeros(n, U64)
    a, b = int(root_children[0]), int(root_children[1])
    left[int(first[a]):a + 1] = rng.integers(1, 1 << 30, size=a + 1 - int(first[a]), dtype=np.uint64)
    right[int(first[b]):b + 1] = rng.integers(1, 1 << 30, size=b + 1 - int(first[b]), dtype=np.uint64)
    rootless = bl.copy()
    rootless[n - 1] = 0.0
    disjoint = cohort_mod.unifrac_host(np.stack([left, right]), first, rootless, "unweighted")
    assert disjoint[0, 1] == 1.0 and disjoint[1, 0] == 1.0
    # all lengths zero: den == 0, the distance is 0 by the rule
    for name in METRICS:
        assert not cohort_mod.unifrac_host(mass[:4], first, np.zeros(n), name).any()


# ---- the errors ------------------------------------------------------------------------------------------------------
def test_errors_of_unifrac_host():
    parent, bl, first, _ = kr_case(7)
    mass = random_cells(np.random.default_rng(1), 3, 7)
    for metric in (0, 4):
        with pytest.raises(capi.EpikAmdError) as e:
            cohort_mod.unifrac_host(mass, first, bl, metric)
        assert e.value.code == capi.ERR_INVALID and f"metric = {metric}" in str(e.value)
    with pytest.raises(ValueError):
        cohort_mod.unifrac_host(mass, first, bl, "bray")
    bad_first = first.copy()
    bad_first[2] = 3
    with pytest.raises(capi.EpikAmdError) as e:
        cohort_mod.unifrac_host(mass, bad_first, bl, 1)
    assert e.value.code == capi.ERR_INVALID and "branch 2" in str(e.value) and "first" in str(e.value)
    for value in (-1.0, np.nan, np.inf):
        bad = bl.copy()
        bad[4] = value
        with pytest.raises(capi.EpikAmdError) as e:
            cohort_mod.unifrac_host(mass, first, bad, 3)
        assert e.value.code == capi.ERR_INVALID and "branch 4" in str(e.value)


# ---- the analyses over a chosen distance -----------------------------------------------------------------------------
def _records_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_analyses_take_a_metric_and_default_to_kr():
    parent, bl, first, _ = kr_case(999)
    rng = np.random.default_rng(23)
    mass = sparse_cells(rng, 33, 999, 0.2, empty=4)
    totals = cohort_mod.totals_of(mass)
    labels = np.stack([np.arange(33) % 3, np.arange(33) % 2], axis=1).astype(np.uint32)
    labels[9, 0] = capi.PERMANOVA_MISSING
    matrices = {"kr": cohort_mod.kr_host(mass, first, bl)}
    for name in METRICS:
        matrices[name] = cohort_mod.unifrac_host(mass, first, bl, name)
    for name, matrix in matrices.items():
        got = cohort_mod.permanova_host(mass, first, bl, labels, 99, 7, pairwise=True, metric=name)
        want = cohort_mod.permanova_kr_host(matrix, totals, labels, 99, 7, pairwise=True)
        assert _records_equal(got.records, want.records) and same_bits(got.ssw, want.ssw) and same_bits(got.group_ss, want.group_ss), name
        got = cohort_mod.permdisp_host(mass, first, bl, labels, 99, 7, pairwise=True, metric=name)
        want = cohort_mod.permdisp_kr_host(matrix, totals, labels, 99, 7, pairwise=True)
        assert _records_equal(got.records, want.records) and same_bits(got.stat, want.stat), name
        assert same_bits(got.group_mean, want.group_mean) and same_bits(got.z, want.z), name
        got = cohort_mod.pcoa_host(mass, first, bl, 4, metric=name)
        want = cohort_mod.pcoa_kr_host(matrix, totals, 4)
        assert same_bits(got.mu, want.mu) and same_bits(got.coord, want.coord) and got.info.tobytes() == want.info.tobytes(), name
    # the default is KR, by name and by number, through the entries that were there before
    lib = capi.load()
    assert _records_equal(cohort_mod.permanova_host(mass, first, bl, labels, 99, 7).records,
                          cohort_mod.permanova_host(mass, first, bl, labels, 99, 7, metric=0).records)
    mu, coord, info = np.full(33, np.nan), np.full((33, 4), np.nan), np.zeros(1, dtype=capi.PCOA_INFO)
    capi.check(lib.epik_amd_cohort_pcoa_host(np.ascontiguousarray(mass).ctypes.data, 33, 999, first.ctypes.data, bl.ctypes.data, 4,
                                             mu.ctypes.data, coord.ctypes.data, info.ctypes.data))
    default = cohort_mod.pcoa_host(mass, first, bl, 4)
    assert same_bits(mu, default.mu) and same_bits(coord, default.coord) and info[0].tobytes() == default.info.tobytes()
    assert not same_bits(default.coord, cohort_mod.pcoa_host(mass, first, bl, 4, metric="unweighted").coord)
    with pytest.raises(capi.EpikAmdError) as e:
        cohort_mod.pcoa_host(mass, first, bl, 4, metric=4)
    assert "metric = 4" in str(e.value)


# ---- the host code stand-alone ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_bins():
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    return BIN


@pytest.mark.parametrize("sanitized", [False, True])
def test_host_test_binary_unifrac_is_the_library_s(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    parent, bl, first, _ = kr_case(999)
    mass = sparse_cells(np.random.default_rng(3), 33, 999, 0.1, empty=2)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array(mass.shape, dtype="<u8").tobytes() + mass.tobytes() + np.ascontiguousarray(first, np.uint32).tobytes() +
                 np.ascontiguousarray(bl, np.float64).tobytes())
    for name, metric in METRICS.items():
        run = subprocess.run([binary, "unifrac", str(tmp_path / "out.bin"), str(tmp_path / "in.bin"), str(metric)], capture_output=True,
                             text=True)
        assert run.returncode == 0 and not run.stderr, (name, run.stderr)
        assert (tmp_path / "out.bin").read_bytes() == cohort_mod.unifrac_host(mass, first, bl, metric).tobytes(), name
    run = subprocess.run([binary, "unifrac", str(tmp_path / "o.bin"), str(tmp_path / "in.bin"), "4"], capture_output=True, text=True)
    assert run.returncode == 1 and "metric = 4" in run.stderr


# ---- the files -------------------------------------------------------------------------------------------------------
def test_the_matrix_file_reads_back(tmp_path):
    parent, bl, first, _ = kr_case(7)
    mass = random_cells(np.random.default_rng(4), 5, 7, empty=3)
    names = ["a", "skin 3", "it's", "none", "z.9_-"]
    for name in METRICS:
        d = cohort_mod.unifrac_host(mass, first, bl, name)
        text = cohort_mod.format_unifrac_tsv(names, d)
        assert text.split("\n")[0] == "name\t" + "\t".join(names) and text == cohort_mod.format_kr_tsv(names, d)
        path = tmp_path / f"cohort_unifrac_{name}_x.tsv"
        path.write_bytes(text.encode())
        back_names, back = cohort_mod.read_unifrac_tsv(str(path))
        assert back_names == names and same_bits(back, d)            # %.17g reads back to the same double


def test_the_distance_field_is_written_and_read_back(tmp_path):
    parent, bl, first, _ = kr_case(7)
    mass = random_cells(np.random.default_rng(6), 8, 7, empty=3)
    totals = cohort_mod.totals_of(mass)
    names = [f"s {i}" for i in range(8)]
    labels = (np.arange(8) % 2).astype(np.uint32)[:, None]
    for distance in cohort_mod.DISTANCES:
        tail = "" if distance == "kr" else f"\tdistance={distance}"
        pcoa = cohort_mod.pcoa_host(mass, first, bl, 2, metric=distance)
        text = cohort_mod.format_pcoa_tsv(names, totals, pcoa, distance=distance)
        assert text.split("\n")[0].endswith(f"negative={'%.17g' % pcoa.negative}" + tail)
        (tmp_path / "pcoa.tsv").write_bytes(text.encode())
        back_names, coord, info = cohort_mod.read_pcoa_tsv(str(tmp_path / "pcoa.tsv"))
        assert info.get("distance", "kr") == distance and ("distance" in info) == (distance != "kr") and same_bits(coord, pcoa.coord[totals > 0][:, :info["components"]])
        perm = cohort_mod.permanova_host(mass, first, bl, labels, 19, 3, metric=distance)
        text = cohort_mod.format_permanova_tsv(names, totals, ["site"], [["x", "y"]], labels, 19, 3, False, perm.records, perm.group_ss,
                                               distance=distance)
        assert text.split("\n")[0].endswith("permutations=19 seed=3 pairwise=0" + tail)
        (tmp_path / "permanova.tsv").write_bytes(text.encode())
        columns, rows, groups, info = cohort_mod.read_permanova_tsv(str(tmp_path / "permanova.tsv"))
        assert info.get("distance", "kr") == distance and columns == ["site"] and rows[0][3]["p"] == perm.records[0, 0]["p"]
        disp = cohort_mod.permdisp_host(mass, first, bl, labels, 19, 3, metric=distance)
        text = cohort_mod.format_permdisp_tsv(names, totals, ["site"], [["x", "y"]], labels, 19, 3, False, disp.records, disp.group_mean,
                                              disp.z, distance=distance)
        assert text.split("\n")[0].endswith("permutations=19 seed=3 pairwise=0" + tail)
        (tmp_path / "permdisp.tsv").write_bytes(text.encode())
        columns, rows, groups, distances, info = cohort_mod.read_permdisp_tsv(str(tmp_path / "permdisp.tsv"))
        assert info.get("distance", "kr") == distance and columns == ["site"] and len(distances) == 7
        assert rows[0][3]["p"] == disp.records[0, 0]["p"] and rows[0][3]["eta2"] == disp.records[0, 0]["eta2"]
        assert [g[4] for g in groups] == [disp.group_mean[0][0], disp.group_mean[0][1]]
    # without the keyword: the bytes of before
    pcoa = cohort_mod.pcoa_host(mass, first, bl, 2)
    assert cohort_mod.format_pcoa_tsv(names, totals, pcoa) == cohort_mod.format_pcoa_tsv(names, totals, pcoa, distance="kr")
    assert "distance=" not in cohort_mod.format_pcoa_tsv(names, totals, pcoa)
    (tmp_path / "bad.tsv").write_text("# epik_amd pcoa v1  samples=8 used=7 components=2 sweeps=3 converged=1 negative=0\tdistance=bray\n")
    with pytest.raises(ValueError):
        cohort_mod.read_pcoa_tsv(str(tmp_path / "bad.tsv"))


# ---- the refusals, before anything is opened -------------------------------------------------------------------------
def test_the_launcher_checks_and_passes_the_flags():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=4, max_ram=None, gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw, cohort=True)
    argv = epik.driver_command(**kw, cohort=True, cohort_unifrac="all", cohort_distance="unweighted", cohort_pcoa=True)
    assert argv == default[:-1] + ["--cohort-pcoa", "--cohort-unifrac", "all", "--cohort-distance", "unweighted"] + default[-1:]
    assert "--cohort-unifrac" not in default and "--cohort-distance" not in default
    both = epik.driver_command(**kw, cohort=True, cohort_unifrac="weighted,unweighted", cohort_permanova="f.tsv", cohort_distance="kr",
                               strand="both", taxonomy="t.tsv", cohort_epca=True)
    assert all(flag in both for flag in ("--cohort-unifrac", "weighted,unweighted", "--cohort-distance", "--strand", "--taxonomy"))
    for bad in (dict(cohort_unifrac="all"), dict(cohort=True, cohort_unifrac="unweighted,bray"), dict(cohort=True, cohort_unifrac="kr"),
                dict(cohort=True, cohort_unifrac="weighted,weighted"), dict(cohort=True, cohort_unifrac=""),
                dict(cohort=True, cohort_distance="weighted"), dict(cohort=True, cohort_unifrac="all", cohort_distance="weighted"),
                dict(cohort=True, cohort_pcoa=True, cohort_distance="bray")):
        with pytest.raises(click.UsageError):
            epik.driver_command(**kw, **bad)
    with pytest.raises(click.UsageError) as e:
        epik.driver_command(**kw, cohort=True, cohort_unifrac="unweighted,bray")
    assert "bray" in str(e.value.message)
    me = os.path.join(ROOT, "epik.py")
    out = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort-unifrac" in out.stdout and "--cohort-distance" in out.stdout
    run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, "--cohort-unifrac", "all", me], capture_output=True, text=True)
    assert run.returncode == 2 and "--cohort" in run.stderr, (run.stdout, run.stderr)
    run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, "--cohort", "--cohort-distance", "weighted", me],
                         capture_output=True, text=True)
    assert run.returncode == 2 and "--cohort-distance needs" in run.stderr, (run.stdout, run.stderr)


def test_epik_dna_refuses_the_flags_before_anything_is_opened(host_bins, tmp_path):
    driver = os.path.join(host_bins, "epik-dna")
    base = [driver, "-d", str(tmp_path / "no.ekdb"), "-q", str(tmp_path / "no.list"), "-o", str(tmp_path / "out")]
    for extra, words in ((["--cohort-unifrac", "all"], ("--cohort-unifrac needs --cohort",)),
                         (["--cohort", "--cohort-unifrac", "unweighted,bray"], ("'bray'", "UniFrac")),
                         (["--cohort", "--cohort-unifrac", "weighted,weighted"], ("'weighted'", "twice")),
                         (["--cohort", "--cohort-unifrac", ""], ("''",)),
                         (["--cohort", "--cohort-distance", "weighted"], ("--cohort-distance needs", "--cohort-pcoa")),
                         (["--cohort", "--cohort-unifrac", "all", "--cohort-distance", "weighted"], ("--cohort-distance needs",)),
                         (["--cohort", "--cohort-pcoa", "--cohort-distance", "bray"], ("'bray'", "--cohort-distance"))):
        run = subprocess.run(base + extra, capture_output=True, text=True)
        text = run.stdout + run.stderr
        assert run.returncode != 0 and all(word in text for word in words), (extra, text)
        assert "no.ekdb" not in text and not (tmp_path / "out").exists(), (extra, text)     # refused before the database is opened
    assert "--cohort-unifrac" in subprocess.run([driver, "--help"], capture_output=True, text=True).stdout
